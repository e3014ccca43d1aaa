"""The fused BatchNorm / GroupNorm kernels (csrc/bn_relu.hip, csrc/gn_relu.hip) against the float64 reference of
tests/_norm_ref.py at the smallest shapes where each piece of index arithmetic can go wrong, at the edge values, and on the
forms only the C ABI reaches. Every tolerance is the bound derived in the docstring of _norm_ref.py; the generator keeps
every ReLU decision away from rounding, so the mask, dx and d_residual are compared at every element, with none forgiven."""
import copy

import numpy as np
import pytest
import torch

import _norm_ref as N
from gga_amd import _lib
from gga_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def within(got, ref, bound, what, sel=None):
    """|got - ref| <= bound at every element (a NaN fails)."""
    got = (host(got) if torch.is_tensor(got) else np.asarray(got)).astype(np.float64)
    if sel is not None:
        got = got.reshape(-1, ref.shape[-1])[sel]
    got = got.reshape(ref.shape)
    bound = np.broadcast_to(bound, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)), ref.shape)
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements beyond the bound; worst at {i}: got {got[i]!r}, '
                             f'reference {ref[i]!r}, error {err[i]:.3e}, bound {bound[i]:.3e}')


def unpack_mask(bits, n_elems):
    """gga_bn_relu_fwd's mask words [float4 index / 64][component] -> bool per element of the [rows, C] matrix."""
    w = host(bits).view(np.uint64).reshape(-1, 4)
    b = (w[:, None, :] >> np.arange(64, dtype=np.uint64)[None, :, None]) & np.uint64(1)          # [word, lane, component]
    return b.reshape(-1)[:n_elems].astype(bool)


# --------------------------------------------------------------------------------------------------- BatchNorm via bn_act
def bn_module(case, gamma=None, beta=None, dims=1):
    C = case['C']
    bn = (torch.nn.BatchNorm2d if dims == 2 else torch.nn.BatchNorm1d)(C, eps=case['eps'], momentum=case['momentum']).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(dev(case['gamma'] if gamma is None else gamma)), bn.bias.copy_(dev(case['beta'] if beta is None else beta))
        bn.running_mean.copy_(dev(case['running_mean'])), bn.running_var.copy_(dev(case['running_var']))
    return bn.train(case['training'])


def shaped(a, shape4):
    """[rows, C] memory as the tensor the op takes: 2-D, or the channels-last [B, C, H, W] view of the same memory."""
    t = dev(a)
    if t is None or shape4 is None:
        return t
    B, C, H, W = shape4
    return t.view(B, H, W, C).permute(0, 3, 1, 2)


def run_bn_act(case, shape4=None, x=None, bn=None):
    bn = bn_module(case, dims=2 if shape4 else 1) if bn is None else bn
    x = shaped(case['x'] if x is None else x, shape4).requires_grad_(True)
    r = shaped(case['residual'], shape4)
    r = r.requires_grad_(True) if r is not None else None
    y = F.bn_act(x, bn, relu=case['relu'], residual=r)
    assert 'BNAct' in type(y.grad_fn).__name__ and y.stride() == x.stride()
    saved, bits = y.grad_fn.saved_tensors[2:4]
    out = dict(y=y.detach(), mean=saved[:case['C']].clone(), invstd=saved[case['C']:].clone(),
               mask=unpack_mask(bits, case['x'].size).reshape(case['x'].shape) if case['relu'] else None)
    y.backward(shaped(case['dy'], shape4))
    rows = lambda t: t.permute(0, 2, 3, 1) if t.dim() == 4 else t
    out.update(y=rows(out['y']), dx=rows(x.grad), d_residual=rows(r.grad) if r is not None else None, d_gamma=bn.weight.grad,
               d_beta=bn.bias.grad, running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone())
    return out


def check_bn(out, case, f, b, sel=None, what='bn'):
    fb, bb = f['bounds'], b['bounds']
    for k in ('mean', 'invstd', 'running_mean', 'running_var'):
        within(out[k], f[k], fb[k], f'{what} {k}')
    if not case['training']:
        assert np.array_equal(host(out['running_mean']), case['running_mean']) and np.array_equal(host(out['running_var']), case['running_var'])
    within(out['y'], f['y'], fb['y'], f'{what} y', sel)
    if case['relu'] and out.get('mask') is not None:
        assert np.array_equal(out['mask'], f['mask']), f'{what}: {(out["mask"] != f["mask"]).sum()} mask bits differ'
        assert np.array_equal(host(out['y']).reshape(f['mask'].shape) > 0, f['mask'])
    within(out['dx'], b['dx'], bb['dx'], f'{what} dx', sel)
    within(out['d_gamma'], b['d_gamma'], bb['d_gamma'], f'{what} d_gamma')
    within(out['d_beta'], b['d_beta'], bb['d_beta'], f'{what} d_beta')
    if out.get('d_residual') is not None:          # dy * mask, bit for bit
        assert np.array_equal(host(out['d_residual']).reshape(case['dy'].shape), case['dy'] * f['mask'].astype(np.float32))


_CASES = {}


def bn_case(n, C, relu, res, training=True, **kw):
    """One generated case and its float64 reference, computed once and shared (nothing modifies them)."""
    key = (n, C, relu, res, training, tuple(sorted(kw.items())))
    if key not in _CASES:
        case = N.make_bn_case(n, C, seed=n + C, relu=relu, residual=res, training=training, **kw)
        f = N.bn_case_forward(case)
        _CASES[key] = (case, f, N.bn_backward(case['x'], case['dy'], case['gamma'], f))
    return _CASES[key]


@pytest.mark.parametrize('relu,res', N.BN_MODES)
@pytest.mark.parametrize('shape', N.BN_SHAPES[:-1] + [(3, 8, 5, 7), N.BN_CAPPED])
def test_bn_act_training_vs_float64(shape, relu, res):
    """Saved statistics, running buffers, y, the mask bits, dx, d_residual, d_gamma and d_beta of ``bn_act`` in training mode.
    (1, 4), (2, 8): one channel quad; (3, 1024): the widest C; 63 / 64 / 65 x 16: around a partial mask word; 511 / 512 / 513
    x 4: around one workgroup's first batch of loads; a 4-D channels-last tensor; 2 * 132 * 125 x 128: the grid capped at
    BN_MAX_BLOCKS, a second partial batch."""
    shape4 = shape if len(shape) == 4 else None
    n, C = (shape[0] * shape[2] * shape[3], shape[1]) if shape4 else shape
    case, f, b = bn_case(n, C, relu, res)
    check_bn(run_bn_act(case, shape4), case, f, b, what=f'bn_act {shape} relu={relu} res={res}')


def test_bn_act_past_the_f32_run_flush_vs_float64():
    """524293 x 64: 80 float4 more than 2048 workgroups x 256 threads x 16 read in one f32 run, so the first threads flush
    a full run into float64 and start a second one. Without ReLU; statistics, running buffers, d_gamma and d_beta in full,
    y and dx on the first row, the last row and 1000 fixed random rows."""
    n, C = N.BN_FLUSH
    case = N.make_bn_case(n, C, seed=3, relu=False)
    sel = np.concatenate([[0, n - 1], np.random.default_rng(11).choice(n, 1000, replace=False)])
    f = N.bn_case_forward(case, rows=sel)
    b = N.bn_backward(case['x'], case['dy'], case['gamma'], f, mask=np.ones((n, C), bool))
    check_bn(run_bn_act(case), case, f, b, sel=sel, what='bn_act 524293x64')


@pytest.mark.parametrize('relu,res', [(True, True), (False, False)])
@pytest.mark.parametrize('shape', [(65, 16), (513, 4)])
def test_bn_act_evaluation_mode_vs_float64(shape, relu, res):
    """Running statistics in forward (no_grad) and under autograd: dx = gamma * invstd * g, the buffers untouched."""
    case, f, b = bn_case(*shape, relu, res, training=False)
    bn = bn_module(case)
    with torch.no_grad():
        y = F.bn_act(dev(case['x']), bn, relu=relu, residual=dev(case['residual']))
    within(y, f['y'], f['bounds']['y'], 'eval y (no_grad)')
    assert int(bn.num_batches_tracked) == 0
    check_bn(run_bn_act(case, bn=bn), case, f, b, what=f'bn_act eval {shape}')
    assert int(bn.num_batches_tracked) == 0


def test_bn_relu_cat_unequal_blocks_vs_float64():
    """Three blocks of 8, 16 and 4 channels written into / read from column blocks of one [105, 28] map."""
    B, H, W = 3, 5, 7
    chans = (8, 16, 4)
    cases = [bn_case(B * H * W, c, True, False) for c in chans]
    bns = [bn_module(c[0], dims=2) for c in cases]
    xs = [shaped(c[0]['x'], (B, ch, H, W)).requires_grad_(True) for c, ch in zip(cases, chans)]
    y = F.bn_relu_cat(xs, bns)
    assert 'BNAct' in type(y.grad_fn).__name__ and y.shape == (B, sum(chans), H, W)
    n, nb = B * H * W, len(chans)
    st = y.grad_fn.saved_tensors                    # the n inputs, gammas, saved statistics and mask bits, block by block
    saved, masks = [t.clone() for t in st[2 * nb:3 * nb]], [unpack_mask(t, n * ch).reshape(n, ch) for t, ch in zip(st[3 * nb:], chans)]
    y.backward(shaped(np.concatenate([c[0]['dy'] for c in cases], 1), (B, sum(chans), H, W)))
    off = 0
    for i, ((case, f, b), bn, x, ch) in enumerate(zip(cases, bns, xs, chans)):
        out = dict(y=y.detach().permute(0, 2, 3, 1).reshape(-1, sum(chans))[:, off:off + ch], dx=x.grad.permute(0, 2, 3, 1),
                   mean=saved[i][:ch], invstd=saved[i][ch:], mask=masks[i], d_gamma=bn.weight.grad, d_beta=bn.bias.grad,
                   running_mean=bn.running_mean, running_var=bn.running_var)
        check_bn(out, case, f, b, what=f'bn_relu_cat block at {off}')
        off += ch


# --------------------------------------------------------------------------------------------------- BatchNorm via the C ABI
def raw_ws(n, C):
    L = _lib.lib()
    return F._workspace('bn', L.gga_bn_relu_workspace_bytes(n, C), torch.device(DEV))


def raw_fwd(case, x=None, y=None, y_ptr=None, y_stride=None, partials=None, relu=None, training=None):
    """gga_bn_relu_fwd on device copies of the case's operands -> dict of tensors."""
    L = _lib.lib()
    n, C = case['n'], case['C']
    relu = int(case['relu']) if relu is None else relu
    t = {k: dev(case[k]) for k in ('x', 'residual', 'gamma', 'beta', 'running_mean', 'running_var')}
    if x is not None:
        t['x'] = x
    if y is None:
        y = torch.empty(n, C, device=DEV)
    t.update(y=y, saved=torch.empty(2 * C, device=DEV),
             bits=torch.zeros(L.gga_bn_relu_mask_bytes(n, C), dtype=torch.uint8, device=DEV) if relu else None)
    ws = raw_ws(n, C)
    rc = L.gga_bn_relu_fwd(F._p(t['x']), F._p(t['residual']), F._p(t['gamma']), F._p(t['beta']), F._p(t['running_mean']),
                           F._p(t['running_var']), n, C, case['eps'], case['momentum'],
                           int(case['training'] if training is None else training), relu,
                           y.data_ptr() if y_ptr is None else y_ptr, C if y_stride is None else y_stride, F._p(t['bits']),
                           F._p(t['saved']), F._p(partials), 0 if partials is None else int(partials.shape[0]), None, F._p(ws),
                           ws.numel(), F._stream())
    assert rc == 0, rc
    return t


def raw_bwd(case, saved, mask_bits, relu, grad_y=None, grad_ptr=None, grad_stride=None, want_res=True):
    L = _lib.lib()
    n, C = case['n'], case['C']
    gy = dev(case['dy']) if grad_y is None else grad_y
    x, gamma = dev(case['x']), dev(case['gamma'])
    o = dict(dx=torch.empty(n, C, device=DEV), d_residual=torch.empty(n, C, device=DEV) if want_res else None,
             d_gamma=torch.empty(C, device=DEV), d_beta=torch.empty(C, device=DEV))
    ws = raw_ws(n, C)
    rc = L.gga_bn_relu_bwd(gy.data_ptr() if grad_ptr is None else grad_ptr, C if grad_stride is None else grad_stride, F._p(x),
                           F._p(mask_bits), F._p(gamma), F._p(saved), n, C, relu, int(case['training']), F._p(o['dx']),
                           F._p(o['d_residual']), F._p(o['d_gamma']), F._p(o['d_beta']), None, F._p(ws), ws.numel(), F._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return o


SENTINEL = -7.25


@pytest.mark.parametrize('shape', [(65, 16), (513, 4)])
def test_raw_forward_into_and_backward_from_a_column_block_of_a_wider_buffer(shape):
    """``y_row_stride > C``: y lands in columns C .. 2C of a [rows, 3C + 4] buffer prefilled with a sentinel and the other
    columns still hold it; ``grad_y_row_stride > C``: the gradient is read from such a block."""
    case, f, b = bn_case(*shape, True, True)
    n, C = shape
    wide = torch.full((n, 3 * C + 4), SENTINEL, device=DEV)
    t = raw_fwd(case, y=wide, y_ptr=wide.data_ptr() + 4 * C, y_stride=3 * C + 4)
    torch.cuda.synchronize()
    within(wide[:, C:2 * C], f['y'], f['bounds']['y'], 'strided y')
    assert bool((wide[:, :C] == SENTINEL).all()) and bool((wide[:, 2 * C:] == SENTINEL).all())
    assert np.array_equal(unpack_mask(t['bits'], n * C).reshape(n, C), f['mask'])
    gwide = torch.full((n, 2 * C + 8), float('nan'), device=DEV)          # a read outside the block poisons the sums
    gwide[:, C + 8:] = dev(case['dy'])
    o = raw_bwd(case, t['saved'], t['bits'], 1, grad_y=gwide, grad_ptr=gwide.data_ptr() + 4 * (C + 8), grad_stride=2 * C + 8)
    out = dict(o, y=wide[:, C:2 * C], mean=t['saved'][:C], invstd=t['saved'][C:], running_mean=t['running_mean'],
               running_var=t['running_var'])
    check_bn(out, case, f, b, what=f'strided {shape}')


@pytest.mark.parametrize('n_partials', [1, 127, 128, 129, 300])
def test_raw_forward_and_stats_from_float64_partials(n_partials):
    """``partials != NULL``: the per-channel sums of x and x^2 computed here in float64 over ``n_partials`` row groups (the
    fold strides by 128 groups). gga_bn_relu_fwd and gga_bn_stats must both reach the reference from them; the bounds are
    those of statistics that carry no float32 run (``run=1``)."""
    n, C = 513, 8
    case = N.make_bn_case(n, C, seed=21, relu=True)
    f = N.bn_case_forward(case, run=1)
    x64 = case['x'].astype(np.float64)
    part = dev(N.partial_sums(x64, x64 * x64, n_partials))
    t = raw_fwd(case, partials=part)
    torch.cuda.synchronize()
    for k, got in (('mean', t['saved'][:C]), ('invstd', t['saved'][C:]), ('running_mean', t['running_mean']),
                   ('running_var', t['running_var']), ('y', t['y'])):
        within(got, f[k], f['bounds'][k], f'fwd from {n_partials} partials: {k}')
    assert np.array_equal(unpack_mask(t['bits'], n * C).reshape(n, C), f['mask'])
    # gga_bn_stats, partials in columns 4 .. 4 + C of rows 2 C wide
    L = _lib.lib()
    wide = torch.full((n_partials, 2, 2 * C), float('nan'), dtype=torch.float64, device=DEV)
    wide[:, :, 4:4 + C] = part
    rm, rv = dev(case['running_mean']), dev(case['running_var'])
    saved, ss = torch.empty(2 * C, device=DEV), torch.empty(2 * C, device=DEV)
    rc = L.gga_bn_stats(None, F._p(t['gamma']), F._p(t['beta']), F._p(rm), F._p(rv), n, C, case['eps'],
                        case['momentum'], 1, F._p(saved), F._p(ss), F._p(wide), n_partials, 2 * C, 4, None, 0, F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(saved, t['saved']) and torch.equal(rm, t['running_mean']) and torch.equal(rv, t['running_var'])
    sc = f['scale']
    e_sc = np.abs(case['gamma']) * f['bounds']['invstd'] + N.SAFETY * N.U * np.abs(sc)
    within(ss[:C], sc, e_sc, 'scale from partials')
    sh = case['beta'] - f['mean'] * sc
    e_sh = np.abs(sc) * f['bounds']['mean'] + np.abs(f['mean']) * e_sc + N.SAFETY * N.U * (np.abs(f['mean'] * sc) + np.abs(sh))
    within(ss[C:], sh, e_sh, 'shift from partials')


@pytest.mark.parametrize('n_partials', [1, 129])
def test_raw_backward_from_float64_partials(n_partials):
    """gga_bn_relu_bwd_partials: the masked gradient and float64 partial sums of g and g * x_hat, as a convolution's
    backward-data epilogue leaves them."""
    n, C = 513, 8
    case = N.make_bn_case(n, C, seed=22, relu=True)
    f = N.bn_case_forward(case, run=1)
    b = N.bn_backward(case['x'], case['dy'], case['gamma'], f)
    L = _lib.lib()
    part = dev(N.partial_sums(b['g_all'], b['g_all'] * b['xhat_all'], n_partials))
    saved = dev(np.concatenate([f['mean'], f['invstd']]).astype(np.float32))
    g, x, gamma = dev(b['g_all'].astype(np.float32)), dev(case['x']), dev(case['gamma'])
    dx, dg, db = torch.empty(n, C, device=DEV), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ws = raw_ws(n, C)
    rc = L.gga_bn_relu_bwd_partials(F._p(g), C, F._p(x), F._p(gamma), F._p(saved), n, C, 1, F._p(part), n_partials, F._p(dx),
                                    F._p(dg), F._p(db), None, F._p(ws), ws.numel(), F._stream())
    assert rc == 0
    torch.cuda.synchronize()
    for k, got in (('dx', dx), ('d_gamma', dg), ('d_beta', db)):
        within(got, b[k], b['bounds'][k], f'bwd from {n_partials} partials: {k}')


@pytest.mark.parametrize('shape', [(65, 16), (513, 4)])
def test_raw_backward_with_the_mask_recomputed_from_scale_and_shift(shape):
    """``relu == 2``: no mask bits, the decision is recomputed from x and the scale / shift table of gga_bn_stats. It must be
    the float64 reference's decision (d_residual = dy * mask bit for bit), hence the same dx, d_gamma and d_beta."""
    case, f, b = bn_case(*shape, True, False)
    n, C = shape
    L = _lib.lib()
    t = {k: dev(case[k]) for k in ('x', 'gamma', 'beta', 'running_mean', 'running_var')}
    saved, ss = torch.empty(2 * C, device=DEV), torch.empty(2 * C, device=DEV)
    ws = raw_ws(n, C)
    rc = L.gga_bn_stats(F._p(t['x']), F._p(t['gamma']), F._p(t['beta']), F._p(t['running_mean']), F._p(t['running_var']), n, C,
                        case['eps'], case['momentum'], 1, F._p(saved), F._p(ss), None, 0, 0, 0, F._p(ws), ws.numel(), F._stream())
    assert rc == 0
    o = raw_bwd(case, saved, ss, 2)
    within(saved[:C], f['mean'], f['bounds']['mean'], 'stats mean')
    within(saved[C:], f['invstd'], f['bounds']['invstd'], 'stats invstd')
    assert np.array_equal(host(o['d_residual']), case['dy'] * f['mask'].astype(np.float32))
    for k in ('dx', 'd_gamma', 'd_beta'):
        within(o[k], b[k], b['bounds'][k], f'relu == 2: {k}')


@pytest.mark.parametrize('shape', [(6, 12), (5, 1028), (3, 8, 5, 7)])
def test_bn_act_shapes_the_kernels_do_not_take_are_the_eager_ops(shape):
    """C = 12 (C / 4 does not divide 256), C = 1028 (beyond 1024), a 4-D tensor in NCHW memory: the eager composition, same
    values and gradients, and no BNAct node."""
    g = torch.Generator().manual_seed(4)
    C = shape[1]
    bn = (torch.nn.BatchNorm2d if len(shape) == 4 else torch.nn.BatchNorm1d)(C, eps=1e-3, momentum=0.01).to(DEV)
    twin = copy.deepcopy(bn)
    x = (torch.randn(*shape, generator=g) * 2 + 0.5).to(DEV)
    r, dy = torch.randn(*shape, generator=g).to(DEV), torch.randn(*shape, generator=g).to(DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y = F.bn_act(xa, bn, relu=True, residual=r)
    assert 'BNAct' not in type(y.grad_fn).__name__
    ref = torch.relu(twin(xb) + r)
    assert torch.equal(y, ref)
    y.backward(dy), ref.backward(dy)
    assert torch.equal(xa.grad, xb.grad) and torch.equal(bn.weight.grad, twin.weight.grad) and torch.equal(bn.bias.grad, twin.bias.grad)
    assert torch.equal(bn.running_mean, twin.running_mean) and torch.equal(bn.running_var, twin.running_var)


# --------------------------------------------------------------------------------------------------- GroupNorm
def gn_module(case, gamma=None, beta=None):
    gn = torch.nn.GroupNorm(case['groups'], case['shape'][1], eps=case['eps']).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(dev(case['gamma'] if gamma is None else gamma)), gn.bias.copy_(dev(case['beta'] if beta is None else beta))
    return gn


def run_gn_act(case, x=None, gn=None):
    gn = gn_module(case) if gn is None else gn
    x = shaped(case['x'] if x is None else x, case['shape']).requires_grad_(True)
    y = F.gn_act(x, gn, relu=case['relu'])
    assert 'GNAct' in type(y.grad_fn).__name__ and y.is_contiguous(memory_format=torch.channels_last)
    stat = y.grad_fn.saved_tensors[2].clone()
    y.backward(shaped(case['dy'], case['shape']))
    B, C, H, W = case['shape']
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(B, H * W, C)
    return dict(y=rows(y), dx=rows(x.grad), mean=stat[:, :, 0], invstd=stat[:, :, 1], d_gamma=gn.weight.grad, d_beta=gn.bias.grad)


def check_gn(out, case, f, b, what='gn'):
    for k in ('mean', 'invstd', 'y'):
        within(out[k], f[k], f['bounds'][k], f'{what} {k}')
    if case['relu']:
        assert np.array_equal(host(out['y']) > 0, f['mask']), f'{what}: ReLU decisions differ'
    for k in ('dx', 'd_gamma', 'd_beta'):
        within(out[k], b[k], b['bounds'][k], f'{what} {k}')


def gn_case(shape, relu, **kw):
    key = ('gn', shape, relu, tuple(sorted(kw.items())))
    if key not in _CASES:
        B, C, G, H, W = shape
        case = N.make_gn_case(B, C, G, H, W, seed=C + H, relu=relu, **kw)
        f = N.gn_forward(case['x'], case['gamma'], case['beta'], G, case['eps'], relu)
        _CASES[key] = (case, f, N.gn_backward(case['x'], case['dy'], case['gamma'], f))
    return _CASES[key]


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('shape', N.GN_SHAPES + [N.GN_FLUSH])
def test_gn_act_vs_float64(shape, relu):
    """(B, C, G, H, W). (1, 4, 1, 1, 1): the smallest; (2, 8, 2, 1, 3): fewer rows than the 64 chunks; 63 / 64 / 65 rows with
    groups of one quad and one group of all channels; (1, 1024, 32, 3, 5): the widest C; (1, 256, 32, 96, 96): 36 rows per
    thread, past the flush of the f32 run into float64."""
    case, f, b = gn_case(shape, relu)
    check_gn(run_gn_act(case), case, f, b, what=f'gn_act {shape} relu={relu}')


@pytest.mark.parametrize('C,G', [(12, 3), (16, 8)])
def test_gn_act_shapes_the_kernels_do_not_take_are_the_eager_ops(C, G):
    """C = 12 and two channels per group: the eager composition, same values and gradients, and no GNAct node."""
    g = torch.Generator().manual_seed(5)
    gn = torch.nn.GroupNorm(G, C).to(DEV)
    twin = copy.deepcopy(gn)
    x = (torch.randn(2, C, 5, 3, generator=g) * 2 + 0.5).to(DEV).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(2, C, 5, 3, generator=g).to(DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y = F.gn_act(xa, gn, relu=True)
    assert 'GNAct' not in type(y.grad_fn).__name__
    ref = torch.relu(twin(xb))
    assert torch.equal(y, ref)
    y.backward(dy), ref.backward(dy)
    assert torch.equal(xa.grad, xb.grad) and torch.equal(gn.weight.grad, twin.weight.grad) and torch.equal(gn.bias.grad, twin.bias.grad)


# --------------------------------------------------------------------------------------------------- edge values
def test_bn_constant_channel():
    """Variance exactly 0 (every sum of the run is exact for 2.5): invstd is 1 / sqrt(eps) to the bit, y = beta within the
    bound, dx finite and within the bound."""
    case = N.make_bn_case(65, 16, seed=31, relu=False)
    case['x'][:, 3] = 2.5
    f = N.bn_case_forward(case)
    b = N.bn_backward(case['x'], case['dy'], case['gamma'], f)
    assert f['var'][3] == 0.0
    out = run_bn_act(case)
    assert float(out['invstd'][3]) == _top(case['eps'])
    assert float(out['mean'][3]) == 2.5 and bool(torch.isfinite(out['dx']).all())
    within(out['y'][:, 3], np.full(65, float(case['beta'][3])), f['bounds']['y'][:, 3], 'y of the constant channel')
    check_bn(out, case, f, b, what='bn constant channel')


def test_gn_constant_group():
    B, C, G, H, W = N.GN_COND
    case = N.make_gn_case(B, C, G, H, W, seed=31, relu=False)
    case['x'][1, :, 8:12] = 2.5
    f = N.gn_forward(case['x'], case['gamma'], case['beta'], G, case['eps'], False)
    b = N.gn_backward(case['x'], case['dy'], case['gamma'], f)
    assert f['var'][1, 2] == 0.0
    out = run_gn_act(case)
    assert float(out['invstd'][1, 2]) == _top(case['eps'])
    assert float(out['mean'][1, 2]) == 2.5 and bool(torch.isfinite(out['dx']).all())
    check_gn(out, case, f, b, what='gn constant group')


def _zero_gamma(case):
    """gamma = 0 in channels 0, 1, 2 with beta < 0, = 0, > 0 (set after the generator ran: the other channels' ReLU margins
    do not depend on these)."""
    gamma, beta = case['gamma'].copy(), case['beta'].copy()
    gamma[:3] = 0.0
    beta[:3] = (-0.3, 0.0, 0.3)
    return dict(case, gamma=gamma, beta=beta)


def _check_zero_gamma(out):
    """Channels 0, 1, 2 of a BatchNorm with gamma = 0: exact where the reference is exact."""
    y, dx = host(out['y'])[..., :3], host(out['dx'])[..., :3]
    assert (y[..., 0] == 0).all() and (y[..., 1] == 0).all() and (y[..., 2] == np.float32(0.3)).all()
    assert (dx == 0).all()                                               # gamma * invstd = 0 whatever the mask
    dg, db = host(out['d_gamma']), host(out['d_beta'])
    assert (dg[:2] == 0).all() and (db[:2] == 0).all()                 # beta <= 0: the mask is 0 everywhere, strict >
    assert db[2] != 0 and dg[2] != 0                                     # beta > 0: every element is live


def test_bn_zero_gamma():
    case = _zero_gamma(N.make_bn_case(65, 16, seed=32, relu=True, residual=False))
    f = N.bn_case_forward(case)
    b = N.bn_backward(case['x'], case['dy'], case['gamma'], f)
    out = run_bn_act(case)
    assert not out['mask'][:, :2].any() and out['mask'][:, 2].all()
    _check_zero_gamma(out)
    check_bn(out, case, f, b, what='bn gamma == 0')


def test_gn_zero_gamma():
    B, C, G, H, W = N.GN_COND
    case = _zero_gamma(N.make_gn_case(B, C, G, H, W, seed=32, relu=True))
    f = N.gn_forward(case['x'], case['gamma'], case['beta'], G, case['eps'], True)
    b = N.gn_backward(case['x'], case['dy'], case['gamma'], f)
    out = run_gn_act(case)
    y, dx = host(out['y'])[..., :3], host(out['dx'])[..., :3]
    assert (y[..., 0] == 0).all() and (y[..., 1] == 0).all() and (y[..., 2] == np.float32(0.3)).all()
    # dx of a GroupNorm channel with gamma = 0 still carries the group's mean terms: only the reference bounds it
    dg, db = host(out['d_gamma']), host(out['d_beta'])
    assert (dg[:2] == 0).all() and (db[:2] == 0).all() and db[2] != 0 and dg[2] != 0
    check_gn(out, case, f, b, what='gn gamma == 0')


def _top(eps):
    """invstd of a variance of exactly 0, as float32."""
    return float(np.float32(1.0 / np.sqrt(np.float64(np.float32(eps)))))


@pytest.mark.parametrize('ch', [6, 5])
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_bn_non_finite_input_stays_in_its_channel(bad, relu, ch):
    """A NaN / +Inf at row 5 of channel ``ch`` (gamma > 0 in channel 6, < 0 in channel 5). Every other channel equals the
    clean run bit for bit in every output. In the channel itself the kernels' specified behaviour ("Domain of
    the normalisation kernels") is asserted:
    * the mean and running_mean are non-finite; the variance (NaN, or Inf - Inf) is clamped at 0, so invstd is
      1 / sqrt(eps) and running_var stays finite;
    * dx is non-finite at every element and d_gamma is non-finite;
    * without ReLU y is non-finite at every element and d_beta, which does not depend on x, is the clean run's;
    * with ReLU the decision ``pre > 0`` is false for a NaN and ``fmaxf(NaN, 0)`` is 0 (torch.relu would keep the NaN): a NaN
      input gives mask 0 and y = 0 in the whole channel; an Inf input gives pre = -Inf (gamma > 0: mask 0, y = 0) or +Inf
      (gamma < 0: mask 1, y = +Inf) except at the Inf element itself, where pre = Inf - Inf is NaN. d_residual = dy * mask."""
    case = N.make_bn_case(65, 16, seed=33, relu=relu, residual=True)
    assert (case['gamma'][ch] > 0) == (ch == 6)
    clean = run_bn_act(case)
    x = case['x'].copy()
    x[5, ch] = bad
    out = run_bn_act(case, x=x)
    other = np.arange(16) != ch
    for k in ('y', 'dx', 'd_residual') + (('mask',) if relu else ()):
        a, c = np.asarray(out[k] if k == 'mask' else host(out[k])).reshape(65, 16), np.asarray(clean[k] if k == 'mask' else host(clean[k])).reshape(65, 16)
        assert np.array_equal(a[:, other], c[:, other]), k
    for k in ('mean', 'invstd', 'running_mean', 'running_var', 'd_gamma', 'd_beta'):
        assert np.array_equal(host(out[k])[other], host(clean[k])[other]), k
    assert not np.isfinite(host(out['mean'])[ch]) and not np.isfinite(host(out['running_mean'])[ch])
    assert float(out['invstd'][ch]) == _top(case['eps']) and np.isfinite(host(out['running_var'])[ch])
    assert not np.isfinite(host(out['dx'])[:, ch]).any() and not np.isfinite(host(out['d_gamma'])[ch])
    y, dres = host(out['y'])[:, ch], host(out['d_residual'])[:, ch]
    if not relu:
        assert not np.isfinite(y).any()
        assert np.array_equal(dres, case['dy'][:, ch]) and host(out['d_beta'])[ch] == host(clean['d_beta'])[ch]
        return
    live = np.zeros(65, bool)
    if np.isinf(bad) and case['gamma'][ch] < 0:
        live[:] = True
        live[5] = False
    assert np.array_equal(out['mask'][:, ch], live)
    assert np.array_equal(y, np.where(live, np.float32(np.inf), np.float32(0)))
    assert np.array_equal(dres, case['dy'][:, ch] * live.astype(np.float32))
    assert np.isfinite(host(out['d_beta'])[ch]) and (live.any() or host(out['d_beta'])[ch] == 0)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_gn_non_finite_input_stays_in_its_sample_and_group(bad, relu):
    """A NaN / +Inf at row 3, channel 9 of sample 1 (group 2 = channels 8 .. 11; gamma < 0 in channels 8 and 11). Every other
    (sample, group) equals the clean run bit for bit, and so do d_gamma / d_beta of the other channels. In the unit itself,
    as for BatchNorm: mean non-finite, invstd = 1 / sqrt(eps) through the clamp of the variance at 0, dx non-finite at every
    element, d_gamma of the four channels non-finite; without ReLU y non-finite everywhere and d_beta the clean run's; with
    ReLU y = 0 where the pre-activation is NaN or -Inf (a NaN input: everywhere; an Inf input: the channels with gamma > 0)
    and +Inf where it is +Inf (an Inf input, gamma < 0)."""
    B, C, G, H, W = N.GN_COND
    case = N.make_gn_case(B, C, G, H, W, seed=33, relu=relu)
    assert [bool(g < 0) for g in case['gamma'][8:12]] == [True, False, False, True]
    clean = run_gn_act(case)
    x = case['x'].copy()
    x[1, 3, 9] = bad
    out = run_gn_act(case, x=x)
    hit = np.zeros((B, 1, C), bool)
    hit[1, 0, 8:12] = True
    hit = np.broadcast_to(hit, (B, H * W, C))
    for k in ('y', 'dx'):
        assert np.array_equal(host(out[k])[~hit], host(clean[k])[~hit]), k
    assert not np.isfinite(host(out['dx'])[hit]).any()
    ch = np.zeros(C, bool)
    ch[8:12] = True
    for k in ('d_gamma', 'd_beta'):
        assert np.array_equal(host(out[k])[~ch], host(clean[k])[~ch]), k
    assert not np.isfinite(host(out['d_gamma'])[ch]).any() and np.isfinite(host(out['d_beta'])[ch]).all()
    unit = np.zeros((B, G), bool)
    unit[1, 2] = True
    for k in ('mean', 'invstd'):
        assert np.array_equal(host(out[k])[~unit], host(clean[k])[~unit]), k
    assert not np.isfinite(float(out['mean'][1, 2])) and float(out['invstd'][1, 2]) == _top(case['eps'])
    y = host(out['y'])[1, :, 8:12]
    if not relu:
        assert not np.isfinite(y).any() and np.array_equal(host(out['d_beta']), host(clean['d_beta']))
        return
    plus_inf = np.isinf(bad) & (case['gamma'][8:12] < 0)                     # per channel
    assert np.array_equal(y, np.broadcast_to(np.where(plus_inf, np.float32(np.inf), np.float32(0)), y.shape))


@pytest.mark.parametrize('shape', [(1, 4), (513, 8), (3, 1024)])
def test_channel_sums_vs_float64(shape):
    x = N.make_bn_case(*shape, seed=41, relu=False)['x']
    s, e = N.column_sums(x)
    within(F.channel_sums(dev(x)), s, e, f'channel_sums {shape}')
    # a view 4 bytes into an allocation is not 16 B aligned: the framework's reduction, bounded by any order of summation
    buf = torch.empty(x.size + 1, device=DEV)
    view = buf[1:].view(*shape)
    view.copy_(dev(x))
    assert view.data_ptr() % 16 != 0
    any_order = N.SAFETY * N.U * (shape[0] * np.abs(x.astype(np.float64)).sum(0) + np.abs(s))
    within(F.channel_sums(view), s, any_order, f'channel_sums {shape}, misaligned')


# --------------------------------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize('r', N.COND_BOUNDED)
def test_conditioning_within_the_derived_bounds(r):
    """|mean| / std = r in one channel / one (sample, group), with ReLU: the bounds grow with r^2 and must still hold, the
    mask bits, dx and d_residual at every element included."""
    case, f, b = bn_case(*N.BN_COND, True, True, r=r)
    check_bn(run_bn_act(case), case, f, b, what=f'bn r={r}')
    case, f, b = gn_case(N.GN_COND, True, r=r)
    check_gn(run_gn_act(case), case, f, b, what=f'gn r={r}')


def _var_of(invstd, eps):
    return 1.0 / np.asarray(invstd, np.float64) ** 2 - float(np.float32(eps))


@pytest.mark.parametrize('r', N.COND_RECORDED)
def test_conditioning_beyond_the_domain_is_finite_and_contained(r):
    """r = 1e3, 1e5: the worst-case bound on the variance is vacuous (recorded, not asserted: EXPERIMENTS.md). Everything is
    finite, 0 < invstd <= 1 / sqrt(eps), and the units next to the ill-conditioned one keep their bounds."""
    # BatchNorm: channel 1
    case, f, b = bn_case(*N.BN_COND, False, False, r=r)
    out = run_bn_act(case)
    for k in ('y', 'dx', 'mean', 'invstd', 'running_mean', 'running_var', 'd_gamma', 'd_beta'):
        assert bool(torch.isfinite(out[k]).all()), k
    top = np.float32(1.0 / np.sqrt(np.float64(np.float32(case['eps']))))
    assert bool((out['invstd'] > 0).all()) and bool((out['invstd'] <= float(top)).all())
    other = np.arange(case['C']) != 1
    for k in ('mean', 'invstd', 'running_mean', 'running_var'):
        within(host(out[k])[other], f[k][other], f['bounds'][k][other], f'bn r={r} neighbours: {k}')
    within(host(out['y'])[:, other], f['y'][:, other], f['bounds']['y'][:, other], f'bn r={r} neighbours: y')
    within(host(out['dx'])[:, other], b['dx'][:, other], b['bounds']['dx'][:, other], f'bn r={r} neighbours: dx')
    for k in ('d_gamma', 'd_beta'):
        within(host(out[k])[other], b[k][other], b['bounds'][k][other], f'bn r={r} neighbours: {k}')
    x = dev(case['x'])
    ty, _, tinv = torch.native_batch_norm(x, dev(case['gamma']), dev(case['beta']), None, None, True, 0.0, case['eps'])
    rel_var = lambda inv: abs(_var_of(float(inv[1]), case['eps']) - f['var'][1]) / f['var'][1]
    rel_y = lambda y: float(np.abs(host(y)[:, 1] - f['y'][:, 1]).max() / np.abs(f['y'][:, 1]).max())
    print(f'bn r={r:g}: relative error of variance {rel_var(out["invstd"]):.2e} (fp32 torch {rel_var(tinv):.2e}), '
          f'of y {rel_y(out["y"]):.2e} (fp32 torch {rel_y(ty):.2e})')
    # GroupNorm: (sample, group) number 1 = sample 0, group 1 = channels 4 .. 7
    case, f, b = gn_case(N.GN_COND, False, r=r)
    out = run_gn_act(case)
    for k in ('y', 'dx', 'mean', 'invstd', 'd_gamma', 'd_beta'):
        assert bool(torch.isfinite(out[k]).all()), k
    top = np.float32(1.0 / np.sqrt(np.float64(np.float32(case['eps']))))
    assert bool((out['invstd'] > 0).all()) and bool((out['invstd'] <= float(top)).all())
    B, C, G, H, W = N.GN_COND
    unit = np.ones((B, G), bool)
    unit[0, 1] = False
    el = np.ones((B, H * W, C), bool)
    el[0, :, 4:8] = False
    ch = np.ones(C, bool)
    ch[4:8] = False
    for k in ('mean', 'invstd'):
        within(host(out[k])[unit], f[k][unit], f['bounds'][k][unit], f'gn r={r} neighbours: {k}')
    within(host(out['y'])[el], f['y'][el], f['bounds']['y'][el], f'gn r={r} neighbours: y')
    within(host(out['dx'])[el], b['dx'][el], b['bounds']['dx'][el], f'gn r={r} neighbours: dx')
    for k in ('d_gamma', 'd_beta'):
        within(host(out[k])[ch], b[k][ch], b['bounds'][k][ch], f'gn r={r} neighbours: {k}')
    x4 = shaped(case['x'], case['shape']).contiguous()
    ty, _, tinv = torch.native_group_norm(x4, dev(case['gamma']), dev(case['beta']), B, C, H * W, G, case['eps'])
    ty = ty.permute(0, 2, 3, 1).reshape(B, H * W, C)
    rel_var = lambda inv: abs(_var_of(float(inv.reshape(-1)[1]), case['eps']) - f['var'][0, 1]) / f['var'][0, 1]
    rel_y = lambda y: float(np.abs(host(y)[0, :, 4:8] - f['y'][0, :, 4:8]).max() / np.abs(f['y'][0, :, 4:8]).max())
    print(f'gn r={r:g}: relative error of variance {rel_var(out["invstd"]):.2e} (fp32 torch {rel_var(tinv):.2e}), '
          f'of y {rel_y(out["y"]):.2e} (fp32 torch {rel_y(ty):.2e})')
