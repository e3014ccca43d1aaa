"""The group max pool (gga_group_max_fwd / _bwd behind pointnet2.group_max_pool), the set abstraction / feature propagation
modules and the PointNet2SASSG backbone on the device: the pool bit for bit against the numpy scan of
tests/_pointnet_modules_ref.py, the modules bit for bit between the pool kernel and the framework's pool, the backbone against
the float64 restatement within the project's 1e-4 (tests/test_model_gpu.py): max|got - ref| <= 1e-4 * max(1, max|ref|)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _pointnet_modules_ref as R
from gga_amd import _lib
from gga_amd import pointnet2 as P
from gga_amd.pointnet_modules import PointSAModule, PointSAModuleMSG
from gga_amd.registry import build_backbone

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAYOUTS = {'nchw': torch.contiguous_format, 'channels_last': torch.channels_last}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same_bits(got, want, what=''):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else want
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        diff = got.view(np.uint8 if got.itemsize == 1 else np.uint32) != want.view(np.uint8 if want.itemsize == 1 else np.uint32)
        raise AssertionError(f'{what}: {int(diff.sum())} of {got.size} elements differ, first at {np.argwhere(diff)[0].tolist()}')


def _pool_fwd(x):
    """The forward entry point on x as it lies in memory -> (y, arg)."""
    B, C, M, K = x.shape
    y = torch.full((B, C, M), float('nan'), device=x.device)
    arg = torch.full((B, C, M), 255, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().gga_group_max_fwd(_ptr(x), B, C, M, K, *x.stride(), _ptr(y), _ptr(arg), _stream()), 'gga_group_max_fwd')
    return y, arg


def _pool_bwd(gy, arg, like):
    """The backward entry point into a NaN-filled tensor of `like`'s memory layout: what it leaves NaN it did not write."""
    B, C, M, K = like.shape
    gx = torch.full_like(like, float('nan'))
    assert gx.stride() == like.stride()
    _lib.check(_lib.lib().gga_group_max_bwd(_ptr(gy), _ptr(arg), B, C, M, K, *gx.stride(), _ptr(gx), _stream()), 'gga_group_max_bwd')
    return gx


def _inputs(shape, rng):
    """name -> float32 [B, C, M, K]: the value patterns a pool has to get right."""
    K, groups = shape[3], shape[:3]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rand = lambda: rng.normal(0, 1, shape).astype(np.float32)      # noqa: E731
    out = {'random': rand(), 'small integers': rng.integers(-2, 3, shape).astype(np.float32),
           'all equal': np.full(shape, 0.37, np.float32), 'signed zeros': rng.choice(np.array([0.0, -0.0], np.float32), shape)}
    x = rand()
    x[rng.random(groups) < 0.3] = -inf
    x.reshape(-1, K)[0] = -inf
    out['-inf groups'] = x
    x = rng.integers(-2, 3, shape).astype(np.float32)
    np.put_along_axis(x, rng.integers(0, K, groups + (1,)), nan, axis=3)         # one NaN in every group
    x.reshape(-1, K)[::2] = rand().reshape(-1, K)[::2]                           # ... of every other group
    out['one NaN'] = x
    x = rand()
    x[rng.random(shape) < 0.3] = nan
    out['several NaNs'] = x
    return out


def _to(x, layout):
    return torch.from_numpy(x).to(DEV).contiguous(memory_format=LAYOUTS[layout])


# ----------------------------------------------------------------------------- the pool, forward
@pytest.mark.parametrize('K', [1, 2, 16, 33, 64, 256])
@pytest.mark.parametrize('C', [1, 3, 4, 130])
def test_pool_forward_matches_the_scan_bit_for_bit(C, K):
    rng = np.random.default_rng(1000 * C + K)
    for B in (1, 2):
        for M in (1, 63, 65):
            for name, x in _inputs((B, C, M, K), rng).items():
                want_y, want_arg = R.group_max(x)
                for layout in LAYOUTS:
                    what = f'{name} [{B},{C},{M},{K}] {layout}'
                    xd = _to(x, layout)
                    y, arg = _pool_fwd(xd)
                    _same_bits(y, want_y, what + ' y')
                    _same_bits(arg, want_arg, what + ' arg')
                    out = P.group_max_pool(xd)
                    assert out.is_contiguous()
                    _same_bits(out, want_y, what + ' group_max_pool')


def test_pool_rule_on_written_out_groups():
    nan, inf = np.nan, np.inf
    x = np.array([[1, 3, 3, 2], [0.0, -0.0, 0, -1], [-0.0, 0.0, -1, -1], [-inf, -inf, -inf, -inf], [1, nan, 5, nan],
                  [nan, 7, 7, 7], [2, 2, 2, 2]], np.float32).reshape(1, 1, 7, 4)
    for layout in LAYOUTS:
        y, arg = _pool_fwd(_to(x, layout))
        assert arg.cpu().numpy().reshape(-1).tolist() == [1, 0, 0, 0, 1, 0, 0]
        _same_bits(y.reshape(-1), np.array([3, 0, -0.0, -inf, nan, nan, 2], np.float32), layout)


def test_pool_takes_the_eager_path_where_the_kernel_does_not_apply(monkeypatch):
    def refuse(*a):
        raise AssertionError('the pool kernel was called')
    eager = lambda t: torch.nn.functional.max_pool2d(t, [1, t.shape[3]]).squeeze(-1).contiguous()      # noqa: E731
    wide = torch.randn(2, 3, 5, _lib.GROUP_MAX_SAMPLES + 1, device=DEV)
    base = torch.randn(2, 5, 3, 16, device=DEV)
    view = base.permute(0, 2, 1, 3)
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last)
    fine = torch.randn(2, 3, 5, 16, device=DEV)
    with monkeypatch.context() as mp:
        mp.setattr(P._GroupMaxPool, 'apply', refuse)
        for t in (wide, view, fine.double(), fine.cpu()):
            got = P.group_max_pool(t)
            assert got.is_contiguous() and torch.equal(got, eager(t))
        with pytest.raises(AssertionError, match='the pool kernel was called'):
            P.group_max_pool(fine)
        mp.setattr(P, 'SA_POOL', False)                   # GGA_SA_POOL=0
        assert torch.equal(P.group_max_pool(fine), eager(fine))
    # the entry point itself refuses the wide tensor
    rc = _lib.lib().gga_group_max_fwd(_ptr(wide), 2, 3, 5, 257, *wide.stride(), _ptr(wide), _ptr(wide), _stream())
    assert rc == -1 and _lib.lib().gga_last_error().decode().startswith('gga_group_max_fwd: K 257')


# ----------------------------------------------------------------------------- the pool, backward
@pytest.mark.parametrize('K', [1, 2, 16, 33, 64, 256])
@pytest.mark.parametrize('C', [1, 3, 4, 130])
def test_pool_backward_writes_every_element_once(C, K):
    rng = np.random.default_rng(2000 * C + K)
    for B in (1, 2):
        for M in (1, 63, 65):
            shape = (B, C, M, K)
            gy = rng.normal(0, 1, shape[:3]).astype(np.float32)
            for x in (rng.integers(-2, 3, shape).astype(np.float32), rng.normal(0, 1, shape).astype(np.float32)):
                _, arg = R.group_max(x)
                want = R.group_max_grad(gy, arg, K)
                for layout in LAYOUTS:
                    xd = _to(x, layout)
                    got = _pool_bwd(torch.from_numpy(gy).to(DEV), torch.from_numpy(arg).to(DEV), xd)
                    _same_bits(got, want, f'[{B},{C},{M},{K}] {layout} gx')          # no NaN left: every element was written
                    # through autograd: the same bits, in the memory layout of x
                    xd.requires_grad_(True)
                    P.group_max_pool(xd).backward(torch.from_numpy(gy).to(DEV))
                    assert xd.grad.stride() == xd.stride()
                    _same_bits(xd.grad, want, f'[{B},{C},{M},{K}] {layout} autograd')


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('shape', [(2, 130, 65, 33), (1, 4, 63, 256), (2, 3, 1, 16), (2, 64, 130, 64)])
def test_pool_gradient_equals_max_pool2d_without_ties(shape, layout):
    rng = np.random.default_rng(7)
    x = rng.permutation(int(np.prod(shape))).astype(np.float32).reshape(shape)      # all values distinct
    g = torch.from_numpy(rng.normal(0, 1, shape[:3]).astype(np.float32)).to(DEV)
    a, b = _to(x, layout).requires_grad_(True), _to(x, layout).requires_grad_(True)
    ya = P.group_max_pool(a)
    yb = torch.nn.functional.max_pool2d(b, [1, shape[3]]).squeeze(-1)
    _same_bits(ya, yb.contiguous(), 'forward')
    ya.backward(g)
    yb.backward(g)
    _same_bits(a.grad, b.grad, 'gradient')


@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_pool_offsets_past_2_to_31(layout):
    # 64-bit index arithmetic: the second batch entry lies 2^31 + 64 elements behind the first. Only the two small regions the
    # strides reach are touched; the storage between them is never read or written.
    C, M, K = 5, 70, 33
    sb = 2 ** 31 + 64
    inner = (M * K, K, 1) if layout == 'nchw' else (1, K * C, C)
    store = torch.empty(sb + C * M * K, device=DEV)
    x = store.as_strided((2, C, M, K), (sb,) + inner)
    assert int(sum((n - 1) * s for n, s in zip(x.shape, x.stride()))) == store.numel() - 1       # the last element of the storage
    rng = np.random.default_rng(31)
    data = rng.integers(-3, 4, (2, C, M, K)).astype(np.float32)
    x.copy_(torch.from_numpy(data).to(DEV))
    want_y, want_arg = R.group_max(data)
    y, arg = _pool_fwd(x)
    _same_bits(y, want_y, 'y')
    _same_bits(arg, want_arg, 'arg')
    gy = rng.normal(0, 1, (2, C, M)).astype(np.float32)
    x.fill_(float('nan'))
    gyd = torch.from_numpy(gy).to(DEV)
    _lib.check(_lib.lib().gga_group_max_bwd(_ptr(gyd), _ptr(arg), 2, C, M, K, *x.stride(), _ptr(x), _stream()), 'gga_group_max_bwd')
    _same_bits(x.contiguous(), R.group_max_grad(gy, want_arg, K), 'gx')
    del x, store
    torch.cuda.empty_cache()                               # hand the 8 GiB back rather than keep them cached for the session


# ----------------------------------------------------------------------------- a set abstraction module
def _cloud(seed=0, feature_channels=1):
    rng = np.random.default_rng(seed)
    xyz = torch.from_numpy(rng.uniform(0, 1, (2, 100, 3)).astype(np.float32)).to(DEV)
    feats = torch.from_numpy(rng.normal(0, 1, (2, feature_channels, 100)).astype(np.float32)).to(DEV)
    return xyz, feats


def _sa_variant(variant):
    """-> (module, forward keyword arguments)"""
    torch.manual_seed(3)
    xyz, _ = _cloud()
    kw = {}
    if variant == 'msg':
        return PointSAModuleMSG(num_point=32, radii=[0.2, 0.4], sample_nums=[4, 8], mlp_channels=[[1, 8, 16], [1, 8, 8, 16]],
                                dilated_group=True, normalize_xyz=True), kw
    if variant == 'all points':
        return PointSAModule(mlp_channels=[1, 8, 8, 16], num_point=None, normalize_xyz=True), kw
    if variant == 'indices':
        kw['indices'] = torch.from_numpy(np.random.default_rng(5).integers(0, 100, (2, 32))).to(DEV).int()
    if variant == 'target_xyz':
        kw['target_xyz'] = xyz[:, 10:42] + 0.01
    return PointSAModule(mlp_channels=[1, 8, 8, 16], num_point=32, radius=0.4, num_sample=8, normalize_xyz=True), kw


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('variant', ['plain', 'indices', 'target_xyz', 'all points', 'msg'])
def test_sa_module_is_the_same_with_either_pool(variant, training, monkeypatch):
    module, kw = _sa_variant(variant)
    xyz, feats = _cloud()
    with torch.no_grad():                                   # running statistics that are not the initial (0, 1)
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    runs = []
    for own in (True, False):
        monkeypatch.setattr(P, 'SA_POOL', own)
        calls = []
        real = P._GroupMaxPool.apply
        monkeypatch.setattr(P._GroupMaxPool, 'apply', lambda x: (calls.append(tuple(x.shape)), real(x))[1])
        mod = copy.deepcopy(module).to(DEV).train(training)
        new_xyz, new_features, indices = mod(xyz, feats, **kw)
        monkeypatch.setattr(P._GroupMaxPool, 'apply', real)
        assert (len(calls) == len(mod.mlps)) if own else not calls
        runs.append((new_xyz, new_features, indices, {k: v.clone() for k, v in mod.state_dict().items()}))
    (xa, fa, ia, sa), (xb, fb, ib, sb) = runs
    M = 1 if variant == 'all points' else 32
    assert fa.shape == (2, 32 if variant == 'msg' else 16, M) and fa.is_contiguous()
    _same_bits(fa, fb, 'new_features')
    for k in sa:
        _same_bits(sa[k], sb[k], k)
    if training:
        assert int(sa['mlps.0.layer0.bn.num_batches_tracked']) == 1
    if variant == 'all points':
        assert xa is None and xb is None and ia is None and ib is None
        return
    _same_bits(xa, xb, 'new_xyz')
    if variant == 'target_xyz':
        assert ia is None and ib is None
        _same_bits(xa, kw['target_xyz'], 'new_xyz is target_xyz')
        return
    _same_bits(ia, ib, 'indices')
    assert ia.shape == (2, 32)
    _same_bits(xa, torch.gather(xyz, 1, ia.long().unsqueeze(-1).expand(-1, -1, 3)), 'new_xyz is points_xyz at indices')
    if variant == 'indices':
        _same_bits(ia, kw['indices'], 'indices as given')


# ----------------------------------------------------------------------------- the backbone
def _device_run(own, monkeypatch):
    """One training-mode forward and backward of the small backbone on the device -> (model, outputs, gradients by name)."""
    monkeypatch.setattr(P, 'SA_POOL', own)
    model, points = R.small_case()
    model = model.to(DEV)
    pts = points.to(DEV).requires_grad_(True)
    out = model(pts)
    last = out['fp_features'][-1]
    (last * R.functional_weights(last.shape).float().to(DEV)).sum().backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    grads['points.features'] = pts.grad[..., 3:]
    return model, out, grads


def _device_indices(out, cfg=R.SMALL):
    """The sampling, ball-query and three-NN indices of the device run, recomputed by the same (deterministic) operators from
    the coordinates the run returned."""
    sa_xyz = out['sa_xyz']
    fps = [P.furthest_point_sample(sa_xyz[i], M).long().cpu() for i, M in enumerate(cfg['num_points'])]
    ball = [P.ball_query(0, r, K, sa_xyz[i], sa_xyz[i + 1]).long().cpu()
            for i, (r, K) in enumerate(zip(cfg['radius'], cfg['num_samples']))]
    n = len(cfg['num_points'])
    nn = [P.three_nn(sa_xyz[n - i - 1], sa_xyz[n - i])[1].long().cpu() for i in range(len(cfg['fp_channels']))]
    return dict(fps=fps, ball=ball, nn=nn)


def _distances(out, grads, out64, grads64):
    """name -> (max|got - ref|, max|ref|) over every element of every compared tensor."""
    pairs = {}
    for key in ('fp_features', 'sa_features'):
        for i, (a, b) in enumerate(zip(out[key], out64[key])):
            pairs[f'{key}[{i}]'] = (a, b)
    assert set(grads) == set(grads64)
    for k in grads64:
        pairs['grad ' + k] = (grads[k], grads64[k])
    res = {}
    for k, (a, b) in pairs.items():
        a, b = a.detach().double().cpu(), b.detach().double()
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), k
        res[k] = (float((a - b).abs().max()), float(b.abs().max()))
    return res


def test_backbone_against_float64(monkeypatch):
    """Forward, backward and the same with GGA_SA_POOL=0 against the float64 restatement; prints max|got - float64| per tensor
    for both runs (copied into EXPERIMENTS.md 6aa: the worst tensor sits at 0.29 of its bound). The pooled run may be at most
    twice as far from float64 as the eager one: the grouping backward's float atomics differ between two runs of one path."""
    model, out, grads = _device_run(True, monkeypatch)
    _, out_e, grads_e = _device_run(False, monkeypatch)
    index = _device_indices(out)
    want = R.indices_numpy(out['sa_xyz'][0].detach().cpu().numpy())
    for k in index:
        for a, b in zip(index[k], want[k]):
            assert torch.equal(a, b), k
    for i, fps in enumerate(index['fps']):                       # the run used these very samples
        _same_bits(out['sa_xyz'][i + 1], torch.gather(out['sa_xyz'][i], 1, fps.to(DEV).unsqueeze(-1).expand(-1, -1, 3)), 'fps')
    out64, grads64 = R.run(model.cpu(), R.small_case()[1], index, torch.float64)
    own, eager = _distances(out, grads, out64, grads64), _distances(out_e, grads_e, out64, grads64)
    assert len(own) == 3 + 5 + 48 + 1
    failures = []
    for k, (d, scale) in own.items():
        bound = 1e-4 * max(1.0, scale)
        print(f'{k:58s} pool kernel {d:.3e}  max_pool2d {eager[k][0]:.3e}  max|ref| {scale:.3e}  bound {bound:.3e}')
        if not d <= bound:
            failures.append((k, 'bound', d, bound))
        if not d <= 2 * eager[k][0]:
            failures.append((k, 'twice the eager distance', d, eager[k][0]))
    assert not failures, failures


def test_backbone_structure(monkeypatch):
    model, out, _ = _device_run(True, monkeypatch)
    cfg = R.SMALL
    pts = R.small_case()[1].to(DEV)
    assert [tuple(t.shape) for t in out['sa_xyz']] == [(2, 100, 3)] + [(2, M, 3) for M in cfg['num_points']]
    assert [tuple(t.shape) for t in out['sa_features']] == [(2, 1, 100)] + [(2, c[-1], M) for c, M in zip(cfg['sa_channels'],
                                                                                                             cfg['num_points'])]
    assert [tuple(t.shape) for t in out['sa_indices']] == [(2, 100)] + [(2, M) for M in cfg['num_points']]
    assert [tuple(t.shape) for t in out['fp_xyz']] == [(2, 4, 3), (2, 8, 3), (2, 16, 3)]
    assert [tuple(t.shape) for t in out['fp_features']] == [(2, 32, 4), (2, 32, 8), (2, 32, 16)]
    assert [tuple(t.shape) for t in out['fp_indices']] == [(2, 4), (2, 8), (2, 16)]
    assert torch.equal(out['sa_indices'][0], torch.arange(100, device=DEV).expand(2, -1))
    for idx, xyz in zip(out['sa_indices'], out['sa_xyz']):
        assert idx.dtype == torch.int64
        _same_bits(xyz, torch.gather(pts[..., :3], 1, idx.unsqueeze(-1).expand(-1, -1, 3)), 'sa_xyz is the cloud at sa_indices')
    for i in range(3):                                     # the deepest level first, then one level up per propagation
        assert out['fp_xyz'][i] is out['sa_xyz'][4 - i] and out['fp_indices'][i] is out['sa_indices'][4 - i]
    assert out['fp_features'][0] is out['sa_features'][4]
    _same_bits(out['sa_features'][0], pts[..., 3:].transpose(1, 2).contiguous(), 'sa_features[0]')
    # the trained statistics travel through a state_dict into a fresh model
    torch.manual_seed(99)
    fresh = build_backbone(cfg).to(DEV)
    assert list(fresh.state_dict()) == list(model.state_dict())
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        a, b = model.eval()(pts), fresh.eval()(pts)
    for key in a:
        for s, t in zip(a[key], b[key]):
            _same_bits(s, t, key)
    assert float((a['fp_features'][-1] - out['fp_features'][-1].detach()).abs().max()) > 0       # evaluation mode is another function
