"""Backward of a head branch on the active tiles of its output gradient (gga_head_tile_activity, gga_head_branch_bwd):
the activity map against a torch reference, the new entry point bit for bit against the two dense entry points it
replaces, a float64 cross-check on a sparse gradient, and the whole head node with one dense and several sparse
branches. Run with ``-m gpu`` on an MI355X."""
import pytest
import torch

from gga_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TR, TW = 8, 32           # the tile of the weight gradient and of the tail kernels
PATTERNS = ('zero', 'corner', 'last', 'last_channel', 'dense', 'cells')


def _grad_y(pattern, B, cout, H, W, seed):
    """Output gradients of the patterns the kernels have to tell apart; returns (grad_y, (y, x) of 'corner')."""
    g = torch.Generator().manual_seed(seed)
    gy = torch.zeros(B, cout, H, W)
    corner = (TR, TW if W > TW else 0)            # first pixel of a tile: its ring reaches the tiles above / left of it
    if pattern == 'corner':
        gy[B - 1, 0, corner[0], corner[1]] = 1.5
    elif pattern == 'last':
        gy[0, cout - 1, H - 1, W - 1] = -2.0
    elif pattern == 'last_channel':
        gy[B - 1, cout - 1, H // 2, W // 2] = 0.75
    elif pattern == 'dense':
        gy = torch.randn(B, cout, H, W, generator=g)
    elif pattern == 'cells':                        # about 20 object cells per frame, every channel of the cell
        for b in range(B):
            ys, xs = torch.randint(0, H, (20,), generator=g), torch.randint(0, W, (20,), generator=g)
            gy[b, :, ys, xs] = torch.randn(cout, 20, generator=g)
    else:
        assert pattern == 'zero'
    return gy.to(DEV), corner


def _activity_ref(gy):
    B, _, H, W = gy.shape
    nz = (gy != 0).float().amax(dim=1, keepdim=True)
    ring = torch.nn.functional.max_pool2d(nz, 3, stride=1, padding=1)
    ty, tx = -(-H // TR), -(-W // TW)
    ring = torch.nn.functional.pad(ring, (0, tx * TW - W, 0, ty * TR - H))
    return ring.view(B, ty, TR, tx, TW).amax(dim=(2, 4)) > 0           # [B, tiles_y, tiles_x]


def _activity(gy):
    from gga_amd import _lib
    B, cout, H, W = gy.shape
    ty, tx = -(-H // TR), -(-W // TW)
    act = torch.full((B, ty, tx), 0x5a, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().gga_head_tile_activity(F._p(gy), B, H, W, cout, F._p(act), F._stream()), 'gga_head_tile_activity')
    assert bool((act <= 1).all())
    return act > 0


@pytest.mark.parametrize('shape', [(3, 37, 29), (2, 50, 216)])
def test_tile_activity_map_vs_torch(shape):
    B, H, W = shape
    for cout in (1, 4):
        for pattern in PATTERNS:
            gy, corner = _grad_y(pattern, B, cout, H, W, seed=H + cout)
            act, ref = _activity(gy), _activity_ref(gy)
            assert torch.equal(act, ref), (cout, pattern)
            n = int(act.sum())
            if pattern == 'zero':
                assert n == 0
            elif pattern == 'corner':
                assert n == (4 if corner[1] else 2)            # the tiles that meet at the corner
            elif pattern == 'last':
                assert n == 1 and bool(act[0, -1, -1])
            elif pattern == 'dense':
                assert n == act.numel()
    # the bits are compared, not the value: NaN and Inf make their tile active
    for bad in (float('nan'), float('inf')):
        gy = torch.zeros(B, 2, H, W, device=DEV)
        gy[1, 1, 3, 5] = bad
        act = _activity(gy)
        assert torch.equal(act, _activity_ref(gy)) and int(act.sum()) == 1 and bool(act[1, 0, 0])


_CASES = {}


def _branch_case(shape):
    """Inputs of a branch on a map, made once per shape: a 64-channel column block of a wider activation with its
    BatchNorm statistics (float64 arithmetic, stored as float32), gamma and the conv weights for every width."""
    if shape not in _CASES:
        B, H, W = shape
        g = torch.Generator().manual_seed(B * 1000 + W)
        wide, blk = 128, 1
        big = torch.randn(B, H, W, wide, generator=g).to(DEV)
        x = big[..., 64 * blk:64 * blk + 64]
        mean = x.double().mean(dim=(0, 1, 2))
        var = x.double().var(dim=(0, 1, 2), unbiased=False)
        gamma = (torch.rand(64, generator=g) + 0.5).to(DEV)
        beta = (torch.rand(64, generator=g) - 0.5).to(DEV)
        invstd = (var + 1e-3).rsqrt()
        scale = gamma.double() * invstd
        saved = torch.cat([mean, invstd]).float()
        ss = torch.cat([scale, beta.double() - mean * scale]).float()
        ws = {c: (torch.randn(c, 64, 3, 3, generator=g) * 0.05).to(DEV) for c in (1, 2, 3, 4)}
        _CASES[shape] = dict(big=big, wide=wide, blk=blk, gamma=gamma, beta=beta, saved=saved, ss=ss, w=ws)
    return _CASES[shape]


def _run_branch(case, shape, cout, gy, sparse, hint=1):
    """(grad_weight, grad_bias, G, grad_gamma, grad_beta, absmax word) of one branch: through gga_head_branch_bwd (hint: its
    sparse_grad_y argument), or through gga_head_conv3x3_wgrad + gga_head_tail_bwd (the dense walk)."""
    from gga_amd import _lib
    L = _lib.lib()
    B, H, W = shape
    xp = case['big'].data_ptr() + 4 * 64 * case['blk']
    w = case['w'][cout]
    nan = float('nan')
    dw, db = torch.full_like(w, nan), torch.full((cout,), nan, device=DEV)
    G = torch.full((B, H, W, 64), nan, device=DEV)
    gg, gb = torch.full((64,), nan, device=DEV), torch.full((64,), nan, device=DEV)
    amax = torch.zeros(1, dtype=torch.int32, device=DEV)
    if sparse:
        ws = torch.empty(L.gga_head_branch_bwd_workspace_bytes(B, H, W, cout), dtype=torch.uint8, device=DEV)
        _lib.check(L.gga_head_branch_bwd(F._p(gy), xp, case['wide'], F._p(case['ss']), F._p(case['gamma']), F._p(case['saved']),
                                         F._p(w), B, H, W, 64, cout, F._p(dw), F._p(db), F._p(G), 64, F._p(gg), F._p(gb),
                                         F._p(amax), hint, F._p(ws), ws.numel(), F._stream()), 'gga_head_branch_bwd')
    else:
        ws = torch.empty(L.gga_head_conv3x3_workspace_bytes(cout), dtype=torch.uint8, device=DEV)
        _lib.check(L.gga_head_conv3x3_wgrad(xp, case['wide'], F._p(case['ss']), F._p(gy), B, H, W, 64, cout, F._p(dw), F._p(db),
                                            F._p(ws), ws.numel(), F._stream()), 'gga_head_conv3x3_wgrad')
        wsb = torch.empty(L.gga_bn_relu_workspace_bytes(B * H * W, 64), dtype=torch.uint8, device=DEV)
        _lib.check(L.gga_head_tail_bwd(F._p(gy), xp, case['wide'], F._p(case['ss']), F._p(case['gamma']), F._p(case['saved']),
                                       F._p(w), B, H, W, 64, cout, F._p(G), 64, F._p(gg), F._p(gb), F._p(amax), F._p(wsb),
                                       wsb.numel(), F._stream()), 'gga_head_tail_bwd')
    return dw, db, G, gg, gb, amax


# (6, 200, 176): 900 tiles, more than one per workgroup of the weight gradient; (4, 200, 704): 2200 tiles, above the tail
# kernels' 2048 workgroups, so those walk more than one tile too
@pytest.mark.parametrize('cout', [1, 2, 3, 4])
@pytest.mark.parametrize('shape', [(3, 37, 29), (6, 200, 176), (4, 200, 704)])
def test_branch_backward_on_active_tiles_equals_dense_walk(shape, cout):
    case = _branch_case(shape)
    B, H, W = shape
    names = ('grad_weight', 'grad_bias', 'G', 'grad_gamma', 'grad_beta', 'absmax')
    for pattern in PATTERNS:
        gy, _ = _grad_y(pattern, B, cout, H, W, seed=W + cout)
        new = _run_branch(case, shape, cout, gy, sparse=True)
        old = _run_branch(case, shape, cout, gy, sparse=False)
        for name, a, b in zip(names, new, old):
            assert not bool(torch.isnan(b).any()), (pattern, name)
            assert torch.equal(a, b), (pattern, name)
        if pattern in ('dense', 'cells'):              # the hint for a dense gradient chooses the walk, not the result
            for name, a, b in zip(names, _run_branch(case, shape, cout, gy, sparse=True, hint=0), old):
                assert torch.equal(a, b), (pattern, name, 'hint 0')


@pytest.mark.parametrize('cout', [1, 3])
def test_branch_backward_on_a_sparse_gradient_vs_float64(cout):
    """Both walks could share a mistake: conv(relu(bn(x))) backward in eager float64 for five non-zero cells.
    Tolerances: test_head_output_conv_on_column_blocks_of_large_maps (dw, db), test_bn_relu_head_conv_fused_vs_torch
    (input gradient, BatchNorm gradients)."""
    shape = (3, 37, 29)
    B, H, W = shape
    case = _branch_case(shape)
    g = torch.Generator().manual_seed(40 + cout)
    gy = torch.zeros(B, cout, H, W)
    for b, y, x in ((0, 0, 0), (0, 7, 28), (1, 8, 13), (2, 36, 28), (2, 20, 1)):
        gy[b, :, y, x] = torch.randn(cout, generator=g)
    gy = gy.to(DEV)
    dw, db, G, gg, gb, _ = _run_branch(case, shape, cout, gy, sparse=True)
    x64 = case['big'][..., 64:128].permute(0, 3, 1, 2).double().requires_grad_(True)
    gam, bet = case['gamma'].double().requires_grad_(True), case['beta'].double().requires_grad_(True)
    w64 = case['w'][cout].double().requires_grad_(True)
    b64 = torch.zeros(cout, dtype=torch.float64, device=DEV, requires_grad=True)
    h = torch.relu(torch.nn.functional.batch_norm(x64, None, None, gam, bet, training=True, eps=1e-3))
    torch.nn.functional.conv2d(h, w64, b64, padding=1).backward(gy.double())
    assert float((dw.double() - w64.grad).abs().max() / w64.grad.abs().max()) < 2e-6
    assert float((db.double() - b64.grad).abs().max() / b64.grad.abs().max()) < 2e-5
    gx_ref = x64.grad.permute(0, 2, 3, 1)
    assert float(gx_ref.abs().max()) > 1e-2
    assert int(((G.double() - gx_ref).abs() > 1e-4).sum()) <= 3       # ReLU-boundary elements may flip
    torch.testing.assert_close(gg, gam.grad.float(), rtol=1e-3, atol=2e-3)
    torch.testing.assert_close(gb, bet.grad.float(), rtol=1e-3, atol=2e-3)


def test_head_node_with_one_dense_and_several_sparse_branches():
    """functional._HeadBranches with the gradients a CenterHead produces - dense on a heat-map branch, a handful of
    cells on the regression branches - against the branches run one by one and against eager torch, at the tolerances
    of test_head_branches_one_node_vs_branch_by_branch."""
    from gga_amd import dense_conv
    B, H, W, couts = 2, 37, 45, (2, 1, 3, 2, 1)

    def make():
        torch.manual_seed(22)
        out = []
        for c in couts:
            conv1 = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).to(DEV).to(memory_format=torch.channels_last)
            bn = torch.nn.BatchNorm2d(64, eps=1e-3, momentum=0.01).to(DEV)
            bn.weight.data.uniform_(0.5, 1.5), bn.bias.data.uniform_(-0.5, 0.5)
            out.append((conv1, bn, torch.nn.Conv2d(64, c, 3, padding=1, bias=True).to(DEV)))
        return out
    torch.manual_seed(23)
    x = torch.randn(B, 64, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
    gs = []
    for i, c in enumerate(couts):
        if i == 1:
            gs.append(torch.randn(B, c, H, W, device=DEV))
        else:
            g = torch.zeros(B, c, H, W, device=DEV)
            for b in range(B):
                ys, xs = torch.randint(0, H, (4,)), torch.randint(0, W, (4,))
                g[b, :, ys, xs] = torch.randn(c, 4, device=DEV)
            gs.append(g)
    results = []
    for mode in ('node', 'single', 'eager'):
        br = make()
        xi = x.clone().requires_grad_(True)
        if mode == 'node':
            ys = F.head_branches(xi, br, sparse_grad=[i != 1 for i in range(len(couts))])
            assert ys is not None and 'HeadBranches' in type(ys[0].grad_fn).__name__
        elif mode == 'single':
            ys = [F.bn_relu_head_conv3x3(dense_conv.conv2d(xi, c1, bn_follows=True), bn, c2, sparse_grad=i != 1)
                  for i, (c1, bn, c2) in enumerate(br)]
        else:
            ys = [c2(torch.relu(bn(c1(xi)))) for c1, bn, c2 in br]
        sum((y * g).sum() for y, g in zip(ys, gs)).backward()
        results.append((xi.grad, br))
    (gx_n, br_n), (gx_s, br_s), (gx_e, br_e) = results
    for i in range(len(couts)):
        for j in (0, 2):
            torch.testing.assert_close(br_n[i][j].weight.grad, br_s[i][j].weight.grad, rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(br_n[i][j].weight.grad, br_e[i][j].weight.grad, rtol=2e-3, atol=2e-3)
        torch.testing.assert_close(br_n[i][2].bias.grad, br_e[i][2].bias.grad, rtol=1e-4, atol=1e-3)
        torch.testing.assert_close(br_n[i][1].weight.grad, br_e[i][1].weight.grad, rtol=1e-3, atol=2e-3)
        torch.testing.assert_close(br_n[i][1].bias.grad, br_e[i][1].bias.grad, rtol=1e-3, atol=2e-3)
    torch.testing.assert_close(gx_n, gx_s, rtol=1e-4, atol=1e-4)
    scale = float(gx_e.abs().max())
    assert int(((gx_n - gx_e).abs() > 1e-4 * scale).sum()) <= 10      # ReLU-boundary elements may flip
