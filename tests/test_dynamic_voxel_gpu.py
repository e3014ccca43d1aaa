"""Dynamic voxelization on the GPU (gga_amd/csrc/dynamic_voxel.hip) against the CPU restatement of
tests/_dynamic_voxel_ref.py and the reference's recorded results (tests/golden/dynamic_voxel.npz). Shapes are the smallest
at which each kernel can still go wrong: empty frames, every boundary of the fp32 cell formula, segments on both sides of
the wave width and of the split chunk, ties, dropped points, M = 0."""
import copy
import os

import numpy as np
import pytest
import torch

import _dynamic_voxel_ref as DR
from conftest import REPO
from gga_amd import Config, _lib, build_model, synthetic
from gga_amd import dynamic_voxel as DV
from gga_amd import functional as F
from gga_amd.ops import DynamicScatter
from gga_amd.registry import VOXEL_ENCODERS
from gga_amd.voxel_layer import Voxelization

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VS, RNG = [0.5, 0.5, 0.5], [0, -2, -1, 4, 2, 1]          # 8 x 8 x 4 cells
GRID = (8, 8, 4)
CHUNK = 256                                               # gga_dynamic_scatter_chunk(): asserted below


def _layer(vs=VS, rng=RNG):
    return Voxelization(voxel_size=vs, point_cloud_range=rng, max_num_points=-1, max_voxels=(-1, -1))


def _edge_frame(n, seed):
    """n points: the boundaries of every axis, non-finite coordinates, the rest random over a box larger than the range."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(RNG[:3]), torch.tensor(RNG[3:], dtype=torch.float32)
    p = torch.rand(n, 4, generator=g)
    p[:, :3] = (lo - 0.4) + p[:, :3] * (hi - lo + 0.8)
    mid = (lo + hi) / 2
    rows = []
    for a in range(3):
        for v in (lo[a], hi[a], torch.nextafter(hi[a], torch.tensor(-np.inf)), lo[a] - 1e-3,
                  torch.nextafter(lo[a], torch.tensor(-np.inf))):
            r = mid.clone()
            r[a] = v
            rows.append(r)
    rows.append(lo.clone())
    rows.append(hi.clone())
    special = torch.stack(rows)
    k = special.shape[0]
    if n < k + 3:
        return p, []
    p[:k, :3] = special
    for j, bad in enumerate((float('nan'), float('inf'), float('-inf'))):
        p[k + j, :3] = mid
        p[k + j, j] = bad
    return p, list(range(k, k + 3))


def test_coors_equal_the_fp32_formula_on_every_boundary():
    big, bad_rows = _edge_frame(257, 0)
    frames = [_edge_frame(1, 1)[0][:1].clone(), torch.zeros(0, 4), big]        # 1, 0 and 257 points: the empty frame in the middle
    frames[0][0, :3] = torch.tensor([0.0, -2.0, -1.0])                         # the single point: exactly at lo
    layer = _layer()
    cat, coors = layer.forward_batch([f.to(DEV) for f in frames])
    want = DR.point_coors(frames, VS, RNG)
    assert cat.shape == (258, 4) and torch.equal(cat.cpu().view(torch.int32), torch.cat(frames).view(torch.int32))
    assert coors.dtype == torch.int32 and torch.equal(coors.cpu(), want)
    assert coors[0].tolist() == [0, 0, 0, 0]
    # the non-finite rule: NaN / +inf / -inf in any coordinate = out of range, as the hard voxelizer treats them
    for r in bad_rows:
        assert coors[1 + r].tolist() == [2, -1, -1, -1]
    dropped = int((want[:, 1] < 0).sum())
    assert 0 < dropped < 258
    vm = coors.voxel_map
    ref = DR.voxel_map(want)
    assert vm.host_counts() == (ref['counts'].numel(), 258 - dropped)
    # single sample: [N, 3] (z, y, x), as mmcv
    c3 = layer(big.to(DEV))
    assert c3.shape == (257, 3) and torch.equal(c3.cpu(), DR.point_coors([big], VS, RNG)[:, 1:])


def test_dynamic_agrees_with_the_hard_voxelizer_where_no_cap_binds():
    from gga_amd.voxel_encoders import DynamicSimpleVFE, HardSimpleVFE
    p = _edge_frame(300, 3)[0]
    hard = Voxelization(voxel_size=VS, point_cloud_range=RNG, max_num_points=64, max_voxels=(1000, 1000))
    voxels, hcoors, npts = hard(p.to(DEV))
    assert int(npts.max()) < 64
    cat, coors = _layer().forward_batch([p.to(DEV)])
    vm = coors.voxel_map
    m = vm.m
    key = (hcoors[:, 0].long() * 8 + hcoors[:, 1]) * 8 + hcoors[:, 2]
    perm = torch.argsort(key)
    assert torch.equal(hcoors[perm], vm.voxel_coors[:m, 1:])                   # hard coors, sorted, = dynamic voxel coors
    counts = (vm.voxel_start[1:m + 1] - vm.voxel_start[:m])
    assert torch.equal(npts[perm].int(), counts)
    hmean = HardSimpleVFE(4)(voxels, npts, hcoors)[perm].cpu().double()
    dmean, dcoors = DynamicSimpleVFE(VS, RNG)(cat, coors)
    assert torch.equal(dcoors, vm.voxel_coors[:m])
    ref = DR.voxel_map(DR.point_coors([p], VS, RNG))
    want, _ = DR.scatter(p, ref, 'avg')
    bound = _mean_bound(p, ref)
    assert ((dmean.cpu().double() - want).abs() <= bound).all() and ((hmean - want).abs() <= bound).all()


def _mean_bound(x, ref):
    """(n + 2) 2^-24 sum|x| / n per voxel and channel: the fp32 bound of a sequential sum of n terms plus the division."""
    keep = ref['point2voxel'] >= 0
    sabs = torch.zeros((ref['counts'].numel(), x.shape[1]), dtype=torch.float64).index_add(0, ref['point2voxel'][keep],
                                                                                             x.double().abs()[keep])
    n = ref['counts'].double()[:, None]
    return (n + 2) * 2.0 ** -24 * sabs / n


# ---- map ------------------------------------------------------------------------------------------------------------------
def _coors_case(name):
    """[N, 4] int32 point coordinates (b, z, y, x), in a shuffled point order."""
    g = torch.Generator().manual_seed(len(name))
    if name == 'segments':
        # 1, 63, 64, 65 points and one voxel of more than two chunks; the last cell of sample 0 next to the first of sample 1
        cells = [((0, 1, 2, 3), 1), ((0, 3, 7, 7), 63), ((1, 0, 0, 0), 64), ((1, 0, 0, 1), 65), ((1, 2, 5, 5), 2 * CHUNK + 5),
                 ((0, 0, 0, 0), CHUNK), ((1, 3, 7, 7), CHUNK + 1)]
        rows = torch.cat([torch.tensor([c], dtype=torch.int32).repeat(n, 1) for c, n in cells])
    elif name == 'one_voxel':
        rows = torch.tensor([[0, 2, 4, 6]], dtype=torch.int32).repeat(3 * CHUNK + 17, 1)
    elif name == 'all_out':
        rows = torch.tensor([[0, -1, -1, -1], [1, -1, -1, -1]], dtype=torch.int32).repeat(40, 1)
    elif name == 'dropped':
        rows = torch.stack([torch.randint(0, 2, (700,), generator=g), torch.randint(0, 4, (700,), generator=g),
                            torch.randint(0, 3, (700,), generator=g), torch.randint(0, 2, (700,), generator=g)], 1).int()
        rows[torch.randperm(700, generator=g)[:70], 1:] = -1
    else:
        raise KeyError(name)
    if name != 'all_out':       # all_out keeps sample 0 before sample 1 like a batch; the map does not rely on it
        rows = rows[torch.randperm(rows.shape[0], generator=g)]
    return rows.contiguous()


MAP_CASES = ('segments', 'one_voxel', 'all_out', 'dropped')


def _check_map(vm, ref, n):
    M = ref['counts'].numel()
    kept = int(ref['counts'].sum())
    assert vm.host_counts() == (M, kept)
    assert torch.equal(vm.point2voxel.cpu().long(), ref['point2voxel'])
    assert torch.equal(vm.voxel_start[:M + 1].cpu().long(), ref['voxel_start'])
    assert torch.equal(vm.order[:kept].cpu().long(), ref['order'])              # stable: ascending inside every segment
    want_vc = ref['voxel_coors'].int()
    assert torch.equal(vm.voxel_coors[:M].cpu(), want_vc if want_vc.shape[1] == 4 else torch.cat([want_vc[:, :1] * 0, want_vc], 1))
    assert int(vm.voxel_coors[M:].abs().sum()) == 0                             # rows past M stay zero
    assert sorted(vm.order.cpu().tolist()) == list(range(n))                    # a permutation: dropped points last


@pytest.mark.parametrize('case', MAP_CASES)
def test_map_is_exact(case):
    assert _lib.lib().gga_dynamic_scatter_chunk() == CHUNK
    coors = _coors_case(case)
    ref = DR.voxel_map(coors)
    vm = DV.map_of(coors.to(DEV), GRID, batch=2)
    _check_map(vm, ref, coors.shape[0])
    order = vm.order[:vm.host_counts()[1]].cpu()
    start = ref['voxel_start']
    for v in range(ref['counts'].numel()):
        seg = order[start[v]:start[v + 1]]
        assert (seg[1:] > seg[:-1]).all()
    if case == 'all_out':
        assert vm.m == 0
        out = DV.scatter(torch.ones(coors.shape[0], 4, device=DEV), vm, DV.MAX)     # nothing is written, no empty launch
        assert out.shape == (0, 4)
    # 3-column coordinates = one sample
    one = coors[coors[:, 0] == 0][:, 1:].contiguous()
    _check_map(DV.map_of(one.to(DEV), GRID), DR.voxel_map(one), one.shape[0])


def test_map_of_an_empty_input():
    vm = DV.map_of(torch.zeros((0, 4), dtype=torch.int32, device=DEV), GRID, batch=1)
    assert vm.host_counts() == (0, 0) and vm.voxel_coors.shape == (0, 4)
    assert DV.scatter(torch.zeros(0, 5, device=DEV), vm, DV.MEAN).shape == (0, 5)


def test_prepared_form_equals_the_list_form():
    frames = [_edge_frame(n, 10 + n)[0] for n in (40, 0, 130)]
    cap = np.array([0, 64, 64, 64 + 200], np.int64)             # frames at capacity offsets, device-side counts
    buf = torch.full((int(cap[-1]), 4), 0.25)                   # stale rows past a count lie INSIDE the range: they must drop
    for b, f in enumerate(frames):
        buf[cap[b]:cap[b] + f.shape[0]] = f
    prep = F.PreparedPoints(buf.to(DEV), cap, torch.tensor([f.shape[0] for f in frames], dtype=torch.int32, device=DEV))
    layer = _layer()
    pts_p, coors_p = layer.forward_prepared(prep)
    _, coors_l = layer.forward_batch([f.to(DEV) for f in frames])
    real = torch.cat([torch.arange(cap[b], cap[b] + f.shape[0]) for b, f in enumerate(frames)])
    assert pts_p.shape[0] == 264 and torch.equal(coors_p.cpu()[real], coors_l.cpu())
    rest = torch.ones(264, dtype=torch.bool)
    rest[real] = False
    assert (coors_p.cpu()[rest][:, 1:] == -1).all()
    mp, ml = coors_p.voxel_map, coors_l.voxel_map
    assert mp.host_counts() == ml.host_counts()
    assert torch.equal(mp.voxel_coors[:mp.m], ml.voxel_coors[:ml.m])
    assert torch.equal(mp.point2voxel.cpu()[real], ml.point2voxel.cpu()) and (mp.point2voxel.cpu()[rest] == -1).all()
    assert torch.equal(mp.voxel_start[:mp.m + 1], ml.voxel_start[:ml.m + 1])


# ---- DynamicScatter ---------------------------------------------------------------------------------------------------------
_SCATTER_REF = {}


def _scatter_case(case, C):
    """(coors, features, reference map, grad_out) of a case, made once."""
    if (case, C) not in _SCATTER_REF:
        coors = _coors_case(case)
        g = torch.Generator().manual_seed(100 + C)
        n = coors.shape[0]
        x = torch.randn(n, C, generator=g)
        x[:, ::2] = torch.round(x[:, ::2] * 2) / 2           # even channels: half-integers, so ties are real
        x[1::7] = x[0::7][:x[1::7].shape[0]]                  # and whole duplicated points
        ref = DR.voxel_map(coors)
        gout = torch.randn(ref['counts'].numel(), C, generator=g)
        _SCATTER_REF[(case, C)] = (coors, x, ref, gout)
    return _SCATTER_REF[(case, C)]


@pytest.mark.parametrize('C', [1, 4, 10, 64, 67])
@pytest.mark.parametrize('case', MAP_CASES)
def test_scatter_max_forward_and_backward_are_exact(case, C):
    coors, x, ref, gout = _scatter_case(case, C)
    vm = DV.map_of(coors.to(DEV), GRID, batch=2)
    xd = x.to(DEV).requires_grad_(True)
    out, arg = DV.scatter(xd, vm, DV.MAX, return_argmax=True)
    want, want_arg = DR.scatter(x, ref, 'max')
    assert torch.equal(out.detach().cpu().double(), want)                        # bit-exact
    assert torch.equal(arg.cpu().long(), want_arg)                               # lowest point index on ties
    out.backward(gout.to(DEV))
    gref = torch.zeros_like(x)
    if want_arg.numel():
        gref.index_put_((want_arg.flatten(), torch.arange(C).repeat(want_arg.shape[0])), gout.flatten(), accumulate=True)
        # (several channels / voxels never share an element: one point is the arg-max of a (voxel, channel) pair once)
    assert torch.equal(xd.grad.cpu(), gref)
    out2 = DV.scatter(x.to(DEV), vm, DV.MAX)
    assert torch.equal(out2, out.detach())


@pytest.mark.parametrize('C', [1, 4, 10, 64, 67])
@pytest.mark.parametrize('case', MAP_CASES)
def test_scatter_mean_forward_and_backward_within_the_fp32_bounds(case, C):
    coors, x, ref, gout = _scatter_case(case, C)
    vm = DV.map_of(coors.to(DEV), GRID, batch=2)
    xd = x.to(DEV).requires_grad_(True)
    out = DV.scatter(xd, vm, DV.MEAN)
    want, _ = DR.scatter(x, ref, 'avg')
    err = (out.detach().cpu().double() - want).abs()
    bound = _mean_bound(x, ref)
    print(f'MEAN {case} C={C}: worst error / bound {float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0:.3f}')
    assert (err <= bound).all()
    out.backward(gout.to(DEV))
    p2v = ref['point2voxel']
    keep = p2v >= 0
    gref = torch.zeros(x.shape, dtype=torch.float64)
    if keep.any():
        gref[keep] = (gout.double() / ref['counts'].double()[:, None])[p2v[keep]]
    got = xd.grad.cpu()
    ulp = torch.from_numpy(np.spacing(gref.float().abs().numpy())).double()
    assert ((got.double() - gref).abs() <= 2 * ulp).all()                        # within 2 ulp of g / n
    assert (got[~keep] == 0).all()
    # the order of the additions is fixed: a second run gives the same bits, forward and backward
    xd2 = x.to(DEV).requires_grad_(True)
    out2 = DV.scatter(xd2, vm, DV.MEAN)
    out2.backward(gout.to(DEV))
    assert torch.equal(out2, out) and torch.equal(xd2.grad, xd.grad)


def test_dynamic_scatter_module_three_and_four_columns():
    coors, x, ref, _ = _scatter_case('dropped', 4)
    for avg, mode in ((True, 'avg'), (False, 'max')):
        mod = DynamicScatter(VS, RNG, avg)
        feats, vc = mod(x.to(DEV), coors.to(DEV))
        want, _ = DR.scatter(x, ref, mode)
        assert torch.equal(vc.cpu(), ref['voxel_coors'].int())
        np.testing.assert_allclose(feats.cpu().numpy(), want.numpy(), rtol=1e-6, atol=1e-6)
        sel = coors[:, 0] == 1
        c3, x3 = coors[sel][:, 1:].contiguous(), x[sel]
        feats3, vc3 = mod(x3.to(DEV), c3.to(DEV))
        ref3 = DR.voxel_map(c3)
        assert vc3.shape[1] == 3 and torch.equal(vc3.cpu(), ref3['voxel_coors'].int())
        np.testing.assert_allclose(feats3.cpu().numpy(), DR.scatter(x3, ref3, mode)[0].numpy(), rtol=1e-6, atol=1e-6)
    # coordinates that come from the voxel layer carry their map: it is reused, not rebuilt
    p = _edge_frame(200, 5)[0].to(DEV)
    _, c = _layer().forward_batch([p])
    assert DV.map_of(c, GRID) is c.voxel_map


# ---- encoders ---------------------------------------------------------------------------------------------------------------
def _golden_module(d, name):
    rng = tuple(float(v) for v in d['pc_range'])
    vs = tuple(float(v) for v in d[f'{name}.voxel_size'])
    if name == 'dpfn':
        cfg = dict(type='DynamicPillarFeatureNet', in_channels=4, feat_channels=(64,), voxel_size=vs, point_cloud_range=rng)
    elif name == 'simple':
        cfg = dict(type='DynamicSimpleVFE', voxel_size=vs, point_cloud_range=rng)
    else:
        cfg = dict(type='DynamicVFE', in_channels=4, feat_channels=[32, 64], with_cluster_center=True, with_voxel_center=True,
                   voxel_size=vs, point_cloud_range=rng, mode=name.split('_')[1])
    m = VOXEL_ENCODERS.build(cfg)
    m.load_state_dict({k: torch.from_numpy(d[f'{name}.init.{k}']) for k in m.state_dict()})
    return m.to(DEV)


def _golden_input(d, name):
    """Points and their cells from the voxel layer (so the map is the batch's own)."""
    sizes = d['frame_sizes'].tolist()
    pts = torch.from_numpy(d['points'])
    layer = _layer([float(v) for v in d[f'{name}.voxel_size']], [float(v) for v in d['pc_range']])
    cat, coors = layer.forward_batch([pts[:sizes[0]].to(DEV), pts[sizes[0]:].to(DEV)])
    assert torch.equal(coors.cpu(), torch.from_numpy(d[f'{name}.coors']))
    return cat, coors


def _check_against_golden(d, name, m, out, vc):
    assert torch.equal(vc.cpu(), torch.from_numpy(d[f'{name}.voxel_coors']))
    np.testing.assert_allclose(out.detach().cpu().numpy(), d[f'{name}.out'], rtol=1e-4, atol=1e-4)
    out.backward(torch.from_numpy(d[f'{name}.grad_out']).to(DEV))
    for k, p in m.named_parameters():
        want = d[f'{name}.grad.{k}']
        rel = np.abs(p.grad.cpu().numpy() - want).max() / np.abs(want).max()
        print(f'GRAD {name} {k}: max|d| / max|ref| = {rel:.2e}')
        assert rel < 2e-4, (name, k, rel)
    for k, v in m.state_dict().items():
        if k.endswith('running_mean'):
            np.testing.assert_allclose(v.cpu().numpy(), d[f'{name}.after.{k}'], rtol=1e-4, atol=1e-7)
        elif k.endswith('running_var'):
            np.testing.assert_allclose(v.cpu().numpy(), d[f'{name}.after.{k}'], rtol=1e-5)
        elif k.endswith('num_batches_tracked'):
            assert int(v) == 1


@pytest.mark.parametrize('name', ['dpfn', 'dpfn_eager', 'vfe_max', 'vfe_avg'])
def test_dynamic_encoders_against_the_golden(golden, name, monkeypatch):
    from gga_amd import voxel_encoders as VE
    monkeypatch.setattr(VE, 'DYNAMIC_PFN_FUSED', name != 'dpfn_eager')          # dpfn: the fused kernels; dpfn_eager: the off-switch
    name = name.split('_eager')[0]
    d = golden('dynamic_voxel')
    m = _golden_module(d, name).train()
    if name == 'dpfn':
        assert m.fusable_config() == VE.DYNAMIC_PFN_FUSED
    cat, coors = _golden_input(d, name)
    before = cat.clone()
    out, vc = m(cat, coors)
    assert torch.equal(cat, before)                                              # the input tensor is left untouched
    _check_against_golden(d, name, m, out, vc)


def test_dynamic_simple_vfe_against_the_golden(golden):
    d = golden('dynamic_voxel')
    m = _golden_module(d, 'simple')
    cat, coors = _golden_input(d, 'simple')
    out, vc = m(cat, coors)
    assert torch.equal(vc.cpu(), torch.from_numpy(d['simple.voxel_coors'])) and not out.requires_grad
    np.testing.assert_allclose(out.cpu().numpy(), d['simple.out'], rtol=1e-4, atol=1e-4)


def test_dynamic_vfe_point_feats(golden):
    d = golden('dynamic_voxel')
    m = _golden_module(d, 'vfe_max').train()
    m.return_point_feats = True
    cat, coors = _golden_input(d, 'vfe_max')
    pf = m(cat, coors)
    layers, _ = DR.golden_layers(d, 'vfe_max', requires_grad=False)
    r = DR.dynamic_encoder(cat.cpu(), coors.cpu(), layers, d['vfe_max.voxel_size'].tolist(), d['pc_range'].tolist(), True, True)
    np.testing.assert_allclose(pf.detach().cpu().numpy(), r['point_feats'].numpy(), rtol=1e-4, atol=1e-4)


def _long_pillar_case():
    """About 5 000 points of two frames on the PointPillars grid, one pillar holding more than two split chunks."""
    g = torch.Generator().manual_seed(21)
    frames = []
    for b, n in enumerate((2600, 2400)):
        p = torch.rand(n, 4, generator=g)
        p[:, 0] = p[:, 0] * 30.0 + 1.0
        p[:, 1] = p[:, 1] * 30.0 - 15.0
        p[:, 2] = p[:, 2] * 3.5 - 2.9
        if b == 1:          # 2 * CHUNK + 40 points of one pillar (cell 0.16 m), interleaved with the others
            rows = torch.randperm(n, generator=g)[:2 * CHUNK + 40]
            p[rows, 0] = 8.0 + 0.01 + 0.14 * torch.rand(rows.shape[0], generator=g)
            p[rows, 1] = 0.0 + 0.01 + 0.14 * torch.rand(rows.shape[0], generator=g)
        frames.append(p)
    return frames


def test_fused_pillar_encoder_equals_its_eager_path_with_a_long_pillar(golden, monkeypatch):
    from gga_amd import voxel_encoders as VE
    vs, rng = [0.16, 0.16, 4], [0, -39.68, -3, 69.12, 39.68, 1]
    frames = _long_pillar_case()
    cat, coors = _layer(vs, rng).forward_batch([f.to(DEV) for f in frames])
    vm = coors.voxel_map
    longest = int((vm.voxel_start[1:vm.m + 1] - vm.voxel_start[:vm.m]).max())
    assert longest > 2 * CHUNK and vm.host_counts()[1] == cat.shape[0]
    results = {}
    for fused in (True, False):
        monkeypatch.setattr(VE, 'DYNAMIC_PFN_FUSED', fused)
        torch.manual_seed(4)
        m = VOXEL_ENCODERS.build(dict(type='DynamicPillarFeatureNet', in_channels=4, feat_channels=(64,), voxel_size=tuple(vs),
                                      point_cloud_range=tuple(rng))).to(DEV).train()
        with torch.no_grad():
            m.pfn_layers[0][1].weight.uniform_(0.5, 1.5)
            m.pfn_layers[0][1].bias.uniform_(-0.3, 0.3)
        before = cat.clone()
        out, vc = m(cat, coors)
        assert torch.equal(cat, before)                                          # the input tensor is left untouched
        gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
        out.backward(gy)
        results[fused] = (out.detach().cpu().numpy(), vc.cpu(), {k: p.grad.cpu().numpy() for k, p in m.named_parameters()},
                          m.pfn_layers[0][1].running_mean.cpu().numpy(), m.pfn_layers[0][1].running_var.cpu().numpy())
        if fused:       # capacity form: the same rows, zeros past the device-side count
            m2 = copy.deepcopy(m)
            cap, cvc = m2(cat, coors, capacity=True)
            assert cap.shape[0] == cat.shape[0] and int(cvc.num_valid) == vm.m
            assert torch.equal(cap[vm.m:], torch.zeros_like(cap[vm.m:])) and torch.equal(cvc[:vm.m], vc)
    (fo, fvc, fg, frm, frv), (eo, evc, eg, erm, erv) = results[True], results[False]
    assert torch.equal(fvc, evc)
    np.testing.assert_allclose(fo, eo, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(frm, erm, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(frv, erv, rtol=1e-5)
    for k in eg:
        rel = np.abs(fg[k] - eg[k]).max() / np.abs(eg[k]).max()
        print(f'FUSED_VS_EAGER grad {k}: max|d| / max|ref| = {rel:.2e}')
        assert rel < 2e-4, (k, rel)


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('training', [True, False])
def test_dynamic_pillar_encoder_with_dropped_points_and_eval_mode(golden, training, fused, monkeypatch):
    """10 % of the points out of range: the result is the restatement's on the points that are left (a dropped point takes
    part in nothing, BatchNorm statistics included); eval mode uses the running statistics."""
    from gga_amd import voxel_encoders as VE
    monkeypatch.setattr(VE, 'DYNAMIC_PFN_FUSED', fused)
    d = golden('dynamic_voxel')
    m = _golden_module(d, 'dpfn').train(training)
    sizes = d['frame_sizes'].tolist()
    pts = torch.from_numpy(d['points']).clone()
    g = torch.Generator().manual_seed(3)
    out_rows = torch.randperm(pts.shape[0], generator=g)[:pts.shape[0] // 10]
    pts[out_rows, 0] = -5.0 - torch.rand(out_rows.shape[0], generator=g)
    frames = [pts[:sizes[0]], pts[sizes[0]:]]
    vs, rng = d['dpfn.voxel_size'].tolist(), d['pc_range'].tolist()
    cat, coors = _layer(vs, rng).forward_batch([f.to(DEV) for f in frames])
    out, vc = m(cat, coors)
    layers, _ = DR.golden_layers(d, 'dpfn', requires_grad=False)
    r = DR.dynamic_encoder(pts, DR.point_coors(frames, vs, rng), layers, vs, rng, True, True, training=training)
    assert int(r['kept'].sum()) == pts.shape[0] - out_rows.shape[0]
    assert torch.equal(vc.cpu().long(), r['voxel_coors'])
    np.testing.assert_allclose(out.detach().cpu().numpy(), r['out'].numpy(), rtol=1e-4, atol=1e-4)
    bn = m.pfn_layers[0][1]
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), r['running'][0][0].numpy(), rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), r['running'][0][1].numpy(), rtol=1e-5)


def test_dynamic_pfn_with_no_kept_point():
    """Every point out of range (kept count 0), training mode: the statistics kernel that the hard and the dynamic fused fronts
    share takes its `no rows, no running-statistics update` branch, which only the dynamic front asks for."""
    coors = _coors_case('all_out').to(DEV)
    n = coors.shape[0]
    vm = DV.map_of(coors, GRID, batch=2)
    assert vm.host_counts() == (0, 0)
    g = torch.Generator().manual_seed(5)
    pts = torch.randn(n, 4, generator=g).to(DEV)
    w = torch.randn(64, 10, generator=g).to(DEV).requires_grad_(True)
    gamma = (torch.rand(64, generator=g) + 0.5).to(DEV).requires_grad_(True)
    beta = torch.randn(64, generator=g).to(DEV).requires_grad_(True)
    rm, rv = torch.randn(64, generator=g).to(DEV), (torch.rand(64, generator=g) + 0.5).to(DEV)
    rm0, rv0 = rm.clone(), rv.clone()
    prm = F.pfn_params(VS, [VS[a] / 2 + RNG[a] for a in range(3)], 1e-3, 0.01, True)
    out = DV.fused_pfn(pts, coors, vm, w, gamma, beta, rm, rv, prm)              # capacity form: n rows
    assert out.shape == (n, 64) and torch.equal(out, torch.zeros_like(out))
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)                         # bit for bit
    saved = out.grad_fn.saved_tensors[7]
    assert saved.numel() == _lib.PFN_SAVED_DOUBLES and float(saved[_lib.PFN_SAVED_DOUBLES - 1]) == 1.0
    out.backward(torch.randn(n, 64, generator=g).to(DEV))
    for p in (w, gamma, beta):
        assert bool(torch.isfinite(p.grad).all()) and torch.equal(p.grad, torch.zeros_like(p.grad))


# ---- detector -------------------------------------------------------------------------------------------------------------
DV_CFGS = {'pp': ('gga_kitti_dv_pointpillars_config.py', 'gga_kitti_pointpillars_config.py', synthetic.RANGE_PP),
           'second': ('gga_kitti_dv_config.py', 'gga_kitti_config.py', synthetic.RANGE_SECOND)}


def _damp_heads(model):
    with torch.no_grad():       # keep exp(log-dims) finite on noise inputs
        for th in model.pts_bbox_head.task_heads:
            for name in ('reg', 'height', 'dim', 'rot'):
                getattr(th, name)[-1].weight.mul_(0.05)


def _losses(model, data, srl):
    feats = model.extract_feat(data['points'], None, data['img_metas'])[1]
    outs = model.pts_bbox_head(feats)
    return model.pts_bbox_head.loss(data['gt_bboxes_3d'], data['gt_labels_3d'], outs, data['GGA_boxes_img'], data['GGA_lidar2img'],
                                    data['GGA_init_pseudo_labels'], data['GGA_bdry_masks'], data['GGA_in_box_points'],
                                    data['img_metas'], srl=srl)


@pytest.mark.parametrize('case', ['pp', 'second'])
def test_detector_trains_a_step_and_tests_a_frame(case):
    dv_cfg, hard_cfg, rng = DV_CFGS[case]
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', dv_cfg))
    torch.manual_seed(0)
    model = build_model(cfg.model).to(DEV).train()
    _damp_heads(model)
    b = synthetic.make_batch(2, n_points=2000, pc_range=rng)
    data = {k: b[k] for k in synthetic.BATCH_KEYS + ('img_metas',)}
    data['points'] = [p.to(DEV) for p in b['points']]
    srl = model.pts_bbox_head.draw_srl(2)
    out = _losses(model, data, srl)
    assert len(out) == 18 and all(np.isfinite(float(v)) for v in out.values())
    if case == 'pp':        # the fused front and the eager one (off-switch) agree on every loss
        from gga_amd import voxel_encoders as VE
        assert model.pts_voxel_encoder.fusable_config() and not model.front_reads_counts
        eager = copy.deepcopy(model)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(VE, 'DYNAMIC_PFN_FUSED', False)
            assert eager.front_reads_counts
            want = _losses(eager, data, srl)
        for k, v in want.items():
            assert abs(float(out[k]) - float(v)) / max(abs(float(v)), 1.0) <= 1e-4, (k, float(out[k]), float(v))
    model._parse_losses(out)[0].backward()
    # every parameter that gets a gradient in the hard counterpart gets one here
    hard = build_model(Config.fromfile(os.path.join(REPO, 'configs', 'gga', hard_cfg)).model).to(DEV).train()
    _damp_heads(hard)
    hard.train_step(data)['loss'].backward()
    with_grad = {k for k, p in hard.named_parameters() if p.grad is not None and not k.startswith('pts_voxel_encoder.')}
    ours = dict(model.named_parameters())
    assert len(with_grad) > 50
    for k in with_grad:
        assert ours[k].grad is not None and torch.isfinite(ours[k].grad).all(), k
    for k, p in model.pts_voxel_encoder.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    model.eval()
    res = model(return_loss=False, points=[data['points']], img_metas=[b['img_metas']])
    assert len(res) == 2
    for r in res:
        n = len(r['pts_bbox']['boxes_3d'])
        assert r['pts_bbox']['boxes_3d'].tensor.shape == (n, 7) and r['pts_bbox']['scores_3d'].shape == (n,)


@pytest.mark.parametrize('fused', [True, False])
def test_runner_steps_with_the_dynamic_front_on_the_side_stream(fused, monkeypatch):
    from gga_amd import voxel_encoders as VE
    from gga_amd.cnn import to_channels_last
    from gga_amd.train import Runner
    monkeypatch.setattr(VE, 'DYNAMIC_PFN_FUSED', fused)
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', DV_CFGS['pp'][0]))
    cfg.model.pts_middle_encoder['channels_last'] = True
    torch.manual_seed(0)
    model = to_channels_last(build_model(cfg.model).to(DEV))
    _damp_heads(model)
    runner = Runner(model, cfg, max_iters=100)
    b = synthetic.make_batch(2, n_points=2000, pc_range=synthetic.RANGE_PP)
    b['points'] = [p.to(DEV) for p in b['points']]
    data = {k: b[k] for k in synthetic.BATCH_KEYS + ('img_metas',)}
    runner.prefetch(data)
    prep = runner._prepared_for(data)
    if fused:       # nothing of the fused front is read back: no prefetch, the front runs inside the step
        assert prep is None and not model.front_reads_counts
        prep = (model.prepare_inputs(data['points']),)
    assert prep is not None and prep[0].coors.voxel_map is not None and prep[0].num_points is None
    assert any(t is prep[0].coors.voxel_map.order for t in prep[0].tensors())     # the map travels with the prepared inputs
    first = float(runner.step(data)['loss'])
    second = float(runner.step(data)['loss'])
    assert np.isfinite(first) and np.isfinite(second)


@pytest.mark.parametrize('case', ['pp', 'second'])
def test_train_and_test_flow_from_a_kitti_tree(case, tmp_path):
    """tools/train.py's flow (dataset -> pipeline -> loader -> train_detector -> checkpoint) and tools/test.py's (checkpoint ->
    detector -> detections of every frame -> evaluate) with the dynamic configs on the synthetic on-disk KITTI tree."""
    from gga_amd import loader as LD
    from gga_amd.apis import generate_pseudo_labels
    from gga_amd.cnn import to_channels_last
    from gga_amd.train import train_detector
    from test_loader import dataset_cfg, kitti_tree, matching_cfg
    dv_cfg, _, rng = DV_CFGS[case]
    path = os.path.join(REPO, 'configs', 'gga', dv_cfg)
    infos = kitti_tree(str(tmp_path))
    ds = LD.build_dataset(dataset_cfg(str(tmp_path), infos, times=2, point_range=list(rng)))
    cfg = Config.fromfile(path)
    cfg.model.pts_middle_encoder['channels_last'] = True
    cfg.data = dict(samples_per_gpu=3, workers_per_gpu=0)
    cfg.runner = dict(type='EpochBasedRunner', max_epochs=1)
    cfg.work_dir, cfg.seed = str(tmp_path / 'work'), 0
    cfg.checkpoint_config = dict(interval=1)
    np.random.seed(0), torch.manual_seed(0)
    model = build_model(cfg.model)
    _damp_heads(model)
    with torch.no_grad():
        for th in model.pts_bbox_head.task_heads:
            th.heatmap[-1].bias.fill_(0.5)                 # a random-init detector that reports boxes
    model = to_channels_last(model.to(DEV)).train()
    runner = train_detector(model, ds, cfg, distributed=False, device=torch.device(DEV))
    ck = os.path.join(cfg.work_dir, 'epoch_1.pth')
    assert runner.iter == 2 and os.path.exists(ck)
    tcfg = matching_cfg(str(tmp_path), infos, path)
    outputs, res = generate_pseudo_labels(tcfg, ck, eval_metrics=('mAP',), eval_options=dict(pseudo_label_file=str(tmp_path / 'pseudo.pkl')))
    assert len(outputs) == 3 and all(set(o['pts_bbox']) >= {'boxes_3d', 'scores_3d', 'labels_3d'} for o in outputs)
    assert res['pseudo_labels/frames'] == 3.0
