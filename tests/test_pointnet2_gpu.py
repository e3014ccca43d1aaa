"""The PointNet++ point operators (gga_amd/pointnet2.py on gga_amd/csrc/pointnet2.hip) on the device against the CPU
restatement of tests/_pointnet2_ref.py: indices and forward values bit for bit, gradients against float64 autograd within the
bound of a float32 sum of k terms, ``|err| <= k * 2^-24 * sum|t_i|``."""
import numpy as np
import pytest
import torch

import _pointnet2_ref as R
from gga_amd import ops
from gga_amd import pointnet2 as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _same_bits(got, want):
    got = got.detach().cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), f'{int((got != want).sum())} of {got.size} elements differ'


def test_ops_are_reexported():
    for name in ('furthest_point_sample', 'gather_points', 'ball_query', 'grouping_operation', 'three_nn', 'three_interpolate',
                 'QueryAndGroup', 'GroupAll', 'PointsSampler'):
        assert getattr(ops, name) is getattr(P, name)


# ----------------------------------------------------------------------------- furthest point sampling
_FPS = {}


def _fps_clouds(N):
    """Four clouds of N points (random, random on another scale, a coarse integer grid with many duplicated points and equal
    distances, all points equal) and their full sampling order: the first k entries are the answer for num_points = k."""
    if N not in _FPS:
        rng = np.random.default_rng(N)
        xyz = np.stack([rng.uniform(-1, 1, (N, 3)), rng.normal(0, 7, (N, 3)), rng.integers(0, 3, (N, 3)).astype(np.float64),
                        np.full((N, 3), 0.37)]).astype(np.float32)
        _FPS[N] = (xyz, R.furthest_point_sample(xyz, N))
    return _FPS[N]


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 1023, 1025, 2500])
def test_furthest_point_sample_matches_bit_for_bit(N, general, monkeypatch):
    # N <= 1024 runs the one-point-per-thread register kernel, 1025 and 2500 the four-point one; `general` forces the any-N
    # kernel (GGA_FPS_GENERAL=1) on the same clouds
    monkeypatch.setattr(P, 'FPS_GENERAL', general)
    xyz, full = _fps_clouds(N)
    assert len(np.unique(xyz[2], axis=0)) < N or N == 1            # the grid cloud has duplicated points
    for k in sorted({1, N, max(1, N // 3)}):
        got = P.furthest_point_sample(_dev(xyz), k)
        assert got.dtype == torch.int32
        _same_bits(got, np.ascontiguousarray(full[:, :k]))


def test_furthest_point_sample_tie_rule():
    # all points equal: every round's maximum is shared by every point, so every sample is index 0; duplicated points: of two
    # equal candidates the lower index is taken
    xyz = np.zeros((1, 130, 3), np.float32)
    assert P.furthest_point_sample(_dev(xyz), 130).cpu().numpy().tolist() == [[0] * 130]
    xyz = np.array([[[0, 0, 0], [1, 0, 0], [-1, 0, 0], [1, 0, 0], [0, 2, 0], [0, 2, 0]]], np.float32)
    want = R.furthest_point_sample(xyz, 4)
    assert want.tolist() == [[0, 4, 1, 2]]
    _same_bits(P.furthest_point_sample(_dev(xyz), 4), want)


@pytest.mark.parametrize('N,k', [(4097, 40), (20000, 2048)])
def test_furthest_point_sample_twenty_points_per_thread(N, k):
    # N > 4096 keeps twenty points per thread in registers: once just past the threshold, once at the VoteNet config's shape
    rng = np.random.default_rng(3)
    xyz = np.stack([rng.uniform(-3, 3, (N, 3)), rng.normal(0, 2, (N, 3))]).astype(np.float32)
    _same_bits(P.furthest_point_sample(_dev(xyz), k), R.furthest_point_sample(xyz, k))


def test_furthest_point_sample_rejects_more_samples_than_points():
    with pytest.raises(RuntimeError, match='num_points 5 > N 4'):
        P.furthest_point_sample(torch.zeros(1, 4, 3, device=DEV), 5)


def test_points_sampler():
    xyz, full = _fps_clouds(65)
    got = P.PointsSampler([20])(_dev(xyz), None)
    _same_bits(got, np.ascontiguousarray(full[:, :20]))
    with pytest.raises(NotImplementedError, match='F-FPS'):
        P.PointsSampler([20], ['F-FPS'], [-1])


# ----------------------------------------------------------------------------- ball query
MAX_R, MIN_R = 0.3, 0.1


def _ball_case(N, M):
    """Points in the unit cube. Point 0 and centre 0 are the origin (d2 == 0); the last point lies exactly on the outer radius
    of centre 0 (d2 == float32(r)^2: excluded), the one before exactly on the inner radius (included); centre 1 is far from
    every point; centre 2 sits in a corner (few neighbours), the rest anywhere."""
    rng = np.random.default_rng(N * 1000 + M)
    xyz = rng.uniform(0, 1, (2, N, 3)).astype(np.float32)
    centre = rng.uniform(0, 1, (2, M, 3)).astype(np.float32)
    xyz[:, 0] = 0
    centre[:, 0] = 0
    if N > 1:
        xyz[:, N - 1] = [np.float32(MAX_R), 0, 0]
    if N > 2:
        xyz[:, N - 2] = [0, np.float32(MIN_R), 0]
    if M > 1:
        centre[:, 1] = 10
    if M > 2:
        centre[:, 2] = 0.98
    return xyz, centre


@pytest.mark.parametrize('K', [1, 16, 64])
@pytest.mark.parametrize('M', [1, 63, 130])
@pytest.mark.parametrize('N', [1, 65, 300])
def test_ball_query_matches_bit_for_bit(N, M, K):
    xyz, centre = _ball_case(N, M)
    for min_r in (0.0, MIN_R):
        want = R.ball_query(min_r, MAX_R, K, xyz, centre)
        got = P.ball_query(min_r, MAX_R, K, _dev(xyz), _dev(centre))
        assert got.dtype == torch.int32
        _same_bits(got, want)
        # what the case is there for: the origin is a hit of centre 0 under either inner radius (d2 == 0), the point on the outer
        # radius never is, the one on the inner radius is
        row = want[0, 0].tolist()
        assert row[0] == 0 and N - 1 not in row[1:] or N == 1
        if M > 1:
            assert not want[:, 1].any()             # no neighbour: index 0 in every slot
    if N == 300 and M == 130:
        hits = [int(((R.d2(xyz[0], centre[0, m]) < np.float32(MAX_R) ** 2)).sum()) for m in range(M)]
        assert min(hits) == 0 and any(0 < h < 16 for h in hits) and any(h > 16 for h in hits)
        assert N - 2 in R.ball_query(MIN_R, MAX_R, 64, xyz, centre)[0, 0].tolist()


# ----------------------------------------------------------------------------- three_nn
@pytest.mark.parametrize('n', [1, 130])
@pytest.mark.parametrize('m', [3, 4, 65, 300])
def test_three_nn_matches_bit_for_bit(m, n):
    rng = np.random.default_rng(m * 10 + n)
    source = rng.uniform(-1, 1, (2, m, 3)).astype(np.float32)
    source[:, 1] = source[:, 0]                         # duplicated source points: equal distances, the earlier index in front
    if m > 4:
        source[:, m - 1] = source[:, 2]
        source[:, m // 2] = source[:, 0]
    target = rng.uniform(-1, 1, (2, n, 3)).astype(np.float32)
    target[:, 0] = source[:, 0]
    want_d, want_i = R.three_nn(target, source)
    dist, idx = P.three_nn(_dev(target), _dev(source))
    assert want_i[0, 0, :2].tolist() == [0, 1] and want_d[0, 0, 0] == 0
    _same_bits(idx, want_i)
    _same_bits(dist, want_d)


def test_three_nn_needs_three_source_points():
    with pytest.raises(RuntimeError, match='m 2 < 3'):
        P.three_nn(torch.zeros(1, 4, 3, device=DEV), torch.zeros(1, 2, 3, device=DEV))


# ----------------------------------------------------------------------------- gather / grouping / interpolation
def _check_sum(got, want, abs_sum, count, what):
    excess = R.summation_excess(got, want, abs_sum, count)
    assert excess <= 0, f'{what}: |err| exceeds k * 2^-24 * sum|t_i| by {excess:.3e}'


def _grads64(fn, inputs, grad_out):
    xs = [x.detach().cpu().double().requires_grad_(True) for x in inputs]
    return torch.autograd.grad(fn(*xs), xs, grad_out.detach().cpu().double())


@pytest.mark.parametrize('shape', [(2, 5, 70, (33,)), (2, 5, 70, (33, 9)), (1, 3, 300, (130, 2))])
def test_gather_and_grouping(shape):
    B, C, N, J = shape
    rng = np.random.default_rng(len(J) * 100 + N)
    feat = rng.normal(0, 1, (B, C, N)).astype(np.float32)
    idx = rng.integers(0, N, (B,) + J).astype(np.int32)
    idx[-1] = 0                                         # point 0 of the last cloud is hit by every entry: k = M (* K) terms
    op = P.gather_points if len(J) == 1 else P.grouping_operation
    f = _dev(feat, True)
    out = op(f, _dev(idx))
    _same_bits(out, R.group_points(feat, idx))
    gout = torch.from_numpy(rng.normal(0, 1, out.shape).astype(np.float32))
    out.backward(gout.to(DEV))
    fn = lambda x: R.group_points_t(x, torch.from_numpy(idx))
    want, = _grads64(fn, [f], gout)
    abs_sum, = _grads64(fn, [f], gout.abs())
    count, = _grads64(fn, [f], torch.ones_like(gout))
    assert int(count[-1, 0, 0]) == int(np.prod(J))
    _check_sum(f.grad, want, abs_sum, count, 'grad_features')


@pytest.mark.parametrize('shape', [(2, 5, 3, 1), (2, 7, 65, 130), (1, 2, 300, 700)])
def test_three_interpolate(shape):
    B, C, m, n = shape
    rng = np.random.default_rng(m + n)
    feat = rng.normal(0, 1, (B, C, m)).astype(np.float32)
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    idx[-1] = 0                                         # source point 0 of the last cloud takes all 3 n terms
    w = rng.uniform(0, 1, (B, n, 3)).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    f = _dev(feat, True)
    out = P.three_interpolate(f, _dev(idx), _dev(w))
    _same_bits(out, R.three_interpolate(feat, idx, w))
    gout = torch.from_numpy(rng.normal(0, 1, out.shape).astype(np.float32))
    out.backward(gout.to(DEV))
    tidx, tw = torch.from_numpy(idx), torch.from_numpy(w).double()
    want, = _grads64(lambda x: R.three_interpolate_t(x, tidx, tw), [f], gout)
    abs_sum, = _grads64(lambda x: R.three_interpolate_t(x, tidx, tw), [f], gout.abs())            # the weights are positive
    count, = _grads64(lambda x: R.three_interpolate_t(x, tidx, torch.ones_like(tw)), [f], torch.ones_like(gout))
    assert int(count[-1, 0, 0]) == 3 * n
    _check_sum(f.grad, want, abs_sum, count, 'grad_features')


# ----------------------------------------------------------------------------- QueryAndGroup
def _group_case(N, M, C, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 1, (2, N, 3)).astype(np.float32)
    centre = xyz[:, rng.integers(0, N, M)].copy() + rng.normal(0, 0.02, (2, M, 3)).astype(np.float32)
    centre[1] += 10                                     # no centre of the second cloud has a neighbour: every group is point 0,
    feat = rng.normal(0, 1, (2, C, N)).astype(np.float32) if C else None      # which is hit k = M * K times
    return xyz, centre.astype(np.float32), feat


@pytest.mark.parametrize('N,M,C,K,use_xyz,normalize', [
    (70, 33, 5, 9, True, True), (70, 33, 5, 9, True, False), (70, 33, 5, 9, False, False),
    (300, 6, 3, 70, True, True), (300, 6, 3, 70, False, False),          # more samples than a wave has lanes
    (65, 130, 0, 16, True, True), (65, 130, 0, 16, True, False)])         # coordinates only
def test_query_and_group_fused_and_composed(N, M, C, K, use_xyz, normalize):
    radius = 0.3
    xyz, centre, feat = _group_case(N, M, C, N + M)
    want_idx = R.ball_query(0.0, radius, K, xyz, centre)
    assert not want_idx[1].any() and want_idx[0].any()
    want = R.query_and_group(xyz, centre, feat, want_idx, radius, use_xyz, normalize)
    rng = np.random.default_rng(K)
    gout = torch.from_numpy(rng.normal(0, 1, want.shape).astype(np.float32))
    tidx = torch.from_numpy(want_idx)

    def fn64(norm_radius):
        def fn(*xs):
            xs = list(xs)
            p, c = (xs.pop(0), xs.pop(0)) if use_xyz else (torch.from_numpy(xyz).double(), torch.from_numpy(centre).double())
            f = xs.pop(0) if C else None
            return R.query_and_group_t(p, c, f, tidx, norm_radius, use_xyz, normalize)
        return fn

    for fused in (True, False):
        p, c, f = _dev(xyz, True), _dev(centre, True), (_dev(feat, True) if C else None)
        grouper = P.QueryAndGroup(radius, K, use_xyz=use_xyz, normalize_xyz=normalize, return_grouped_idx=True)
        was, P.GROUP_FUSED = P.GROUP_FUSED, fused              # GGA_SA_GROUP_FUSED=0
        try:
            out, idx = grouper(p, c, f)
        finally:
            P.GROUP_FUSED = was
        _same_bits(idx, want_idx)
        _same_bits(out, want)
        out.backward(gout.to(DEV))
        inputs = ([p, c] if use_xyz else []) + ([f] if C else [])
        names = (['points_xyz', 'center_xyz'] if use_xyz else []) + (['features'] if C else [])
        wants = _grads64(fn64(radius), inputs, gout)
        abs_sums = _grads64(fn64(radius), inputs, gout.abs())               # the terms are +-g / r and g: |t| = |g| / r, |g|
        for name, x, want_g, abs_sum in zip(names, inputs, wants, abs_sums):
            assert x.grad is not None, f'{name} received no gradient (fused={fused})'
            _check_sum(x.grad, want_g, abs_sum, _count(name, tidx, N, K), f'grad_{name} (fused={fused})')
        if use_xyz:
            assert int(_count('points_xyz', tidx, N, K)[1, 0, 0]) == M * K


def _count(name, idx, N, K):
    """How many terms each gradient element sums: a point (and its features) one per group entry that names it, a centre K."""
    B, M, _ = idx.shape
    if name == 'center_xyz':
        return torch.full((B, M, 3), float(K), dtype=torch.float64)
    hits = torch.stack([torch.bincount(idx[b].reshape(-1).long(), minlength=N) for b in range(B)]).double()
    return hits[:, :, None].expand(B, N, 3) if name == 'points_xyz' else hits[:, None, :]


def test_query_and_group_given_indices_and_group_all():
    N, M, C, K = 70, 33, 4, 9
    xyz, centre, feat = _group_case(N, M, C, 5)
    idx = np.random.default_rng(0).integers(0, N, (2, M, K)).astype(np.int32)
    out = P.QueryAndGroup(0.3, K, normalize_xyz=True)(_dev(xyz), _dev(centre), _dev(feat), indices=_dev(idx))
    _same_bits(out, R.query_and_group(xyz, centre, feat, idx, 0.3, True, True))
    out = P.GroupAll()(_dev(xyz), None, _dev(feat))
    _same_bits(out, np.concatenate([xyz.transpose(0, 2, 1)[:, :, None], feat[:, :, None]], 1))
