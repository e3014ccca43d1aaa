"""The PointNet++ point operators on the HIP kernels of gga_amd/csrc/pointnet2.hip, under ``mmcv.ops``' names, argument
order and shapes, as the reference's point modules call them (mmdet3d/ops/pointnet_modules/point_sa_module.py:5-8,
point_fp_module.py:4, models/model_utils/vote_module.py, models/dense_heads/vote_head.py:5):

* ``furthest_point_sample(points_xyz [B,N,3], num_points) -> int32 [B,num_points]``
* ``gather_points(features [B,C,N], indices [B,M]) -> [B,C,M]``
* ``ball_query(min_radius, max_radius, sample_num, xyz [B,N,3], center_xyz [B,M,3]) -> int32 [B,M,sample_num]``
* ``grouping_operation(features [B,C,N], indices [B,M,K]) -> [B,C,M,K]``
* ``three_nn(target [B,n,3], source [B,m,3]) -> (dist [B,n,3], idx int32 [B,n,3])``
* ``three_interpolate(features [B,C,m], indices [B,n,3], weight [B,n,3]) -> [B,C,n]``
* ``QueryAndGroup``, ``GroupAll``, ``PointsSampler`` (``D-FPS`` only)
* ``group_max_pool(x [B,C,M,K]) -> [B,C,M]``: the pool over a group's samples (not an mmcv op: the reference calls
  ``F.max_pool2d`` there)

mmcv's sources are not part of the reference tree, so the definitions are this project's (include/gga_hip.h "Point
operators", DESIGN.md "Point operators"): float32 ``d2 = (dx*dx + dy*dy) + dz*dz`` rounded per operation, furthest point
sampling from index 0 with the lowest index among equal maxima, ball query in ascending index with mmcv's padding by the
first hit (index 0 for a centre without a hit), three_nn with the earlier index in front on ties. GPU only.
"""
import os

import torch
from torch import nn

from . import _lib
from . import functional as F
from ._lib import check

GROUP_FUSED = os.environ.get('GGA_SA_GROUP_FUSED', '1') != '0'      # QueryAndGroup as one launch (0: the separate ops)
FPS_GENERAL = os.environ.get('GGA_FPS_GENERAL', '0') != '0'         # force the any-N path of furthest point sampling
SA_POOL = os.environ.get('GGA_SA_POOL', '1') != '0'                 # group_max_pool on the pool kernel (0: F.max_pool2d)


def _f32(t):
    return t.detach().float().contiguous()


def _i32(t):
    return t.detach().to(torch.int32).contiguous()


@torch.no_grad()
def furthest_point_sample(points_xyz, num_points):
    F._need_cuda(points_xyz)
    assert points_xyz.dim() == 3 and points_xyz.shape[2] == 3, f'points_xyz {tuple(points_xyz.shape)} must be [B,N,3]'
    xyz = _f32(points_xyz)
    B, N, _ = xyz.shape
    out = torch.empty((B, int(num_points)), dtype=torch.int32, device=xyz.device)
    general = FPS_GENERAL or N > _lib.FPS_REGISTER_MAX_N
    temp = torch.empty((B, N), dtype=torch.float32, device=xyz.device) if general else None
    check(_lib.lib().gga_furthest_point_sample(F._p(xyz), B, N, int(num_points), int(general), F._p(temp), F._p(out),
                                               F._stream()), 'gga_furthest_point_sample')
    return out


@torch.no_grad()
def ball_query(min_radius, max_radius, sample_num, xyz, center_xyz):
    F._need_cuda(xyz, center_xyz)
    assert xyz.dim() == 3 and center_xyz.dim() == 3 and xyz.shape[0] == center_xyz.shape[0]
    assert xyz.shape[2] == 3 and center_xyz.shape[2] == 3
    p, c = _f32(xyz), _f32(center_xyz)
    B, N, _ = p.shape
    M = c.shape[1]
    idx = torch.empty((B, M, int(sample_num)), dtype=torch.int32, device=p.device)
    check(_lib.lib().gga_ball_query(F._p(p), F._p(c), B, N, M, float(min_radius), float(max_radius), int(sample_num),
                                    F._p(idx), F._stream()), 'gga_ball_query')
    return idx


class _GroupPoints(torch.autograd.Function):
    """out[b,c,j] = features[b,c,idx[b,j]] with idx [B, ...]: gather_points and grouping_operation."""

    @staticmethod
    def forward(ctx, features, indices):
        F._need_cuda(features, indices)
        assert features.dim() == 3 and indices.shape[0] == features.shape[0]
        feat, idx = _f32(features), _i32(indices)
        B, C, N = feat.shape
        J = idx[0].numel()
        out = torch.empty((B, C) + tuple(idx.shape[1:]), dtype=torch.float32, device=feat.device)
        check(_lib.lib().gga_group_points_fwd(F._p(feat), F._p(idx), B, C, N, J, F._p(out), F._stream()),
              'gga_group_points_fwd')
        ctx.save_for_backward(idx)
        ctx.n = N
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, = ctx.saved_tensors
        g = _f32(grad_out)
        B, C = g.shape[:2]
        grad = torch.zeros((B, C, ctx.n), dtype=torch.float32, device=g.device)
        check(_lib.lib().gga_group_points_bwd(F._p(g), F._p(idx), B, C, ctx.n, idx[0].numel(), F._p(grad), F._stream()),
              'gga_group_points_bwd')
        return grad, None


def gather_points(features, indices):
    assert indices.dim() == 2, f'indices {tuple(indices.shape)} must be [B,M]'
    return _GroupPoints.apply(features, indices)


def grouping_operation(features, indices):
    assert indices.dim() == 3, f'indices {tuple(indices.shape)} must be [B,M,K]'
    return _GroupPoints.apply(features, indices)


@torch.no_grad()
def three_nn(target, source):
    F._need_cuda(target, source)
    assert target.dim() == 3 and source.dim() == 3 and target.shape[0] == source.shape[0]
    assert target.shape[2] == 3 and source.shape[2] == 3
    t, s = _f32(target), _f32(source)
    B, n, _ = t.shape
    dist = torch.empty((B, n, 3), dtype=torch.float32, device=t.device)
    idx = torch.empty((B, n, 3), dtype=torch.int32, device=t.device)
    check(_lib.lib().gga_three_nn(F._p(t), F._p(s), B, n, s.shape[1], F._p(dist), F._p(idx), F._stream()), 'gga_three_nn')
    return dist, idx


class _ThreeInterpolate(torch.autograd.Function):

    @staticmethod
    def forward(ctx, features, indices, weight):
        F._need_cuda(features, indices, weight)
        assert features.dim() == 3 and indices.dim() == 3 and indices.shape == weight.shape and indices.shape[2] == 3
        feat, idx, w = _f32(features), _i32(indices), _f32(weight)
        B, C, m = feat.shape
        assert idx.shape[0] == B
        n = idx.shape[1]
        out = torch.empty((B, C, n), dtype=torch.float32, device=feat.device)
        check(_lib.lib().gga_three_interpolate_fwd(F._p(feat), F._p(idx), F._p(w), B, C, m, n, F._p(out), F._stream()),
              'gga_three_interpolate_fwd')
        ctx.save_for_backward(idx, w)
        ctx.m = m
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, w = ctx.saved_tensors
        g = _f32(grad_out)
        B, C, n = g.shape
        grad = torch.zeros((B, C, ctx.m), dtype=torch.float32, device=g.device)
        check(_lib.lib().gga_three_interpolate_bwd(F._p(g), F._p(idx), F._p(w), B, C, ctx.m, n, F._p(grad), F._stream()),
              'gga_three_interpolate_bwd')
        return grad, None, None


def three_interpolate(features, indices, weight):
    return _ThreeInterpolate.apply(features, indices, weight)


class _QueryAndGroup(torch.autograd.Function):
    """gga_query_and_group / gga_query_and_group_bwd: -> (grouped [B, 3 + C | C, M, K], idx [B,M,K]); gradients to
    ``points_xyz``, ``center_xyz`` and ``features`` (grouped coordinates carry gradient when the points are votes)."""

    @staticmethod
    def forward(ctx, points_xyz, center_xyz, features, min_radius, max_radius, sample_num, use_xyz, normalize_xyz, indices):
        F._need_cuda(points_xyz, center_xyz, features, indices)
        p, c = _f32(points_xyz), _f32(center_xyz)
        feat = _f32(features) if features is not None else None
        B, N, _ = p.shape
        M = c.shape[1]
        C = feat.shape[1] if feat is not None else 0
        K = int(sample_num)
        query = indices is None
        idx = torch.empty((B, M, K), dtype=torch.int32, device=p.device) if query else _i32(indices)
        assert tuple(idx.shape) == (B, M, K), f'indices {tuple(idx.shape)} must be [B,M,sample_num] = {(B, M, K)}'
        assert feat is None or (feat.dim() == 3 and feat.shape[0] == B and feat.shape[2] == N)
        out = torch.empty((B, (3 if use_xyz else 0) + C, M, K), dtype=torch.float32, device=p.device)
        check(_lib.lib().gga_query_and_group(F._p(p), F._p(c), F._p(feat), B, N, M, C, float(min_radius), float(max_radius), K,
                                             int(use_xyz), int(normalize_xyz), int(query), F._p(idx), F._p(out), F._stream()),
              'gga_query_and_group')
        ctx.save_for_backward(idx)
        ctx.args = (B, N, M, C, float(max_radius), K, int(use_xyz), int(normalize_xyz))
        ctx.mark_non_differentiable(idx)
        return out, idx

    @staticmethod
    def backward(ctx, grad_out, _grad_idx):
        idx, = ctx.saved_tensors
        B, N, M, C, max_radius, K, use_xyz, normalize_xyz = ctx.args
        g = _f32(grad_out)
        need = ctx.needs_input_grad
        gx = torch.zeros((B, N, 3), dtype=torch.float32, device=g.device) if need[0] and use_xyz else None
        gc = torch.empty((B, M, 3), dtype=torch.float32, device=g.device) if need[1] and use_xyz else None
        gf = torch.zeros((B, C, N), dtype=torch.float32, device=g.device) if need[2] and C else None
        if gx is not None or gc is not None or gf is not None:
            check(_lib.lib().gga_query_and_group_bwd(F._p(g), F._p(idx), B, N, M, C, max_radius, K, use_xyz, normalize_xyz,
                                                     F._p(gx), F._p(gc), F._p(gf), F._stream()), 'gga_query_and_group_bwd')
        return gx, gc, gf, None, None, None, None, None, None


def query_and_group(points_xyz, center_xyz, features, min_radius, max_radius, sample_num, use_xyz=True, normalize_xyz=False,
                    indices=None, fused=None):
    """Ball query (unless ``indices`` is given) and grouping -> (grouped, idx). ``fused=False`` (``GGA_SA_GROUP_FUSED=0``)
    composes the separate ops instead; the forward bits are the same."""
    assert features is not None or use_xyz, 'Cannot have not features and not use xyz as a feature!'
    fused = GROUP_FUSED if fused is None else fused
    if fused and sample_num <= _lib.GROUP_MAX_SAMPLES:
        return _QueryAndGroup.apply(points_xyz, center_xyz, features, min_radius, max_radius, sample_num, use_xyz,
                                    normalize_xyz, indices)
    idx = ball_query(min_radius, max_radius, sample_num, points_xyz, center_xyz) if indices is None else indices
    parts = []
    if use_xyz:
        diff = grouping_operation(points_xyz.transpose(1, 2).contiguous(), idx) - center_xyz.transpose(1, 2).unsqueeze(-1)
        if normalize_xyz:
            # a tensor divisor: a Python number would turn the division into a multiplication by its reciprocal
            diff = diff / torch.full((), float(max_radius), dtype=torch.float32, device=diff.device)
        parts.append(diff)
    if features is not None:
        parts.append(grouping_operation(features, idx))
    return (parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)), idx


class _GroupMaxPool(torch.autograd.Function):
    """gga_group_max_fwd / gga_group_max_bwd: x [B,C,M,K] in contiguous or channels-last memory -> [B,C,M] contiguous; the
    positions of the maxima are kept as one byte each, and the gradient comes back in x's memory format."""

    @staticmethod
    def forward(ctx, x):
        B, C, M, K = x.shape
        y = torch.empty((B, C, M), dtype=torch.float32, device=x.device)
        arg = torch.empty((B, C, M), dtype=torch.uint8, device=x.device)
        check(_lib.lib().gga_group_max_fwd(F._p(x), B, C, M, K, *x.stride(), F._p(y), F._p(arg), F._stream()),
              'gga_group_max_fwd')
        ctx.save_for_backward(arg)
        ctx.layout = (tuple(x.shape), tuple(x.stride()))
        return y

    @staticmethod
    def backward(ctx, grad_y):
        arg, = ctx.saved_tensors
        (B, C, M, K), stride = ctx.layout
        g = _f32(grad_y)
        grad_x = torch.empty_strided((B, C, M, K), stride, dtype=torch.float32, device=g.device)
        check(_lib.lib().gga_group_max_bwd(F._p(g), F._p(arg), B, C, M, K, *stride, F._p(grad_x), F._stream()),
              'gga_group_max_bwd')
        return grad_x


def _eager_max_pool(x):
    return torch.nn.functional.max_pool2d(x, kernel_size=[1, x.shape[3]]).squeeze(-1).contiguous()


def group_max_pool(x):
    """The max over the samples of every group, x [B,C,M,K] -> [B,C,M] contiguous: what the reference's set abstraction
    modules take from ``F.max_pool2d(kernel_size=[1, K])`` (point_sa_module.py:146-168). A float32 CUDA tensor in contiguous
    or channels-last memory with K <= 256 runs on the pool kernel (first maximum on ties, a NaN wins); anything else, or
    ``GGA_SA_POOL=0``, is the framework's pool."""
    own = (SA_POOL and x.dim() == 4 and x.is_cuda and x.dtype == torch.float32 and x.numel() > 0
           and x.shape[3] <= _lib.GROUP_MAX_SAMPLES
           and (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)))
    return _GroupMaxPool.apply(x) if own else _eager_max_pool(x)


class QueryAndGroup(nn.Module):
    """``mmcv.ops.QueryAndGroup``: forward(points_xyz [B,N,3], center_xyz [B,M,3], features [B,C,N] or None) ->
    [B, 3 + C, M, sample_num] (and the extras asked for, in mmcv's order: grouped_xyz, unique_cnt, grouped_idx)."""

    def __init__(self, max_radius, sample_num, min_radius=0., use_xyz=True, return_grouped_xyz=False, normalize_xyz=False,
                 uniform_sample=False, return_unique_cnt=False, return_grouped_idx=False):
        super().__init__()
        if max_radius is None:
            raise NotImplementedError('QueryAndGroup(max_radius=None): kNN grouping is not implemented')
        if uniform_sample or return_unique_cnt:
            raise NotImplementedError('QueryAndGroup(uniform_sample / return_unique_cnt) is not implemented')
        self.max_radius, self.min_radius, self.sample_num = max_radius, min_radius, sample_num
        self.use_xyz, self.normalize_xyz = use_xyz, normalize_xyz
        self.return_grouped_xyz, self.return_grouped_idx = return_grouped_xyz, return_grouped_idx

    def forward(self, points_xyz, center_xyz, features=None, indices=None):
        new_features, idx = query_and_group(points_xyz, center_xyz, features, self.min_radius, self.max_radius, self.sample_num,
                                            self.use_xyz, self.normalize_xyz, indices)
        ret = [new_features]
        if self.return_grouped_xyz:
            ret.append(grouping_operation(points_xyz.transpose(1, 2).contiguous(), idx))
        if self.return_grouped_idx:
            ret.append(idx)
        return new_features if len(ret) == 1 else tuple(ret)


class GroupAll(nn.Module):
    """``mmcv.ops.GroupAll``: every point in one group -> [B, 3 + C, 1, N]."""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return grouped_xyz
        grouped_features = features.unsqueeze(2)
        return torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features


class PointsSampler(nn.Module):
    """``mmcv.ops.PointsSampler`` with distance furthest point sampling: forward(points_xyz [B,N,3], features) ->
    int32 [B, sum(num_point)]; range i samples ``points_xyz[:, start:fps_sample_range_list[i]]`` (-1: to the end)."""

    def __init__(self, num_point, fps_mod_list=['D-FPS'], fps_sample_range_list=[-1]):
        super().__init__()
        assert len(num_point) == len(fps_mod_list) == len(fps_sample_range_list)
        for mod in fps_mod_list:
            if mod != 'D-FPS':
                raise NotImplementedError(f'PointsSampler: sampling mode {mod!r} is not implemented (only D-FPS)')
        self.num_point, self.fps_mod_list, self.fps_sample_range_list = num_point, fps_mod_list, fps_sample_range_list

    def forward(self, points_xyz, features=None):
        indices, last = [], 0
        for sample_range, npoint in zip(self.fps_sample_range_list, self.num_point):
            assert sample_range < points_xyz.shape[1]
            part = points_xyz[:, last:] if sample_range == -1 else points_xyz[:, last:sample_range]
            indices.append(furthest_point_sample(part, npoint) + last)
            last += sample_range
        return indices[0] if len(indices) == 1 else torch.cat(indices, dim=1)
