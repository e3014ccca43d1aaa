"""CPU restatement of the PointNet++ point operators (include/gga_hip.h "Point operators", DESIGN.md "Point operators").

mmcv's sources are not part of the reference tree (the reference imports the ops from the mmcv wheel:
mmdet3d/ops/pointnet_modules/point_sa_module.py:5-8, point_fp_module.py:4), so the definitions are stated by this project
and restated here: parity with mmcv is unpinned. The numpy functions are float32 operation by operation (numpy rounds every
array operation once and fuses nothing) and give the indices and forward values the kernels must reproduce bit for bit; the
torch functions are the same maps in any dtype, for float64 autograd.
"""
import numpy as np
import torch

F32 = np.float32


def d2(a, b):
    """(dx*dx + dy*dy) + dz*dz of float32 points a [..., 3] and b [..., 3], each operation rounded once."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def furthest_point_sample(xyz, num_points):
    """xyz [B,N,3] -> int32 [B,num_points]: sample 0 first, running minima from 1e10, each round the largest minimum and the
    lowest index among equal ones (np.argmax returns the first maximum)."""
    xyz = np.asarray(xyz, F32)
    B, N, _ = xyz.shape
    assert 1 <= num_points <= N
    out = np.zeros((B, num_points), np.int32)
    for b in range(B):
        mins = np.full(N, 1e10, F32)
        last = 0
        for j in range(1, num_points):
            d = d2(xyz[b], xyz[b, last])
            mins = np.where(d < mins, d, mins)
            last = int(np.argmax(mins))
            out[b, j] = last
    return out


def ball_query(min_radius, max_radius, sample_num, xyz, center_xyz):
    """-> int32 [B,M,sample_num]: hits in ascending index, d2 < r_max^2 and (d2 == 0 or d2 >= r_min^2) with the squares in
    float32; the first hit fills every slot, later hits slots 1, 2, ...; no hit leaves index 0 (mmcv's behaviour)."""
    xyz, center_xyz = np.asarray(xyz, F32), np.asarray(center_xyz, F32)
    B, M = center_xyz.shape[:2]
    r2min, r2max = F32(min_radius) * F32(min_radius), F32(max_radius) * F32(max_radius)
    out = np.zeros((B, M, sample_num), np.int32)
    for b in range(B):
        for m in range(M):
            d = d2(xyz[b], center_xyz[b, m])
            hits = np.nonzero((d < r2max) & ((d == 0) | (d >= r2min)))[0][:sample_num]
            if len(hits):
                out[b, m, :] = hits[0]
                out[b, m, :len(hits)] = hits
    return out


def three_nn(target, source):
    """-> (dist [B,n,3] = sqrt(d2) float32, idx int32 [B,n,3]): the three smallest d2, the earlier index first on ties (a
    stable sort of the distances)."""
    target, source = np.asarray(target, F32), np.asarray(source, F32)
    B, n = target.shape[:2]
    assert source.shape[1] >= 3
    dist, idx = np.zeros((B, n, 3), F32), np.zeros((B, n, 3), np.int32)
    for b in range(B):
        for i in range(n):
            d = d2(source[b], target[b, i])
            order = np.argsort(d, kind='stable')[:3]
            idx[b, i], dist[b, i] = order, np.sqrt(d[order])
    return dist, idx


def group_points(features, idx):
    """out[b,c,...] = features[b,c,idx[b,...]]: gather_points (idx [B,M]) and grouping_operation (idx [B,M,K])."""
    features, idx = np.asarray(features), np.asarray(idx)
    return np.stack([features[b][:, idx[b]] for b in range(features.shape[0])])


def three_interpolate(features, idx, weight):
    """(w0*f0 + w1*f1) + w2*f2 in float32."""
    features, weight = np.asarray(features, F32), np.asarray(weight, F32)
    f = group_points(features, idx)                     # [B,C,n,3]
    w = weight[:, None]
    return (w[..., 0] * f[..., 0] + w[..., 1] * f[..., 1]) + w[..., 2] * f[..., 2]


def query_and_group(xyz, center_xyz, features, idx, max_radius, use_xyz=True, normalize_xyz=False):
    """cat((xyz[idx] - centre) [/ float32(max_radius), a true division], features[idx]) -> [B, 3 + C, M, K] float32."""
    xyz, center_xyz = np.asarray(xyz, F32), np.asarray(center_xyz, F32)
    parts = []
    if use_xyz:
        diff = group_points(xyz.transpose(0, 2, 1), idx) - center_xyz.transpose(0, 2, 1)[..., None]
        if normalize_xyz:
            diff = diff / F32(max_radius)
        parts.append(diff.astype(F32))
    if features is not None:
        parts.append(group_points(np.asarray(features, F32), idx))
    return np.concatenate(parts, 1)


# ----------------------------------------------------------------------------- the same maps in torch (any dtype), for autograd
def group_points_t(features, idx):
    B, C, N = features.shape
    flat = idx.reshape(B, 1, -1).long().expand(B, C, -1)
    return torch.gather(features, 2, flat).reshape((B, C) + tuple(idx.shape[1:]))


def three_interpolate_t(features, idx, weight):
    f = group_points_t(features, idx)
    w = weight[:, None]
    return (w[..., 0] * f[..., 0] + w[..., 1] * f[..., 1]) + w[..., 2] * f[..., 2]


def query_and_group_t(xyz, center_xyz, features, idx, max_radius, use_xyz=True, normalize_xyz=False):
    parts = []
    if use_xyz:
        diff = group_points_t(xyz.transpose(1, 2), idx) - center_xyz.transpose(1, 2).unsqueeze(-1)
        if normalize_xyz:
            diff = diff / float(np.float32(max_radius))
        parts.append(diff)
    if features is not None:
        parts.append(group_points_t(features, idx))
    return torch.cat(parts, 1)


def summation_excess(got, want, abs_sum, count):
    """A float32 sum of k terms t_i added in any order (float atomics) is within ``k * 2^-24 * sum|t_i|`` of the exact sum, the
    standard bound of float32 summation: -> the largest ``|got - want| - bound`` over the elements (<= 0 when all hold).
    ``want`` float64 exact sums, ``abs_sum`` = sum|t_i|, ``count`` = k, per element."""
    err = (got.detach().cpu().double() - want.cpu().double()).abs()
    return float((err - count.cpu().double().abs() * 2.0 ** -24 * abs_sum.cpu().double().abs()).max())
