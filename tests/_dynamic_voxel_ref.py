"""Restatement of dynamic voxelization in plain torch on the CPU (test infrastructure, next to _geometry_ref.py; nothing
under gga_amd/ imports it): per-point cells, mmcv's DynamicScatter as ``torch.unique`` + float64 reductions, and the three
dynamic voxel encoders op by op in float64 (mmdet3d voxel_encoders/voxel_encoder.py:48-286, pillar_encoder.py:162-323).

One stated deviation from the reference: a point outside the grid, (b,-1,-1,-1), takes part in nothing here - the reference
feeds it through the linear layer and BatchNorm and reads its cluster centre at a wrapped canvas index. Parity with the
reference is for inputs whose points are all in range."""
import numpy as np
import torch
from torch import nn


def grid_size(voxel_size, point_cloud_range):
    """(x, y, z) cells: round((max - min) / voxel_size) in f32, as mmcv."""
    vs = np.asarray(voxel_size, np.float32)
    r = np.asarray(point_cloud_range, np.float32)
    return [int(v) for v in np.round((r[3:] - r[:3]) / vs)]


def point_coors(points, voxel_size, point_cloud_range, counts=None):
    """list of [N_b, C] f32 -> [sum N, 4] int32 (b, z, y, x); the cell is floor((p - lo) / vs) in f32 and the fp32 formula
    decides the boundaries. Out of range (or not finite, or at / past ``counts[b]``) -> (b, -1, -1, -1)."""
    lo = torch.tensor(point_cloud_range[:3], dtype=torch.float32)
    vs = torch.tensor(voxel_size, dtype=torch.float32)
    grid = torch.tensor(grid_size(voxel_size, point_cloud_range), dtype=torch.float32)
    rows = []
    for b, p in enumerate(points):
        c = torch.floor((p[:, :3].float() - lo) / vs)
        ok = ((c >= 0) & (c < grid)).all(dim=1)
        if counts is not None:
            ok &= torch.arange(p.shape[0]) < int(counts[b])
        ci = torch.where(ok[:, None], c, torch.full_like(c, -1.0)).nan_to_num(-1.0).to(torch.int32)
        rows.append(torch.cat([torch.full((p.shape[0], 1), b, dtype=torch.int32), ci.flip(1)], 1))
    return torch.cat(rows, 0) if rows else torch.zeros((0, 4), dtype=torch.int32)


def voxel_map(coors):
    """coors [N, 3|4] -> dict(voxel_coors [M, 3|4] ascending, point2voxel [N] (-1 dropped), counts [M], order [n_kept]
    (point indices grouped by voxel, ascending inside), voxel_start [M + 1])."""
    coors = coors.long()
    keep = (coors >= 0).all(dim=1)
    idx = keep.nonzero().squeeze(1)
    p2v = torch.full((coors.shape[0],), -1, dtype=torch.long)
    if idx.numel() == 0:
        return dict(voxel_coors=coors[:0], point2voxel=p2v, counts=torch.zeros(0, dtype=torch.long),
                    order=torch.zeros(0, dtype=torch.long), voxel_start=torch.zeros(1, dtype=torch.long))
    vc, inv, cnt = torch.unique(coors[idx], dim=0, return_inverse=True, return_counts=True)
    p2v[idx] = inv
    order = idx[torch.sort(inv, stable=True)[1]]
    start = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt, 0)])
    return dict(voxel_coors=vc, point2voxel=p2v, counts=cnt, order=order, voxel_start=start)


def lowest_argmax(x, vm):
    """Per voxel and channel the point holding the maximum, the lowest point index on ties (mmcv's atomicMin traceback)."""
    M, C = vm['counts'].numel(), x.shape[1]
    arg = torch.zeros((M, C), dtype=torch.long)
    for v in range(M):
        pts = vm['order'][vm['voxel_start'][v]:vm['voxel_start'][v + 1]]          # ascending point index
        seg = x[pts]
        first = (seg == seg.max(dim=0, keepdim=True)[0]).to(torch.uint8).argmax(dim=0)      # first True = lowest index
        arg[v] = pts[first]
    return arg


def scatter(x, vm, mode):
    """Differentiable mean / max of x [N, C] over the voxels of ``vm`` in float64 -> ([M, C] float64, argmax or None)."""
    M = vm['counts'].numel()
    x64 = x.double()
    if mode == 'max':
        arg = lowest_argmax(x64.detach(), vm)
        return x64.gather(0, arg) if M else x64[:0], arg
    keep = vm['point2voxel'] >= 0
    s = torch.zeros((M, x.shape[1]), dtype=torch.float64).index_add(0, vm['point2voxel'][keep], x64[keep])
    return s / vm['counts'].double()[:, None], None


class DynamicScatterRef(nn.Module):
    """Stands in for ``mmcv.ops.DynamicScatter`` when the reference's encoders are imported (tools_dev/make_golden.py):
    same constructor and ``forward(points, coors) -> (voxel_feats, voxel_coors)``, results in the input's dtype."""

    def __init__(self, voxel_size, point_cloud_range, average_points):
        super().__init__()
        self.voxel_size, self.point_cloud_range, self.average_points = voxel_size, point_cloud_range, average_points

    def forward(self, points, coors):
        vm = voxel_map(coors)
        out, _ = scatter(points, vm, 'avg' if self.average_points else 'max')
        return out.to(points.dtype), vm['voxel_coors'].to(coors.dtype)


def batch_norm(x, gamma, beta, running_mean, running_var, eps, momentum, training):
    """BatchNorm1d over the rows of x [R, C] (float64); -> (y, new running_mean, new running_var)."""
    if not training:
        return (x - running_mean) / torch.sqrt(running_var + eps) * gamma + beta, running_mean, running_var
    mean, var = x.mean(0), x.var(0, unbiased=False)
    R = x.shape[0]
    y = (x - mean) / torch.sqrt(var + eps) * gamma + beta
    new_mean = (1 - momentum) * running_mean + momentum * mean.detach()
    new_var = (1 - momentum) * running_var + momentum * var.detach() * R / max(R - 1, 1)
    return y, new_mean, new_var


def dynamic_encoder(features, coors, layers, voxel_size, point_cloud_range, with_cluster_center, with_voxel_center,
                    with_distance=False, mode='max', eps=1e-3, momentum=0.01, training=True):
    """DynamicVFE / DynamicPillarFeatureNet forward in float64. ``layers``: list of dict(weight [out, in], gamma, beta,
    running_mean, running_var) float64 tensors (weight / gamma / beta may require grad).
    -> dict(out [M, C], voxel_coors [M, 4], point_feats, running [(mean, var) per layer], kept (point mask))."""
    vm_all = voxel_map(coors)
    kept = vm_all['point2voxel'] >= 0
    f, c = features.double()[kept], coors[kept]
    vm = voxel_map(c)
    p2v = vm['point2voxel']
    cols = [f]
    if with_cluster_center:
        mean, _ = scatter(f[:, :3], vm, 'avg')
        cols.append(f[:, :3] - mean[p2v])
    if with_voxel_center:
        off = [v / 2 + float(point_cloud_range[i]) for i, v in enumerate(voxel_size)]
        cd = c.double()
        centre = torch.stack([cd[:, 3] * voxel_size[0] + off[0], cd[:, 2] * voxel_size[1] + off[1],
                              cd[:, 1] * voxel_size[2] + off[2]], 1)
        cols.append(f[:, :3] - centre)
    if with_distance:
        cols.append(torch.norm(f[:, :3], 2, 1, keepdim=True))
    x = torch.cat(cols, 1)
    running = []
    for i, L in enumerate(layers):
        z = x @ L['weight'].t()
        y, rm, rv = batch_norm(z, L['gamma'], L['beta'], L['running_mean'], L['running_var'], eps, momentum, training)
        pf = torch.relu(y)
        running.append((rm, rv))
        vf, _ = scatter(pf, vm, mode)
        if i != len(layers) - 1:
            x = torch.cat([pf, vf[p2v]], 1)
    return dict(out=vf, voxel_coors=vm['voxel_coors'], point_feats=pf, running=running, kept=kept)


def golden_layers(d, name, requires_grad=True):
    """Layer dicts of :func:`dynamic_encoder` from the initial state of module ``name`` in tests/golden/dynamic_voxel.npz
    (``<stack>.<i>.0`` = Linear, ``<stack>.<i>.1`` = BatchNorm1d) -> (layers, stack name)."""
    keys = [str(k) for k in d[f'{name}.state_keys']]
    stack = keys[0].split('.')[0]
    layers = []
    for i in range(len([k for k in keys if k.endswith('.0.weight')])):
        get = lambda k: torch.from_numpy(d[f'{name}.init.{stack}.{i}.{k}']).double()
        L = dict(weight=get('0.weight'), gamma=get('1.weight'), beta=get('1.bias'), running_mean=get('1.running_mean'),
                 running_var=get('1.running_var'))
        for k in ('weight', 'gamma', 'beta'):
            L[k].requires_grad_(requires_grad)
        layers.append(L)
    return layers, stack


GOLDEN_ENCODERS = dict(dpfn=dict(mode='max'), vfe_max=dict(mode='max'), vfe_avg=dict(mode='avg'))
