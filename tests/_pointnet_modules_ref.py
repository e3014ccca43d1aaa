"""Restatements for the tests of gga_amd/pointnet_modules.py and the group max pool (gga_amd/csrc/pointnet2.hip "group max
pool"): the pool as a plain scan in numpy, and the PointNet2SASSG backbone in plain torch on the CPU at a chosen precision
(1x1 products as einsum, training-mode batch statistics, ReLU, the pool by the first-maximum rule, grouping and interpolation by
indexing, plain autograd). The backbone restatement takes the sampling, ball-query and three-NN index tensors as inputs: they
depend on the coordinates alone, the device run's are pinned bit for bit by tests/test_pointnet2_gpu.py, and the numpy
definitions of tests/_pointnet2_ref.py give the same ones without a device."""
import numpy as np
import torch

import _pointnet2_ref as R2

# the small backbone of the float64 comparison, and the backbone dict of the reference's configs/_base_/models/votenet.py
SMALL = dict(type='PointNet2SASSG', in_channels=4, num_points=(32, 16, 8, 4), radius=(0.4, 0.8, 1.6, 2.4),
             num_samples=(8, 4, 4, 4), sa_channels=((8, 8, 16), (16, 16, 32), (16, 16, 32), (16, 16, 32)),
             fp_channels=((32, 32), (32, 32)), norm_cfg=dict(type='BN2d'),
             sa_cfg=dict(type='PointSAModule', pool_mod='max', use_xyz=True, normalize_xyz=True))
VOTENET = dict(type='PointNet2SASSG', in_channels=4, num_points=(2048, 1024, 512, 256), radius=(0.2, 0.4, 0.8, 1.2),
               num_samples=(64, 32, 16, 16), sa_channels=((64, 64, 128), (128, 128, 256), (128, 128, 256), (128, 128, 256)),
               fp_channels=((256, 256), (256, 256)), norm_cfg=dict(type='BN2d'),
               sa_cfg=dict(type='PointSAModule', pool_mod='max', use_xyz=True, normalize_xyz=True))
# Chosen on the CPU by this file alone: of the seeds 0 .. 599 that meet the first two conditions of
# tests/test_pointnet_modules_abi.py::test_small_case_is_well_conditioned (48 of them), the one whose plain float32 restatement
# lies closest to the float64 one. Batch statistics over as few as 16 values per channel, sixteen layers deep, amplify rounding:
# over those seeds the float32 restatement lies 1.8e-5 .. 5.6e-4 (relative, worst tensor) from float64, so at many seeds float32
# arithmetic itself misses the 1e-4 of the device comparison.
SEED = 219
B, N = 2, 100
BN_EPS = 1e-5


def group_max(x):
    """x [..., K] float32 -> (y [...] float32, arg [...] uint8): scan k = 0 .. K-1 from best = x[0], arg = 0; x[k] is taken
    when x[k] > best, or when x[k] is NaN and best is not."""
    x = np.asarray(x, np.float32)
    best, arg = x[..., 0].copy(), np.zeros(x.shape[:-1], np.uint8)
    for k in range(1, x.shape[-1]):
        v = x[..., k]
        with np.errstate(invalid='ignore'):
            take = (v > best) | (np.isnan(v) & ~np.isnan(best))
        best = np.where(take, v, best)
        arg = np.where(take, np.uint8(k), arg)
    return best, arg


def group_max_grad(gy, arg, K):
    """gx [..., K]: gy at k == arg, +0 elsewhere."""
    gx = np.zeros(gy.shape + (K,), np.float32)
    np.put_along_axis(gx, arg[..., None].astype(np.int64), np.asarray(gy, np.float32)[..., None], axis=-1)
    return gx


# ----------------------------------------------------------------------------- the backbone
def small_case(seed=SEED):
    """-> (model on the CPU in training mode, points [B, N, 4] float32): the small backbone with Kaiming weights from `seed`, the
    BatchNorm scales and shifts drawn away from (1, 0) so that their gradients are not special, points uniform in the unit
    cube with one normal feature channel."""
    from gga_amd.registry import build_backbone
    torch.manual_seed(seed)
    model = build_backbone(SMALL)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.2)
    rng = np.random.default_rng(seed)
    points = np.concatenate([rng.uniform(0, 1, (B, N, 3)), rng.normal(0, 1, (B, N, 1))], axis=2).astype(np.float32)
    return model.train(), torch.from_numpy(points)


def functional_weights(shape, seed=SEED):
    """The fixed random linear functional of fp_features[-1]: loss = sum(weights * fp_features[-1])."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed + 1000), dtype=torch.float64)


def indices_numpy(xyz, cfg=SMALL):
    """The index tensors of a forward pass by the numpy definitions: dict(fps=[level -> int64 [B,M]], ball=[level -> int64
    [B,M,K]], nn=[propagation -> int64 [B,n,3]])."""
    xyz = np.asarray(xyz, np.float32)
    levels, fps, ball = [xyz], [], []
    for M, radius, K in zip(cfg['num_points'], cfg['radius'], cfg['num_samples']):
        s = R2.furthest_point_sample(levels[-1], M)
        centre = np.stack([levels[-1][b][s[b]] for b in range(xyz.shape[0])])
        fps.append(torch.from_numpy(s.astype(np.int64)))
        ball.append(torch.from_numpy(R2.ball_query(0, radius, K, levels[-1], centre).astype(np.int64)))
        levels.append(centre)
    num_sa = len(cfg['num_points'])
    nn = [torch.from_numpy(R2.three_nn(levels[num_sa - i - 1], levels[num_sa - i])[1].astype(np.int64))
          for i in range(len(cfg['fp_channels']))]
    return dict(fps=fps, ball=ball, nn=nn)


def _take(t, idx):
    """t [B, C, N], idx [B, ...] -> [B, C, ...]: t[b, :, idx[b]]."""
    Bn, C = t.shape[:2]
    flat = idx.reshape(Bn, 1, -1).expand(Bn, C, -1)
    return torch.gather(t, 2, flat).reshape((Bn, C) + tuple(idx.shape[1:]))


def _layer(x, prefix, params, record):
    """conv 1x1 (no bias) -> BatchNorm with the batch's statistics -> ReLU on x [B, C, H, W]."""
    z = torch.einsum('oc,bchw->bohw', params[prefix + '.conv.weight'][:, :, 0, 0], x)
    mean = z.mean(dim=(0, 2, 3), keepdim=True)
    var = ((z - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    pre = (z - mean) / torch.sqrt(var + BN_EPS) * params[prefix + '.bn.weight'].view(1, -1, 1, 1) \
        + params[prefix + '.bn.bias'].view(1, -1, 1, 1)
    record['pre'].append(pre)
    return torch.relu(pre)


def first_max_pool(x):
    """x [B, C, M, K] -> (max over K at the first position that holds it [B, C, M], that position)."""
    K = x.shape[3]
    top = x.max(dim=3, keepdim=True).values
    pos = torch.where(x == top, torch.arange(K).view(1, 1, 1, K), torch.tensor(K)).min(dim=3).values
    return torch.gather(x, 3, pos.unsqueeze(-1)).squeeze(-1), pos


def backbone(params, points, index, cfg=SMALL):
    """The forward pass of PointNet2SASSG(**cfg) in training mode at the precision of `points`. params: name -> tensor of that
    precision (the module's state_dict names); points [B, N, 4] (the feature channel may require grad through
    ``features``); index: as indices_numpy. -> dict(sa_features, fp_features, pre = every pre-activation in order, pooled /
    pool_pos = every level's pooled tensor and pool positions)."""
    record = dict(pre=[], pooled=[], pool_pos=[])
    xyz, features = points[..., :3], points[..., 3:].transpose(1, 2)
    sa_xyz, sa_features = [xyz], [features]
    for lvl, (radius, layers) in enumerate(zip(cfg['radius'], cfg['sa_channels'])):
        p, f = sa_xyz[-1], sa_features[-1]
        centre = _take(p.transpose(1, 2), index['fps'][lvl]).transpose(1, 2)
        diff = (_take(p.transpose(1, 2), index['ball'][lvl]) - centre.transpose(1, 2).unsqueeze(-1)) / radius
        x = torch.cat([diff, _take(f, index['ball'][lvl])], dim=1)
        for i in range(len(layers)):
            x = _layer(x, f'SA_modules.{lvl}.mlps.0.layer{i}', params, record)
        pooled, pos = first_max_pool(x)
        record['pooled'].append(pooled)
        record['pool_pos'].append(pos)
        sa_xyz.append(centre)
        sa_features.append(pooled)
    num_sa = len(cfg['sa_channels'])
    fp_features = [sa_features[-1]]
    for i, layers in enumerate(cfg['fp_channels']):
        target, source = sa_xyz[num_sa - i - 1], sa_xyz[num_sa - i]
        idx = index['nn'][i]
        near = _take(source.transpose(1, 2), idx)                                    # [B, 3, n, 3 neighbours]
        dist = torch.sqrt(((target.transpose(1, 2).unsqueeze(-1) - near) ** 2).sum(dim=1))
        w = 1.0 / (dist + 1e-8)
        w = w / w.sum(dim=2, keepdim=True)
        x = (_take(fp_features[-1], idx) * w.unsqueeze(1)).sum(dim=3)
        x = torch.cat([x, sa_features[num_sa - i - 1]], dim=1).unsqueeze(-1)
        for j in range(len(layers)):
            x = _layer(x, f'FP_modules.{i}.mlps.layer{j}', params, record)
        fp_features.append(x.squeeze(-1))
    return dict(sa_features=sa_features, fp_features=fp_features, **record)


def run(model, points, index, dtype, cfg=SMALL):
    """Forward and backward of the restatement at `dtype` with `model`'s weights -> (outputs of backbone(), gradients: name ->
    tensor for every parameter and 'points.features' [B, N, 1])."""
    params = {k: v.detach().to(dtype).requires_grad_(True) for k, v in model.state_dict().items() if v.is_floating_point()}
    pts = points.detach().to(dtype)
    feats = pts[..., 3:].clone().requires_grad_(True)
    out = backbone(params, torch.cat([pts[..., :3], feats], dim=2), index, cfg)
    last = out['fp_features'][-1]
    (last * functional_weights(last.shape).to(dtype)).sum().backward()
    named = dict(model.named_parameters())
    grads = {k: params[k].grad for k in named}
    grads['points.features'] = feats.grad
    return out, grads
