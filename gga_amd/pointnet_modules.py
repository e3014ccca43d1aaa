"""Set abstraction and feature propagation modules of PointNet++ (reference mmdet3d/ops/pointnet_modules/builder.py,
point_sa_module.py, point_fp_module.py), assembled from this project's point operators (pointnet2.py), ``cnn.ConvModule`` and
the group max pool. Constructor keys and defaults, forward signatures and ``state_dict`` names are the reference's
(``mlps.0.layer0.conv.weight``, ``mlps.0.layer0.bn.*`` for a set abstraction module, ``mlps.layer0.conv.weight`` for a
feature propagation module), so its configs build unchanged and its checkpoints load.

Memory: the grouped tensor [B, 3 + C, M, K] is turned to channels-last memory once, so every layer of the shared MLP is a
[B*M*K, C] matrix: ``dense_conv.conv2d`` decides the 1x1 products as for every other ``ConvModule``, ``functional.bn_act`` runs
its fused pass pair, and ``pointnet2.group_max_pool`` reads the last activation channels-last and leaves [B, C', M] contiguous,
which is what the next level reads as ``features``. Not built: ``F-FPS`` / ``FS`` sampling (``PointsSampler`` refuses them) and the
``PAConv`` modules.
"""
import torch
from torch import nn

from . import pointnet2 as P
from .cnn import ConvModule
from .registry import Registry

SA_MODULES = Registry('point_sa_module')


def build_sa_module(cfg, *args, **kwargs):
    """``cfg``: None (a ``PointSAModule``) or a dict with ``type`` and constructor keys; further arguments go to the
    constructor as they are."""
    if cfg is None:
        cfg = dict(type='PointSAModule')
    if not isinstance(cfg, dict):
        raise TypeError('cfg must be a dict')
    if 'type' not in cfg:
        raise KeyError('the cfg dict must contain the key "type"')
    cfg = dict(cfg)
    module_type = cfg.pop('type')
    if isinstance(module_type, str) and module_type.startswith('PAConv'):
        raise NotImplementedError(f'build_sa_module: module type {module_type!r} is not implemented (PAConv)')
    cls = SA_MODULES.get(module_type)
    if cls is None:
        raise KeyError(f'Unrecognized module type {module_type}')
    return cls(*args, **kwargs, **cfg)


def _shared_mlp(channels, norm_cfg, bias='auto'):
    mlp = nn.Sequential()
    for i in range(len(channels) - 1):
        mlp.add_module(f'layer{i}', ConvModule(channels[i], channels[i + 1], kernel_size=(1, 1), stride=(1, 1),
                                               conv_cfg=dict(type='Conv2d'), norm_cfg=norm_cfg, bias=bias))
    return mlp


@SA_MODULES.register_module()
class PointSAModuleMSG(nn.Module):
    """Set abstraction with one grouper and one shared MLP per radius; the pooled features of all radii are concatenated.
    forward(points_xyz [B,N,3], features [B,C,N] or None, indices [B,num_point] or None, target_xyz [B,M,3] or None) ->
    (new_xyz [B,M,3], new_features [B, sum of the MLPs' last widths, M], indices [B,M])."""

    def __init__(self, num_point, radii, sample_nums, mlp_channels, fps_mod=['D-FPS'], fps_sample_range_list=[-1],
                 dilated_group=False, norm_cfg=dict(type='BN2d'), use_xyz=True, pool_mod='max', normalize_xyz=False,
                 bias='auto'):
        super().__init__()
        assert len(radii) == len(sample_nums) == len(mlp_channels)
        assert pool_mod in ('max', 'avg')
        assert isinstance(fps_mod, (list, tuple)) and isinstance(fps_sample_range_list, (list, tuple))
        assert len(fps_mod) == len(fps_sample_range_list)
        if isinstance(num_point, int):
            num_point = [num_point]
        elif not (num_point is None or isinstance(num_point, (list, tuple))):
            raise NotImplementedError('Error type of num_point!')
        self.num_point = num_point
        self.mlp_channels = [list(c) for c in mlp_channels]
        self.pool_mod = pool_mod
        self.fps_mod_list, self.fps_sample_range_list = fps_mod, fps_sample_range_list
        # PointsSampler refuses F-FPS / FS (NotImplementedError)
        self.points_sampler = P.PointsSampler(num_point, fps_mod, fps_sample_range_list) if num_point is not None else None
        self.groupers, self.mlps = nn.ModuleList(), nn.ModuleList()
        for i, (radius, sample_num) in enumerate(zip(radii, sample_nums)):
            if num_point is not None:
                # a dilated group takes the ring between the previous radius and its own
                min_radius = radii[i - 1] if dilated_group and i != 0 else 0
                self.groupers.append(P.QueryAndGroup(radius, sample_num, min_radius=min_radius, use_xyz=use_xyz,
                                                     normalize_xyz=normalize_xyz))
            else:
                self.groupers.append(P.GroupAll(use_xyz))
        for channels in self.mlp_channels:
            if use_xyz:
                channels[0] += 3
            self.mlps.append(_shared_mlp(channels, norm_cfg, bias))

    def _sample_points(self, points_xyz, features, indices, target_xyz):
        """-> (new_xyz, indices): the points at ``indices`` when given, else ``target_xyz`` when given, else the sampler's."""
        if indices is None and target_xyz is not None:
            return target_xyz.contiguous(), None
        if self.num_point is None:
            return None, indices
        if indices is None:
            indices = self.points_sampler(points_xyz, features)
        else:
            assert indices.shape[1] == self.num_point[0]
        xyz_flipped = points_xyz.transpose(1, 2).contiguous()
        return P.gather_points(xyz_flipped, indices).transpose(1, 2).contiguous(), indices

    def _pool_features(self, features):
        """[B, C, M, K] -> [B, C, M] contiguous."""
        if self.pool_mod == 'max':
            return P.group_max_pool(features)
        return features.mean(dim=3).contiguous()

    def forward(self, points_xyz, features=None, indices=None, target_xyz=None):
        new_xyz, indices = self._sample_points(points_xyz, features, indices, target_xyz)
        pooled = []
        for grouper, mlp in zip(self.groupers, self.mlps):
            grouped = grouper(points_xyz, new_xyz, features)
            grouped = grouped.contiguous(memory_format=torch.channels_last)
            pooled.append(self._pool_features(mlp(grouped)))
        return new_xyz, pooled[0] if len(pooled) == 1 else torch.cat(pooled, dim=1), indices


@SA_MODULES.register_module()
class PointSAModule(PointSAModuleMSG):
    """Set abstraction with a single radius. ``num_point=None`` groups all points into one group."""

    def __init__(self, mlp_channels, num_point=None, radius=None, num_sample=None, norm_cfg=dict(type='BN2d'), use_xyz=True,
                 pool_mod='max', fps_mod=['D-FPS'], fps_sample_range_list=[-1], normalize_xyz=False):
        super().__init__(mlp_channels=[mlp_channels], num_point=num_point, radii=[radius], sample_nums=[num_sample],
                         norm_cfg=norm_cfg, use_xyz=use_xyz, pool_mod=pool_mod, fps_mod=fps_mod,
                         fps_sample_range_list=fps_sample_range_list, normalize_xyz=normalize_xyz)


class PointFPModule(nn.Module):
    """Feature propagation: the source features, interpolated to the target points from their three nearest source points
    with weights 1 / (distance + 1e-8) normalised to sum 1, are concatenated in front of the target's own features and pass a
    shared MLP. forward(target [B,n,3], source [B,m,3] or None, target_feats [B,C1,n] or None, source_feats [B,C2,m]) ->
    [B, mlp_channels[-1], n]. The [B, C, n, 1] map stays in contiguous memory: its layers run on the framework."""

    def __init__(self, mlp_channels, norm_cfg=dict(type='BN2d'), init_cfg=None):
        super().__init__()
        self.fp16_enabled = False
        self.mlps = _shared_mlp(mlp_channels, norm_cfg)

    def forward(self, target, source, target_feats, source_feats):
        if source is not None:
            dist, idx = P.three_nn(target, source)
            dist_reciprocal = 1.0 / (dist + 1e-8)
            weight = dist_reciprocal / torch.sum(dist_reciprocal, dim=2, keepdim=True)
            interpolated = P.three_interpolate(source_feats, idx, weight)
        else:
            interpolated = source_feats.expand(*source_feats.shape[:2], target.shape[1])
        new_features = interpolated if target_feats is None else torch.cat([interpolated, target_feats], dim=1)
        return self.mlps(new_features.unsqueeze(-1)).squeeze(-1)
