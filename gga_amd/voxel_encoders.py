"""Voxel encoders of the GGA configs: ``HardSimpleVFE`` (SECOND trunk,
mmdet3d/models/voxel_encoders/voxel_encoder.py:13-45) and ``PillarFeatureNet`` +
``PFNLayer`` (PointPillars trunk, voxel_encoders/pillar_encoder.py:12-159,
voxel_encoders/utils.py:107-182). Same constructor arguments, parameter names and
``forward(features, num_points, coors)`` signature. The dynamic encoders (``DynamicSimpleVFE``, ``DynamicVFE``:
voxel_encoder.py:48-286; ``DynamicPillarFeatureNet``: pillar_encoder.py:162-323) take ``forward(features, coors)`` with one
row per POINT and return ``(voxel_feats, voxel_coors)``; their reductions run on ``ops.DynamicScatter``."""
import os

import torch
from torch import nn
from torch.nn import functional as TF

from . import functional as F
from .cnn import build_norm_layer
from .ops import DynamicScatter
from .registry import VOXEL_ENCODERS


@VOXEL_ENCODERS.register_module()
class HardSimpleVFE(nn.Module):
    def __init__(self, num_features=4):
        super().__init__()
        self.num_features = num_features
        self.fp16_enabled = False

    def forward(self, features, num_points, coors):
        return F.voxel_mean(features, num_points, self.num_features)


def get_paddings_indicator(actual_num, max_num, axis=0):
    actual_num = torch.unsqueeze(actual_num, axis + 1)
    shape = [1] * len(actual_num.shape)
    shape[axis + 1] = -1
    max_num = torch.arange(max_num, dtype=torch.int, device=actual_num.device).view(shape)
    return actual_num.int() > max_num


class PFNLayer(nn.Module):
    def __init__(self, in_channels, out_channels, norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01),
                 last_layer=False, mode='max'):
        super().__init__()
        self.fp16_enabled = False
        self.name = 'PFNLayer'
        self.last_vfe = last_layer
        if not self.last_vfe:
            out_channels = out_channels // 2
        self.units = out_channels
        self.norm = build_norm_layer(norm_cfg, self.units)[1]
        self.linear = nn.Linear(in_channels, self.units, bias=False)
        assert mode in ['max', 'avg']
        self.mode = mode

    def forward(self, inputs, num_voxels=None, aligned_distance=None):
        x = self.linear(inputs)
        x = self.norm(x.permute(0, 2, 1).contiguous()).permute(0, 2, 1).contiguous()
        x = TF.relu(x)
        if aligned_distance is not None:
            x = x.mul(aligned_distance.unsqueeze(-1))
        if self.mode == 'max':
            x_max = torch.max(x, dim=1, keepdim=True)[0]
        else:
            x_max = x.sum(dim=1, keepdim=True) / num_voxels.type_as(inputs).view(-1, 1, 1)
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max.repeat(1, inputs.shape[1], 1)], dim=2)


@VOXEL_ENCODERS.register_module()
class PillarFeatureNet(nn.Module):
    def __init__(self, in_channels=4, feat_channels=(64, ), with_distance=False, with_cluster_center=True,
                 with_voxel_center=True, voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1),
                 norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), mode='max', legacy=True):
        super().__init__()
        assert len(feat_channels) > 0
        self.legacy = legacy
        if with_cluster_center:
            in_channels += 3
        if with_voxel_center:
            in_channels += 3
        if with_distance:
            in_channels += 1
        self._with_distance = with_distance
        self._with_cluster_center = with_cluster_center
        self._with_voxel_center = with_voxel_center
        self.fp16_enabled = False
        self.in_channels = in_channels
        feat_channels = [in_channels] + list(feat_channels)
        self.pfn_layers = nn.ModuleList([
            PFNLayer(feat_channels[i], feat_channels[i + 1], norm_cfg=norm_cfg,
                     last_layer=(i >= len(feat_channels) - 2), mode=mode)
            for i in range(len(feat_channels) - 1)])
        self.vx, self.vy, self.vz = voxel_size[0], voxel_size[1], voxel_size[2]
        self.x_offset = self.vx / 2 + point_cloud_range[0]
        self.y_offset = self.vy / 2 + point_cloud_range[1]
        self.z_offset = self.vz / 2 + point_cloud_range[2]
        self.point_cloud_range = point_cloud_range

    def _fusable(self, features):
        l0 = self.pfn_layers[0]
        return (features.is_cuda and len(self.pfn_layers) == 1 and l0.units == 64 and l0.mode == 'max'
                and self.legacy and self._with_cluster_center and self._with_voxel_center
                and not self._with_distance and features.shape[-1] == 4 and features.shape[1] <= 254
                and features.shape[0] > 0 and isinstance(l0.norm, nn.BatchNorm1d) and l0.norm.affine
                and l0.norm.track_running_stats and l0.norm.momentum is not None and features.dtype == torch.float32)

    accepts_num_valid = True        # capacity-sized inputs with a device-side count (detectors.voxelize)

    def forward(self, features, num_points, coors):
        if self._fusable(features):
            # one fused HIP pass (gga_amd/csrc/pfn.hip) instead of the [M,P,64] eager pipeline
            l0 = self.pfn_layers[0]
            bn = l0.norm
            prm = F.pfn_params((self.vx, self.vy, self.vz), (self.x_offset, self.y_offset, self.z_offset),
                               bn.eps, bn.momentum, self.training)
            if self.training:
                F.count_batch(bn)
            return F.fused_pfn(features, num_points.int(), coors.int(), l0.linear.weight, bn.weight, bn.bias,
                               bn.running_mean, bn.running_var, prm, num_valid=F.num_valid_of(coors))
        if F.num_valid_of(coors) is not None:     # capacity-sized buffers: the eager ops need the exact rows
            m = int(F.num_valid_of(coors).item())
            features, num_points, coors = features[:m], num_points[:m], coors[:m]
        return self.forward_eager(features, num_points, coors)

    def forward_eager(self, features, num_points, coors):
        """The reference's op sequence in eager PyTorch (general configurations)."""
        features_ls = [features]
        if self._with_cluster_center:
            points_mean = features[:, :, :3].sum(dim=1, keepdim=True) / num_points.type_as(features).view(-1, 1, 1)
            features_ls.append(features[:, :, :3] - points_mean)
        if self._with_voxel_center:
            centre = torch.stack([coors[:, 3].type_as(features) * self.vx + self.x_offset,
                                  coors[:, 2].type_as(features) * self.vy + self.y_offset,
                                  coors[:, 1].type_as(features) * self.vz + self.z_offset], 1).unsqueeze(1)
            f_center = features[:, :, :3] - centre
            if self.legacy:
                # legacy=True subtracts in place through a view (pillar_encoder.py:129-139): the
                # first three input channels ARE the centre offsets afterwards.
                features_ls[0] = torch.cat([f_center, features[:, :, 3:]], dim=-1)
            features_ls.append(f_center)
        if self._with_distance:
            features_ls.append(torch.norm(features[:, :, :3], 2, 2, keepdim=True))
        features = torch.cat(features_ls, dim=-1)
        mask = get_paddings_indicator(num_points, features.shape[1], axis=0)
        features = features * torch.unsqueeze(mask, -1).type_as(features)
        for pfn in self.pfn_layers:
            features = pfn(features, num_points)
        return features.squeeze(1)


# ---- dynamic voxelization ---------------------------------------------------------------------------------------------
# GGA_DYNAMIC_PFN_FUSED=0: DynamicPillarFeatureNet on its eager path (Linear / BatchNorm of the framework between the scatter
# kernels) instead of the fused kernels - a debugging switch
DYNAMIC_PFN_FUSED = os.environ.get('GGA_DYNAMIC_PFN_FUSED', '1') == '1'


def _kept_points(features, coors, grid):
    """Points that lie in the grid, with the map of their voxels. Where the reference lets a point at (b,-1,-1,-1) through
    the linear layer and BatchNorm (and reads its cluster centre at a wrapped canvas index), a dropped point takes part in
    nothing here, BatchNorm statistics included: such rows are filtered out up front. The pipelines'
    PointsRangeFilter leaves none, and then this is the identity."""
    from . import dynamic_voxel as DV
    vmap = DV.map_of(coors, grid)
    if vmap.host_counts()[1] == vmap.n:
        return features, coors, vmap
    keep = (vmap.point2voxel >= 0).nonzero().squeeze(1)
    features, coors = features.index_select(0, keep), coors.index_select(0, keep)
    return features, coors, DV.map_of(coors, grid, batch=vmap.batch)


class _DynamicEncoderBase(nn.Module):
    """What DynamicVFE and DynamicPillarFeatureNet share: the decorations of a point and the layer stack
    Linear - BatchNorm - ReLU -> scatter -> [point feats, its voxel's feats] -> next layer."""

    def _setup(self, in_channels, feat_channels, with_distance, with_cluster_center, with_voxel_center, voxel_size,
               point_cloud_range, norm_cfg, mode):
        assert mode in ['avg', 'max']
        assert len(feat_channels) > 0
        in_channels += 3 * bool(with_cluster_center) + 3 * bool(with_voxel_center) + bool(with_distance)
        self.in_channels = in_channels
        self._with_distance = with_distance
        self._with_cluster_center = with_cluster_center
        self._with_voxel_center = with_voxel_center
        self.fp16_enabled = False
        self.vx, self.vy, self.vz = voxel_size[0], voxel_size[1], voxel_size[2]
        self.x_offset = self.vx / 2 + point_cloud_range[0]
        self.y_offset = self.vy / 2 + point_cloud_range[1]
        self.z_offset = self.vz / 2 + point_cloud_range[2]
        self.point_cloud_range = point_cloud_range
        self.mode = mode
        chans = [in_channels] + list(feat_channels)
        layers = []
        for i in range(len(chans) - 1):
            cin = chans[i] * (2 if i > 0 else 1)
            layers.append(nn.Sequential(nn.Linear(cin, chans[i + 1], bias=False), build_norm_layer(norm_cfg, chans[i + 1])[1],
                                        nn.ReLU(inplace=True)))
        self._grid = None
        return layers, DynamicScatter(voxel_size, point_cloud_range, mode != 'max'), \
            DynamicScatter(voxel_size, point_cloud_range, average_points=True)

    def _grid_size(self):
        if self._grid is None:
            from . import dynamic_voxel as DV
            self._grid = DV.grid_of((self.vx, self.vy, self.vz), self.point_cloud_range)
        return self._grid

    def map_voxel_center_to_point(self, pts_coors, voxel_mean, voxel_coors=None):
        """Per point, the row of ``voxel_mean`` of its voxel: ``voxel_mean[point2voxel]`` - no canvas is built."""
        from . import dynamic_voxel as DV
        vmap = DV.map_of(pts_coors, self._grid_size())
        return voxel_mean.index_select(0, vmap.point2voxel.clamp(min=0).long())

    def _decorate(self, features, coors, vmap):
        from . import dynamic_voxel as DV
        cols = [features]
        if self._with_cluster_center:
            mean = DV.scatter(features[:, :3], vmap, DV.MEAN)
            cols.append(features[:, :3] - mean.index_select(0, vmap.point2voxel.long()))
        if self._with_voxel_center:
            # the centre is rounded as a product and a sum of its own (no fused multiply-add), as the eager ops round it
            c = coors.to(features.dtype)
            centre = torch.stack([c[:, 3] * self.vx + self.x_offset, c[:, 2] * self.vy + self.y_offset,
                                  c[:, 1] * self.vz + self.z_offset], 1)
            cols.append(features[:, :3] - centre)
        if self._with_distance:
            cols.append(torch.norm(features[:, :3], 2, 1, keepdim=True))
        return torch.cat(cols, dim=-1)

    def _stack(self, layers, features, coors, return_point_feats=False):
        from . import dynamic_voxel as DV
        if coors.shape[1] != 4:
            raise ValueError(f'coors must be [N, 4] (b, z, y, x), got {tuple(coors.shape)}')
        features, coors, vmap = _kept_points(features, coors, self._grid_size())
        features = self._decorate(features, coors, vmap)
        mode = DV.MAX if self.mode == 'max' else DV.MEAN
        p2v = vmap.point2voxel.long()
        for i, layer in enumerate(layers):
            point_feats = layer(features)
            voxel_feats = DV.scatter(point_feats, vmap, mode)
            if i != len(layers) - 1:
                features = torch.cat([point_feats, voxel_feats.index_select(0, p2v)], dim=1)
        if return_point_feats:
            return point_feats
        return voxel_feats, vmap.voxel_coors[:vmap.m]


@VOXEL_ENCODERS.register_module()
class DynamicSimpleVFE(nn.Module):
    def __init__(self, voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1)):
        super().__init__()
        self.scatter = DynamicScatter(voxel_size, point_cloud_range, True)
        self.fp16_enabled = False

    @torch.no_grad()
    def forward(self, features, coors):
        """features [N, C] points, coors [N, 4] -> (mean of the points of every voxel [M, C], voxel coors [M, 4])."""
        return self.scatter(features, coors)


@VOXEL_ENCODERS.register_module()
class DynamicVFE(_DynamicEncoderBase):
    def __init__(self, in_channels=4, feat_channels=[], with_distance=False, with_cluster_center=False,
                 with_voxel_center=False, voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1),
                 norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), mode='max', fusion_layer=None,
                 return_point_feats=False):
        super().__init__()
        if fusion_layer is not None:
            raise NotImplementedError('fusion_layer: the GGA configs are LiDAR-only; the image branch is out of scope')
        layers, vfe_scatter, cluster_scatter = self._setup(in_channels, feat_channels, with_distance, with_cluster_center,
                                                           with_voxel_center, voxel_size, point_cloud_range, norm_cfg, mode)
        self.return_point_feats = return_point_feats
        self.scatter = DynamicScatter(voxel_size, point_cloud_range, True)
        self.vfe_layers = nn.ModuleList(layers)
        self.num_vfe = len(layers)
        self.vfe_scatter = vfe_scatter
        self.cluster_scatter = cluster_scatter
        self.fusion_layer = None

    def forward(self, features, coors, points=None, img_feats=None, img_metas=None):
        return self._stack(self.vfe_layers, features, coors, self.return_point_feats)


@VOXEL_ENCODERS.register_module()
class DynamicPillarFeatureNet(_DynamicEncoderBase):
    def __init__(self, in_channels=4, feat_channels=(64, ), with_distance=False, with_cluster_center=True,
                 with_voxel_center=True, voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1),
                 norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), mode='max', legacy=True):
        super().__init__()
        self.legacy = legacy        # (a constructor key of the base class; the dynamic forward has no in-place quirk)
        layers, pfn_scatter, cluster_scatter = self._setup(in_channels, feat_channels, with_distance, with_cluster_center,
                                                           with_voxel_center, voxel_size, point_cloud_range, norm_cfg, mode)
        self.num_pfn = len(layers)
        self.pfn_layers = nn.ModuleList(layers)
        self.pfn_scatter = pfn_scatter
        self.cluster_scatter = cluster_scatter

    accepts_num_valid = True        # forward(capacity=True): capacity-sized rows with a device-side count, no read-back

    def fusable_config(self):
        """The shipped form, which the fused kernels (gga_amd/csrc/dynamic_voxel.hip) cover."""
        if not DYNAMIC_PFN_FUSED or len(self.pfn_layers) != 1:
            return False
        lin, bn = self.pfn_layers[0][0], self.pfn_layers[0][1]
        return (lin.out_features == 64 and lin.in_features == 10 and self.mode == 'max' and self._with_cluster_center
                and self._with_voxel_center and not self._with_distance and isinstance(bn, nn.BatchNorm1d) and bn.affine
                and bn.track_running_stats and bn.momentum is not None)

    def _fusable(self, features, coors):
        return (self.fusable_config() and features.is_cuda and features.dim() == 2 and features.shape[1] == 4
                and features.shape[0] > 0 and features.dtype == torch.float32 and coors.dim() == 2 and coors.shape[1] == 4
                and self.pfn_layers[0][0].weight.dtype == torch.float32)

    def forward(self, features, coors, capacity=False):
        """features [N, 4+] points, coors [N, 4] -> (voxel_feats [M, C], voxel_coors [M, 4]). ``capacity=True`` (the fused form
        only): both keep N rows, the rows past the voxel count are zero and ``voxel_coors.num_valid`` carries the count on the
        device - what ``PointPillarsScatter`` consumes without a host read."""
        if not self._fusable(features, coors):
            return self.forward_eager(features, coors)
        from . import dynamic_voxel as DV
        lin, bn = self.pfn_layers[0][0], self.pfn_layers[0][1]
        coors = coors if coors.dtype == torch.int32 else coors.int()
        vmap = DV.map_of(coors, self._grid_size())
        prm = F.pfn_params((self.vx, self.vy, self.vz), (self.x_offset, self.y_offset, self.z_offset), bn.eps, bn.momentum,
                           bn.training)
        if bn.training:
            F.count_batch(bn)
        rows = vmap.n if capacity else vmap.m
        voxel_coors = vmap.voxel_coors[:rows]
        if rows == 0:
            return features.new_zeros((0, 64)), voxel_coors
        out = DV.fused_pfn(features.contiguous(), coors.contiguous(), vmap, lin.weight, bn.weight, bn.bias, bn.running_mean,
                           bn.running_var, prm, rows=rows)
        if capacity:
            voxel_coors.num_valid = vmap.num_valid
        return out, voxel_coors

    def forward_eager(self, features, coors):
        """The reference's op sequence (general configurations): the framework's Linear / BatchNorm / ReLU between the
        ``DynamicScatter`` kernels."""
        return self._stack(self.pfn_layers, features, coors)
