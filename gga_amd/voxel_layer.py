"""``Voxelization`` — same constructor / forward contract as ``mmcv.ops.Voxelization``
as the reference uses it (mmdet3d/models/detectors/mvx_two_stage_gga.py:43,225:
``Voxelization(**pts_voxel_layer)``, ``voxels, coors, num_points = layer(points)``),
plus ``forward_batch`` which voxelizes every frame of the batch in ONE call of the HIP
path instead of the reference's per-frame Python loop."""
import torch
from torch import nn

from . import functional as F


class Voxelization(nn.Module):
    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000,
                 deterministic=True):
        super().__init__()
        self.voxel_size = list(voxel_size)
        self.point_cloud_range = list(point_cloud_range)
        self.max_num_points = int(max_num_points)
        self.max_voxels = tuple(max_voxels) if isinstance(max_voxels, (tuple, list)) else (max_voxels, max_voxels)
        self.deterministic = deterministic      # the HIP path is always deterministic
        prm = F.voxel_params(self.voxel_size, self.point_cloud_range, 1, 1)
        grid = F.voxel_grid_size(prm)
        self.grid_size = torch.tensor(grid)
        self.pcd_shape = [*grid[:2], 1][::-1]
        # max_num_points = -1 or max_voxels = -1: dynamic voxelization (mmcv's rule) - every point keeps its cell
        self.dynamic = self.max_num_points == -1 or self.max_voxels[0] == -1

    def _cap(self):
        return self.max_voxels[0] if self.training else self.max_voxels[1]

    def forward(self, input):
        """points [N, C] -> voxels [M, P, C], coors [M, 3] (z, y, x), num_points [M]; dynamic mode: -> coors [N, 3] (z, y, x)
        per point, (-1, -1, -1) outside the grid (as mmcv's ``dynamic_voxelize``)."""
        if self.dynamic:
            return self.forward_batch([input])[1][:, 1:].contiguous()
        voxels, num_points, coors, _ = F.hard_voxelize_batch([input], self.voxel_size, self.point_cloud_range,
                                                             self.max_num_points, self._cap())
        return voxels, coors[:, 1:].contiguous(), num_points

    def forward_batch(self, points, sync=True):
        """list of [N_b, C] -> voxels [SM, P, C], num_points [SM], coors [SM, 4] (b, z, y, x),
        voxel_num [B+1] — what ``MVXTwoStageDetector_GGA.voxelize`` assembles. Dynamic mode: -> (points [SN, C] concatenated,
        coors [SN, 4] (b, z, y, x) per point), the sorted point-to-voxel map riding on the coordinates as ``coors.voxel_map``
        (``dynamic_voxel.VoxelMap``); nothing is read back."""
        if self.dynamic:
            import numpy as np
            from . import dynamic_voxel as DV
            offs = np.zeros(len(points) + 1, np.int64)
            offs[1:] = np.cumsum([p.shape[0] for p in points])
            cat = points[0] if len(points) == 1 else torch.cat(points, 0)
            cat = cat.contiguous() if cat.dtype == torch.float32 else cat.float().contiguous()
            return cat, DV.dynamic_voxelize(cat, offs, None, self.voxel_size, self.point_cloud_range)
        return F.hard_voxelize_batch(points, self.voxel_size, self.point_cloud_range, self.max_num_points,
                                     self._cap(), sync=sync)

    def forward_prepared(self, prep, sync=True):
        """``forward_batch`` for the output of ``functional.points_prepare_batch`` (device-resident
        frames with device-side point counts). Dynamic mode: as ``forward_batch``, over the capacity-sized point buffer;
        the rows past a frame's count are dropped points."""
        if self.dynamic:
            from . import dynamic_voxel as DV
            pts = prep.points[:int(prep.capacity_offsets[-1])]
            return pts, DV.dynamic_voxelize(pts, prep.capacity_offsets, prep.counts, self.voxel_size, self.point_cloud_range)
        return F.hard_voxelize_prepared(prep, self.voxel_size, self.point_cloud_range, self.max_num_points,
                                        self._cap(), sync=sync)

    def __repr__(self):
        return (f'{self.__class__.__name__}(voxel_size={self.voxel_size}, point_cloud_range='
                f'{self.point_cloud_range}, max_num_points={self.max_num_points}, max_voxels={self.max_voxels}, '
                f'deterministic={self.deterministic})')
