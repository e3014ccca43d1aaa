"""``LiDARPoints`` / ``DepthPoints`` — the slice of the reference's point structure the GGA train pipeline touches
(mmdet3d/core/points/base_points.py:11-440, lidar_points.py): ``tensor [N, points_dim]``,
``coord``, ``in_range_3d`` (strict inequalities, :203-225), ``shuffle`` (``torch.randperm``,
:135-143), ``cat`` (:356-377), indexing, ``new_point``; for the indoor pipelines ``color`` (:96-128), ``rotate`` by a matrix (:151-190),
``translate`` (:192-216)."""
import warnings

import numpy as np
import torch


class BasePoints:
    def __init__(self, tensor, points_dim=3, attribute_dims=None):
        device = tensor.device if isinstance(tensor, torch.Tensor) else torch.device('cpu')
        tensor = torch.as_tensor(tensor, dtype=torch.float32, device=device)
        if tensor.numel() == 0:
            tensor = tensor.reshape((0, points_dim)).to(dtype=torch.float32, device=device)
        assert tensor.dim() == 2 and tensor.size(-1) == points_dim, tensor.size()
        self.tensor = tensor
        self.points_dim = points_dim
        self.attribute_dims = attribute_dims
        self.rotation_axis = 0

    @property
    def coord(self):
        return self.tensor[:, :3]

    @property
    def color(self):
        """[N, 3] colour columns named by ``attribute_dims['color']``, or None when the points carry none."""
        if self.attribute_dims is not None and 'color' in self.attribute_dims:
            return self.tensor[:, self.attribute_dims['color']]
        return None

    @color.setter
    def color(self, tensor):
        try:
            tensor = tensor.reshape(self.shape[0], 3)
        except (RuntimeError, ValueError):
            raise ValueError(f'got unexpected shape {tensor.shape}')
        if tensor.max() >= 256 or tensor.min() < 0:
            warnings.warn('point got color value beyond [0, 255]')
        if not isinstance(tensor, torch.Tensor):
            tensor = self.tensor.new_tensor(tensor)
        if self.attribute_dims is not None and 'color' in self.attribute_dims:
            self.tensor[:, self.attribute_dims['color']] = tensor
        else:                                   # points without colour gain three columns
            if self.attribute_dims is None:
                self.attribute_dims = dict()
            first = self.shape[1]
            self.tensor = torch.cat([self.tensor, tensor], dim=1)
            self.attribute_dims.update(dict(color=[first, first + 1, first + 2]))
            self.points_dim += 3

    @property
    def shape(self):
        return self.tensor.shape

    def rotate(self, rot_mat_t):
        """Row vectors times the 3 x 3 matrix ``rot_mat_t`` (the transposed rotation), in place. -> the matrix as a tensor."""
        rot_mat_t = self.tensor.new_tensor(rot_mat_t) if not isinstance(rot_mat_t, torch.Tensor) else rot_mat_t
        assert rot_mat_t.shape == torch.Size([3, 3]), f'invalid rotation shape {rot_mat_t.shape}'
        self.tensor[:, :3] = self.tensor[:, :3] @ rot_mat_t
        return rot_mat_t

    def translate(self, trans_vector):
        """[3] (or [1, 3] / [N, 3]) added to the coordinates, in place."""
        if not isinstance(trans_vector, torch.Tensor):
            trans_vector = self.tensor.new_tensor(trans_vector)
        trans_vector = trans_vector.squeeze(0)
        assert trans_vector.dim() == 1 and trans_vector.numel() == 3 or trans_vector.shape == (len(self), 3), \
            f'Unsupported translation vector of shape {trans_vector.shape}'
        self.tensor[:, :3] += trans_vector

    @property
    def bev(self):
        return self.tensor[:, [0, 1]]

    @property
    def device(self):
        return self.tensor.device

    def shuffle(self):
        idx = torch.randperm(len(self), device=self.tensor.device)
        self.tensor = self.tensor[idx]
        return idx

    def in_range_3d(self, point_range):
        t = self.tensor
        return ((t[:, 0] > point_range[0]) & (t[:, 1] > point_range[1]) & (t[:, 2] > point_range[2])
                & (t[:, 0] < point_range[3]) & (t[:, 1] < point_range[4]) & (t[:, 2] < point_range[5]))

    def __getitem__(self, item):
        # base_points.py:276-346 — int / slice / mask / index array on the first axis, optional column
        # selection on the second
        cls = type(self)
        if isinstance(item, int):
            return cls(self.tensor[item].view(1, -1), points_dim=self.points_dim, attribute_dims=self.attribute_dims)
        if isinstance(item, np.ndarray):
            item = torch.from_numpy(item)
        t = self.tensor[item]
        assert t.dim() == 2, f'Indexing on Points with {item} failed to return a matrix!'
        return cls(t, points_dim=t.shape[1], attribute_dims=self.attribute_dims if t.shape[1] == self.points_dim else None)

    def __len__(self):
        return self.tensor.shape[0]

    def __repr__(self):
        return self.__class__.__name__ + '(\n    ' + str(self.tensor) + ')'

    @classmethod
    def cat(cls, points_list):
        assert isinstance(points_list, (list, tuple))
        if len(points_list) == 0:
            return cls(torch.empty(0))
        assert all(isinstance(p, cls) for p in points_list)
        return cls(torch.cat([p.tensor for p in points_list], dim=0), points_dim=points_list[0].tensor.shape[1],
                   attribute_dims=points_list[0].attribute_dims)

    def to(self, device):
        return type(self)(self.tensor.to(device), points_dim=self.points_dim, attribute_dims=self.attribute_dims)

    def clone(self):
        return type(self)(self.tensor.clone(), points_dim=self.points_dim, attribute_dims=self.attribute_dims)

    def new_point(self, data):
        t = self.tensor.new_tensor(data) if not isinstance(data, torch.Tensor) else data.to(self.device)
        return type(self)(t, points_dim=self.points_dim, attribute_dims=self.attribute_dims)


class LiDARPoints(BasePoints):
    FLIP_AXIS = dict(horizontal=1, vertical=0)         # lidar_points.py: a horizontal flip negates y, a vertical one x

    def __init__(self, tensor, points_dim=3, attribute_dims=None):
        super().__init__(tensor, points_dim=points_dim, attribute_dims=attribute_dims)
        self.rotation_axis = 2


class DepthPoints(BasePoints):
    """depth_points.py: points in depth coordinates (indoor scenes); rotation about z like the LiDAR points."""
    FLIP_AXIS = dict(horizontal=0, vertical=1)         # depth_points.py: a horizontal flip negates x, a vertical one y

    def __init__(self, tensor, points_dim=3, attribute_dims=None):
        super().__init__(tensor, points_dim=points_dim, attribute_dims=attribute_dims)
        self.rotation_axis = 2
