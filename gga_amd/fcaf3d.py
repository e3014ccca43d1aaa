"""FCAF3D (BASELINE config 4): ``MinkResNet`` backbone, ``FCAF3DHead`` (sparse FPN with generative transposed convolutions
and pruning + anchor-free head) and ``MinkSingleStage3DDetector`` - registry names, constructor keys, parameter names and
loss-dict keys of the reference (mmdet3d/models/backbones/mink_resnet.py:18-114, mmdet3d/models/dense_heads/
fcaf3d_head.py:49-678, mmdet3d/models/detectors/mink_single_stage.py:16-109; configs/_base_/models/fcaf3d.py,
configs/fcaf3d/fcaf3d_8x2_sunrgbd-3d-10class.py), on the MinkowskiEngine-semantics layers of ``gga_amd.mink``.

There is no GGA head for this trunk in the reference tree: what is built - and what can be checked - is
stock FCAF3D. Third-party pieces restated from their published code, parity unpinned: MinkowskiEngine (``mink.py``), mmcv's
``diff_iou_rotated_3d`` (``rotated_iou_3d`` below), ``nms3d`` / ``nms3d_normal`` (BEV overlap of the upright boxes, on
``postproc.hip``'s rotated-NMS kernel), ``Scale``, ``bias_init_with_prob``; mmdet's ``FocalLoss`` /
``CrossEntropyLoss`` are those of ``losses.py``. The head's own target assignment, loss and box decoding are plain torch in the
reference and are pinned by golden vectors from a run of the reference's class (tests/golden/fcaf3d_head.npz)."""
import math

import torch
from torch import nn

from . import mink as ME
from . import ops
from .losses import weight_reduce_loss
from .registry import BACKBONES, DETECTORS, HEADS, LOSSES, build_backbone, build_head, build_loss


# ----------------------------------------------------------------------------------------------------------------- boxes
def rotation_3d_in_axis_z(points, angles):
    """``rotation_3d_in_axis(points [N, M, 3], angles [N], axis=2)`` (core/bbox/structures/utils.py:79-117): points @ R with
    R = [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]] per entry - the counter-clockwise rotation of the row vectors."""
    c, s = torch.cos(angles), torch.sin(angles)
    o, z = torch.ones_like(c), torch.zeros_like(c)
    rot = torch.stack([torch.stack([c, s, z], -1), torch.stack([-s, c, z], -1), torch.stack([z, z, o], -1)], -2)     # [N, 3, 3]
    return torch.einsum('aij,ajk->aik', points, rot)


class DepthInstance3DBoxes:
    """The part of ``DepthInstance3DBoxes`` (core/bbox/structures/depth_box3d.py) the FCAF3D head, the SUN RGB-D dataset and
    the indoor evaluation touch: (x, y, z, dx, dy, dz[, yaw]) with the origin converted to the bottom centre (0.5, 0.5, 0)."""

    def __init__(self, tensor, box_dim=7, with_yaw=True, origin=(0.5, 0.5, 0)):
        tensor = torch.as_tensor(tensor, dtype=torch.float32)
        if tensor.numel() == 0:
            tensor = tensor.reshape((0, box_dim))
        assert tensor.dim() == 2 and tensor.size(-1) == box_dim, tensor.size()
        if tensor.shape[-1] == 6:
            assert box_dim == 6
            tensor = torch.cat((tensor, tensor.new_zeros(tensor.shape[0], 1)), dim=-1)
            self.box_dim, self.with_yaw = box_dim + 1, False
        else:
            self.box_dim, self.with_yaw = box_dim, with_yaw
        self.tensor = tensor.clone()
        if origin != (0.5, 0.5, 0):
            dst, src = self.tensor.new_tensor((0.5, 0.5, 0)), self.tensor.new_tensor(origin)
            self.tensor[:, :3] += self.tensor[:, 3:6] * (dst - src)

    @property
    def gravity_center(self):
        bc = self.tensor[:, :3]
        gc = torch.zeros_like(bc)
        gc[:, :2] = bc[:, :2]
        gc[:, 2] = bc[:, 2] + self.tensor[:, 5] * 0.5
        return gc

    volume = property(lambda self: self.tensor[:, 3] * self.tensor[:, 4] * self.tensor[:, 5])
    bev = property(lambda self: self.tensor[:, [0, 1, 3, 4, 6]])
    bottom_height = property(lambda self: self.tensor[:, 2])
    top_height = property(lambda self: self.tensor[:, 2] + self.tensor[:, 5])
    device = property(lambda self: self.tensor.device)

    def __len__(self):
        return self.tensor.shape[0]

    def __getitem__(self, item):
        """base_box3d.py:303-337: one box for an int, else what indexing the rows gives."""
        t = self.tensor[item].view(1, -1) if isinstance(item, int) else self.tensor[item]
        assert t.dim() == 2, f'Indexing on Boxes with {item} failed to return a matrix!'
        return self._wrap(t)

    def _wrap(self, tensor):
        out = object.__new__(type(self))
        out.tensor, out.box_dim, out.with_yaw = tensor, self.box_dim, self.with_yaw
        return out

    def to(self, device):
        return self._wrap(self.tensor.to(device))

    def new_box(self, data):
        """base_box3d.py:491-508: a box object of the same kind on the same device from array-like ``data``."""
        t = self.tensor.new_tensor(data) if not isinstance(data, torch.Tensor) else data.to(self.tensor.device)
        return type(self)(t, box_dim=self.box_dim, with_yaw=self.with_yaw)

    # ---- the moves of the train pipelines (depth_box3d.py:93-186, base_box3d.py:210-240), all in place
    MOVES_WITH_POINTS = True          # GlobalRotScaleTrans / RandomFlip3D carry these boxes along with the points

    @property
    def corners(self):
        """[N, 8, 3] corners (depth_box3d.py:38-91): the sizes times the unit corners about the bottom centre, turned by the
        yaw about z, moved to the box."""
        if self.tensor.numel() == 0:
            return torch.empty([0, 8, 3], device=self.tensor.device)
        dims = self.tensor[:, 3:6]
        unit = dims.new_tensor([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]]) - \
            dims.new_tensor([0.5, 0.5, 0])
        corners = rotation_3d_in_axis_z(dims.view(-1, 1, 3) * unit.reshape(1, 8, 3), self.tensor[:, 6])
        return corners + self.tensor[:, :3].view(-1, 1, 3)

    def rotate(self, rot_mat_t):
        """Centres times the transposed rotation about z ``rot_mat_t`` [3, 3]; boxes with a yaw turn by its angle, axis-aligned
        boxes become the axis-aligned boxes that enclose the turned ones."""
        rot_mat_t = self.tensor.new_tensor(rot_mat_t) if not isinstance(rot_mat_t, torch.Tensor) else rot_mat_t.to(self.tensor)
        assert rot_mat_t.shape == torch.Size([3, 3]), f'invalid rotation shape {rot_mat_t.shape}'
        self.tensor[:, 0:3] = self.tensor[:, 0:3] @ rot_mat_t
        if self.with_yaw:
            self.tensor[:, 6] += math.atan2(float(rot_mat_t[0, 1]), float(rot_mat_t[0, 0]))
        elif len(self):
            turned = self.corners @ rot_mat_t
            self.tensor[:, 3] = turned[..., 0].max(dim=1)[0] - turned[..., 0].min(dim=1)[0]
            self.tensor[:, 4] = turned[..., 1].max(dim=1)[0] - turned[..., 1].min(dim=1)[0]

    def flip(self, bev_direction='horizontal'):
        """Depth coordinates: a horizontal flip negates x (yaw -> pi - yaw), a vertical one y (yaw -> -yaw)."""
        assert bev_direction in ('horizontal', 'vertical')
        if bev_direction == 'horizontal':
            self.tensor[:, 0] = -self.tensor[:, 0]
            if self.with_yaw:
                self.tensor[:, 6] = -self.tensor[:, 6] + math.pi
        else:
            self.tensor[:, 1] = -self.tensor[:, 1]
            if self.with_yaw:
                self.tensor[:, 6] = -self.tensor[:, 6]

    def scale(self, scale_factor):
        self.tensor[:, :6] *= scale_factor

    def translate(self, trans_vector):
        if not isinstance(trans_vector, torch.Tensor):
            trans_vector = self.tensor.new_tensor(trans_vector)
        self.tensor[:, :3] += trans_vector

    def convert_to(self, dst, rt_mat=None):
        """depth_box3d.py ``convert_to``: Depth boxes stay what they are; another mode needs Box3DMode, which is not here."""
        if dst is not None and dst not in ('Depth', 'DEPTH', 2) and getattr(dst, 'name', None) != 'DEPTH' and dst is not type(self):
            raise NotImplementedError(f'DepthInstance3DBoxes.convert_to({dst!r}): only the Depth mode is supported')
        return self

    @classmethod
    def height_overlaps(cls, boxes1, boxes2, mode='iou'):
        top = torch.min(boxes1.top_height.view(-1, 1), boxes2.top_height.view(1, -1))
        bottom = torch.max(boxes1.bottom_height.view(-1, 1), boxes2.bottom_height.view(1, -1))
        return torch.clamp(top - bottom, min=0)

    @classmethod
    def overlaps(cls, boxes1, boxes2, mode='iou'):
        """3D IoU / IoF of two box sets (base_box3d.py:437-489), the BEV part on the HIP rotated-IoU kernel."""
        assert type(boxes1) == type(boxes2), f'"boxes1" and "boxes2" should be in the same type, got {type(boxes1)} and {type(boxes2)}.'
        assert mode in ['iou', 'iof']
        rows, cols = len(boxes1), len(boxes2)
        if rows * cols == 0:
            return boxes1.tensor.new(rows, cols)
        overlaps_h = cls.height_overlaps(boxes1, boxes2)
        iou2d = ops.box_iou_rotated(boxes1.bev, boxes2.bev)
        areas1 = (boxes1.bev[:, 2] * boxes1.bev[:, 3]).unsqueeze(1).expand(rows, cols)
        areas2 = (boxes2.bev[:, 2] * boxes2.bev[:, 3]).unsqueeze(0).expand(rows, cols)
        overlaps_bev = iou2d * (areas1 + areas2) / (1 + iou2d)
        overlaps_3d = overlaps_bev.to(boxes1.device) * overlaps_h
        volume1, volume2 = boxes1.volume.view(-1, 1), boxes2.volume.view(1, -1)
        if mode == 'iou':
            return overlaps_3d / torch.clamp(volume1 + volume2 - overlaps_3d, min=1e-8)
        return overlaps_3d / torch.clamp(volume1, min=1e-8)


# ---------------------------------------------------------------------------------------------------------------- losses
def axis_aligned_iou(b1, b2, eps=1e-6):
    """``axis_aligned_bbox_overlaps_3d(..., mode='iou', is_aligned=True)`` (iou3d_calculator.py:210-329) on (x1,y1,z1,x2,y2,z2)."""
    a1 = (b1[..., 3] - b1[..., 0]) * (b1[..., 4] - b1[..., 1]) * (b1[..., 5] - b1[..., 2])
    a2 = (b2[..., 3] - b2[..., 0]) * (b2[..., 4] - b2[..., 1]) * (b2[..., 5] - b2[..., 2])
    wh = (torch.min(b1[..., 3:], b2[..., 3:]) - torch.max(b1[..., :3], b2[..., :3])).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1] * wh[..., 2]
    union = torch.max(a1 + a2 - overlap, a1.new_tensor([eps]))
    return overlap / union


def _box2corners(box):
    """(..., 5) x, y, w, h, alpha -> (..., 4, 2), mmcv's corner order."""
    x, y, w, h, alpha = box.split([1, 1, 1, 1, 1], dim=-1)
    x4 = box.new_tensor([0.5, -0.5, -0.5, 0.5]) * w
    y4 = box.new_tensor([0.5, 0.5, -0.5, -0.5]) * h
    sin, cos = torch.sin(alpha), torch.cos(alpha)
    return torch.stack([x4 * cos - y4 * sin + x, x4 * sin + y4 * cos + y], dim=-1)


def _in_box(c1, c2):
    a, b, d = c2[..., 0:1, :], c2[..., 1:2, :], c2[..., 3:4, :]
    ab, am, ad = b - a, c1 - a, d - a
    p1, p2 = (ab * am).sum(-1) / (ab * ab).sum(-1), (ad * am).sum(-1) / (ad * ad).sum(-1)
    return (p1 > -1e-6) & (p1 < 1 + 1e-6) & (p2 > -1e-6) & (p2 < 1 + 1e-6)


def rotated_iou_3d(box1, box2):
    """mmcv ``diff_iou_rotated_3d`` for aligned pairs, [N, 7] (x, y, z, w, h, l, alpha) -> IoU [N], differentiable: the 24
    candidate vertices of the BEV intersection polygon (4 + 4 corners, 16 edge intersections), the valid ones ordered by
    angle around their mean (mmcv does this step in a CUDA op; indices only, no gradient), shoelace area, times the
    overlap in z."""
    c1, c2 = _box2corners(box1[:, [0, 1, 3, 4, 6]]), _box2corners(box2[:, [0, 1, 3, 4, 6]])          # [N, 4, 2]
    l1 = torch.cat([c1, c1[:, [1, 2, 3, 0]]], -1)[:, :, None]                                       # [N, 4, 1, 4]
    l2 = torch.cat([c2, c2[:, [1, 2, 3, 0]]], -1)[:, None]                                          # [N, 1, 4, 4]
    x1, y1, x2, y2 = l1.unbind(-1)
    x3, y3, x4, y4 = l2.unbind(-1)
    num = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4)
    den_t = (x1 - x3) * (y3 - y4) - (y1 - y3) * (x3 - x4)
    den_u = (x1 - x2) * (y1 - y3) - (y1 - y2) * (x1 - x3)
    zero = num == 0
    t = torch.where(zero, torch.full_like(num, -1.0), den_t / torch.where(zero, torch.ones_like(num), num))
    u = torch.where(zero, torch.full_like(num, -1.0), -den_u / torch.where(zero, torch.ones_like(num), num))
    mask = ((t > 0) & (t < 1) & (u > 0) & (u < 1)).detach()
    t = den_t / (num + 1e-8)
    inter = torch.stack([x1 + t * (x2 - x1), y1 + t * (y2 - y1)], -1) * mask[..., None].float()    # [N, 4, 4, 2]
    N = box1.shape[0]
    verts = torch.cat([c1, c2, inter.reshape(N, 16, 2), c1.new_zeros(N, 1, 2)], 1)                  # [N, 25, 2]; 24 = the zero pad vertex
    vmask = torch.cat([_in_box(c1, c2), _in_box(c2, c1), mask.reshape(N, 16), mask.new_zeros(N, 1)], 1)
    with torch.no_grad():
        nv = vmask.sum(1)
        mean = (verts * vmask[..., None].float()).sum(1, keepdim=True) / nv.clamp(min=1)[:, None, None]
        vn = verts - mean
        ang = torch.atan2(vn[..., 1], vn[..., 0])
        ang = torch.where(vmask, ang, torch.full_like(ang, float('inf')))
        order = torch.argsort(ang, dim=1)[:, :8]                                                    # valid vertices first, by angle
        j = torch.arange(9, device=box1.device)[None]
        idx = torch.where(j < nv[:, None], torch.cat([order, order[:, :1]], 1), torch.full((N, 9), 24, device=box1.device))
        idx = torch.where(j == nv[:, None], order[:, :1].expand(-1, 9), idx)                        # close the polygon
        idx = torch.where((nv < 3)[:, None], torch.full_like(idx, 24), idx)
    sel = torch.gather(verts, 1, idx[..., None].expand(-1, -1, 2))
    area = (sel[:, :-1, 0] * sel[:, 1:, 1] - sel[:, :-1, 1] * sel[:, 1:, 0]).sum(1).abs() / 2
    zmax = torch.min(box1[:, 2] + box1[:, 5] * 0.5, box2[:, 2] + box2[:, 5] * 0.5)
    zmin = torch.max(box1[:, 2] - box1[:, 5] * 0.5, box2[:, 2] - box2[:, 5] * 0.5)
    inter3d = area * (zmax - zmin).clamp(min=0)
    vol1, vol2 = box1[:, 3] * box1[:, 4] * box1[:, 5], box2[:, 3] * box2[:, 4] * box2[:, 5]
    return inter3d / (vol1 + vol2 - inter3d)


class _IoULoss(nn.Module):
    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        assert reduction in ('none', 'sum', 'mean')
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        if weight is not None and not torch.any(weight > 0):          # the two reference classes word this case differently
            if type(self) is RotatedIoU3DLoss:
                return pred.sum() * weight.sum()
            if reduction != 'none':
                return (pred * weight).sum()
        if type(self) is RotatedIoU3DLoss and weight is not None and weight.dim() > 1:
            weight = weight.mean(-1)
        return self.loss_weight * weight_reduce_loss(1 - self.iou(pred, target), weight, reduction, avg_factor)


@LOSSES.register_module()
class AxisAlignedIoULoss(_IoULoss):
    """models/losses/axis_aligned_iou_loss.py:10-80: 1 - IoU of (x1, y1, z1, x2, y2, z2) boxes."""
    iou = staticmethod(axis_aligned_iou)


@LOSSES.register_module()
class RotatedIoU3DLoss(_IoULoss):
    """models/losses/rotated_iou_loss.py:10-86: 1 - diff_iou_rotated_3d of (x, y, z, w, l, h, alpha) boxes."""
    iou = staticmethod(rotated_iou_3d)


def nms3d(boxes, scores, iou_threshold):
    """mmcv ``nms3d``: greedy NMS on the BEV overlap of the upright boxes [N, 7] (x, y, z, dx, dy, dz, heading) -> kept
    indices in descending score order."""
    if boxes.shape[0] == 0:
        return torch.zeros(0, dtype=torch.long, device=boxes.device)
    return ops.nms_rotated(boxes[:, [0, 1, 3, 4, 6]].contiguous(), scores.contiguous(), iou_threshold)[1]


def nms3d_normal(boxes, scores, iou_threshold):
    """mmcv ``nms3d_normal``: the same with the heading ignored (axis-aligned BEV boxes)."""
    b = boxes[:, [0, 1, 3, 4, 6]].clone()
    b[:, 4] = 0
    if boxes.shape[0] == 0:
        return torch.zeros(0, dtype=torch.long, device=boxes.device)
    return ops.nms_rotated(b.contiguous(), scores.contiguous(), iou_threshold)[1]


class _SplitRows(torch.autograd.Function):
    """t [n, C], index vectors with DISTINCT rows overall -> tuple(t[p] for p in perms). Backward: every gradient is copied
    to its rows of one zero tensor (no duplicates, so no accumulation and no sort)."""

    @staticmethod
    def forward(ctx, t, *perms):
        ctx.perms, ctx.shape = perms, t.shape
        return tuple(t.index_select(0, p) for p in perms)

    @staticmethod
    def backward(ctx, *gs):
        g = gs[0].new_zeros(ctx.shape) if gs[0] is not None else None
        for p, gi in zip(ctx.perms, gs):
            if gi is not None:
                if g is None:
                    g = gi.new_zeros(ctx.shape)
                g.index_copy_(0, p, gi)
        return (g,) + (None,) * len(ctx.perms)


def split_rows(t, perms):
    """[t[p] for p in perms] for index vectors that name every row at most once (the samples of a batch)."""
    perms = list(perms)
    if not perms or not t.requires_grad:
        return [t[p] for p in perms]
    return list(_SplitRows.apply(t, *perms))


def take_rows(t, idx):
    """t[idx] for an index vector without duplicates (e.g. from nonzero)."""
    if not t.requires_grad:
        return t[idx]
    return _SplitRows.apply(t, idx)[0]


class Scale(nn.Module):
    """mmcv.cnn.Scale: a learnable scalar factor."""

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

    def forward(self, x):
        return x * self.scale


def bias_init_with_prob(prior_prob):
    return float(-math.log((1 - prior_prob) / prior_prob))


def reduce_mean(tensor):
    """mmdet.core.reduce_mean: the mean over the ranks (the one collective of this head besides the gradient all-reduce)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return tensor
    tensor = tensor.clone()
    dist.all_reduce(tensor.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
    return tensor


# -------------------------------------------------------------------------------------------------------------- backbone
@BACKBONES.register_module()
class MinkResNet(nn.Module):
    arch_settings = {18: (ME.BasicBlock, (2, 2, 2, 2)), 34: (ME.BasicBlock, (3, 4, 6, 3))}

    def __init__(self, depth, in_channels, num_stages=4, pool=True):
        super().__init__()
        if depth not in self.arch_settings:
            raise KeyError(f'invalid depth {depth} for resnet (the BasicBlock depths 18 / 34 are built)')
        assert 4 >= num_stages >= 1
        block, stage_blocks = self.arch_settings[depth]
        stage_blocks = stage_blocks[:num_stages]
        self.num_stages, self.pool = num_stages, pool
        self.inplanes = 64
        self.conv1 = ME.MinkowskiConvolution(in_channels, self.inplanes, kernel_size=3, stride=2, dimension=3)
        self.norm1 = ME.MinkowskiInstanceNorm(self.inplanes)
        self.relu = ME.MinkowskiReLU(inplace=True)
        if self.pool:
            self.maxpool = ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=3)
        for i, _ in enumerate(stage_blocks):
            setattr(self, f'layer{i + 1}', self._make_layer(block, 64 * 2 ** i, stage_blocks[i], stride=2))

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, ME.MinkowskiConvolution):        # ME.utils.kaiming_normal_(kernel, mode='fan_out', nonlinearity='relu')
                fan_out = m.kernel.shape[0] * m.kernel.shape[2]
                nn.init.normal_(m.kernel, 0, math.sqrt(2.0 / fan_out))
            if isinstance(m, ME.MinkowskiBatchNorm):
                nn.init.constant_(m.bn.weight, 1)
                nn.init.constant_(m.bn.bias, 0)

    def _make_layer(self, block, planes, blocks, stride):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                ME.MinkowskiConvolution(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, dimension=3),
                ME.MinkowskiBatchNorm(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride=stride, downsample=downsample, dimension=3)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, stride=1, dimension=3))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.relu(self.norm1(self.conv1(x)))
        if self.pool:
            x = self.maxpool(x)
        outs = []
        for i in range(self.num_stages):
            x = getattr(self, f'layer{i + 1}')(x)
            outs.append(x)
        return outs


# ------------------------------------------------------------------------------------------------------------------ head
from .fcaf3d_head import FCAF3DHead, LevelOutput, decode_boxes, top_per_segment       # noqa: E402,F401  (registers the head)


# -------------------------------------------------------------------------------------------------------------- detector
@DETECTORS.register_module()
class MinkSingleStage3DDetector(nn.Module):
    def __init__(self, backbone, head, voxel_size, train_cfg=None, test_cfg=None, init_cfg=None, pretrained=None):
        super().__init__()
        self.backbone = build_backbone(backbone)
        head = dict(head)
        head.update(train_cfg=train_cfg)
        head.update(test_cfg=test_cfg)
        self.head = build_head(head)
        self.voxel_size = voxel_size
        self.init_weights()

    def init_weights(self):
        self.backbone.init_weights()
        self.head.init_weights()

    def extract_feat(self, points):
        coordinates, features = ME.batch_sparse_collate([(p[:, :3] / self.voxel_size, p[:, 3:]) for p in points], device=points[0].device)
        x = ME.SparseTensor(coordinates=coordinates, features=features, batch_size=len(points))
        return self.backbone(x)

    def forward_train(self, points, gt_bboxes_3d, gt_labels_3d, img_metas):
        x = self.extract_feat(points)
        return self.head.forward_train(x, gt_bboxes_3d, gt_labels_3d, img_metas)

    @torch.no_grad()
    def simple_test(self, points, img_metas, *args, **kwargs):
        from .box3d import bbox3d2result
        x = self.extract_feat(points)
        bbox_list = self.head.forward_test(x, img_metas)
        return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in bbox_list]

    def aug_test(self, points, img_metas, **kwargs):
        raise NotImplementedError

    def forward(self, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(**kwargs)
        return self.simple_test(kwargs['points'][0], kwargs['img_metas'][0])

    def _parse_losses(self, losses):
        from collections import OrderedDict
        log_vars = OrderedDict((k, v.mean() if isinstance(v, torch.Tensor) else sum(x.mean() for x in v)) for k, v in losses.items())
        loss = torch.stack([v for k, v in log_vars.items() if 'loss' in k]).sum()
        log_vars['loss'] = loss
        return loss, log_vars

    def train_step(self, data, optimizer=None):
        losses = self(**data)
        loss, log_vars = self._parse_losses(losses)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data['img_metas']))
