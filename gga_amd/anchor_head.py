"""``Anchor3DHead`` with its anchor generators, assigner, sampler and box coder - the head of the KITTI SECOND / PointPillars
detectors (``VoxelNet``), under the reference's registry names, constructor keys, ``state_dict`` names and loss-dict keys:

* ``Anchor3DRangeGenerator`` / ``AlignedAnchor3DRangeGenerator`` - mmdet3d/core/anchor/anchor_3d_generator.py:20-340
* ``DeltaXYZWLHRBBoxCoder`` - mmdet3d/core/bbox/coders/delta_xyzwhlr_bbox_coder.py:20-91
* ``BboxOverlapsNearest3D`` - mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py:9-145, structures/base_box3d.py:144-162
* ``MaxIoUAssigner`` / ``PseudoSampler`` / ``bbox_overlaps`` - mmdet (third-party, not in the reference tree), restated from
  their published behaviour; the reference's known answer tests/test_utils/test_assigners.py:13-34 pins the assigner
* ``Anchor3DHead`` - mmdet3d/models/dense_heads/anchor3d_head.py:42-516 with train_mixins.py:9-349

What differs is where the work of a training step runs. The reference assigns targets frame by frame and, inside a frame,
assigner by assigner: an IoU matrix, a few ``max`` calls, a Python loop over the ground truths and several ``nonzero`` calls
each, then a positive-anchor gather and three eager losses. Here the boxes of the batch go up in one staging buffer,
``functional.anchor_targets`` builds every target of the batch with nothing read back, and ``functional.anchor_losses`` computes the
three losses in one entry point each way, reading ``avg_factor`` on the device (csrc/anchor_head.hip). ``get_bboxes`` decodes
the kept anchors of all frames in one launch and runs the per-class NMS of all frames at once. The reference's loops stay as the
eager path: the fallback for what the kernels do not cover and what the tests compare the kernels against.
"""
import os

import numpy as np
import torch
from torch import nn

from . import functional as F
from . import ops
from .bbox_coders import limit_period
from .cnn import build_conv_layer
from .dense_heads import _to_np, multi_apply
from .registry import (BBOX_ASSIGNERS, BBOX_CODERS, BBOX_SAMPLERS, HEADS, IOU_CALCULATORS, PRIOR_GENERATORS, build_assigner,
                       build_bbox_coder, build_iou_calculator, build_loss, build_prior_generator, build_sampler)

# GGA_ANCHOR_TARGETS=0: the eager per-frame, per-assigner targets and the eager losses (the reference's sequence of launches).
DEVICE_TARGETS = os.environ.get('GGA_ANCHOR_TARGETS', '1') != '0'
# GGA_ANCHOR_DETECT_BATCHED=0: ``get_bboxes`` loops over the frames.
DETECT_BATCHED = os.environ.get('GGA_ANCHOR_DETECT_BATCHED', '1') != '0'


def _get(cfg, key, default=None):
    if cfg is None:
        return default
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


# ----------------------------------------------------------------------------- anchor generators
@PRIOR_GENERATORS.register_module()
class Anchor3DRangeGenerator:
    """Anchors spread uniformly between the ends of a range (anchor_3d_generator.py:20-221): per level a tensor
    ``[1, H, W, n_sizes, n_rot, 7 + len(custom_values)]`` of (x, y, z, dx, dy, dz, yaw), flattened to ``[N, .]`` with
    ``reshape_out``. The centres are ``torch.linspace`` between the range's ends, as the reference builds them, so the values
    are the reference's bit for bit. Built once per (feature-map sizes, device) and kept."""

    def __init__(self, ranges, sizes=[[3.9, 1.6, 1.56]], scales=[1], rotations=[0, 1.5707963], custom_values=(), reshape_out=True,
                 size_per_range=True):
        assert isinstance(ranges, (list, tuple)) and all(isinstance(r, (list, tuple)) for r in ranges)
        assert isinstance(sizes, (list, tuple)) and all(isinstance(s, (list, tuple)) for s in sizes)
        assert isinstance(scales, (list, tuple))
        ranges = [list(r) for r in ranges]
        if size_per_range:
            if len(sizes) != len(ranges):
                assert len(ranges) == 1
                ranges = ranges * len(sizes)
            assert len(ranges) == len(sizes)
        else:
            assert len(ranges) == 1
        self.sizes, self.scales, self.ranges, self.rotations = [list(s) for s in sizes], list(scales), ranges, list(rotations)
        self.custom_values, self.reshape_out, self.size_per_range = custom_values, reshape_out, size_per_range
        self.cached_anchors = None
        self._cache = {}

    def __repr__(self):
        return (f'{self.__class__.__name__}(anchor_range={self.ranges},\nscales={self.scales},\nsizes={self.sizes},\n'
                f'rotations={self.rotations},\nreshape_out={self.reshape_out},\nsize_per_range={self.size_per_range})')

    @property
    def num_base_anchors(self):
        return len(self.rotations) * int(np.asarray(self.sizes, dtype=np.float64).reshape(-1, 3).shape[0])

    @property
    def num_levels(self):
        return len(self.scales)

    def grid_anchors(self, featmap_sizes, device='cuda'):
        assert self.num_levels == len(featmap_sizes)
        key = (tuple(tuple(int(v) for v in s) for s in featmap_sizes), str(torch.device(device)))
        hit = self._cache.get(key)
        if hit is None:
            hit = []
            for size, scale in zip(featmap_sizes, self.scales):
                anchors = self.single_level_grid_anchors(size, scale, device=device)
                hit.append(anchors.reshape(-1, anchors.size(-1)) if self.reshape_out else anchors)
            if len(self._cache) > 16:
                self._cache.clear()
            self._cache[key] = hit
        return list(hit)

    def single_level_grid_anchors(self, featmap_size, scale, device='cuda'):
        if not self.size_per_range:
            return self.anchors_single_range(featmap_size, self.ranges[0], scale, self.sizes, self.rotations, device=device)
        per_range = [self.anchors_single_range(featmap_size, r, scale, s, self.rotations, device=device)
                     for r, s in zip(self.ranges, self.sizes)]
        return torch.cat(per_range, dim=-3)

    def _centres(self, lo, hi, n, device):
        """``n`` centres of one axis between the tensor elements ``lo`` and ``hi``."""
        return torch.linspace(lo, hi, n, device=device)

    def anchors_single_range(self, feature_size, anchor_range, scale=1, sizes=[[3.9, 1.6, 1.56]], rotations=[0, 1.5707963],
                             device='cuda'):
        """-> ``[D, H, W, n_sizes, n_rot, 7 (+ custom)]`` for ``feature_size`` (D, H, W) or (H, W)."""
        if len(feature_size) == 2:
            feature_size = [1, feature_size[0], feature_size[1]]
        D, H, W = (int(v) for v in feature_size)
        rng = torch.tensor(anchor_range, device=device)
        z = self._centres(rng[2], rng[5], D, device)
        y = self._centres(rng[1], rng[4], H, device)
        x = self._centres(rng[0], rng[3], W, device)
        sizes = torch.tensor(sizes, device=device).reshape(-1, 3) * scale
        rot = torch.tensor(rotations, device=device)
        S, R = sizes.shape[0], rot.shape[0]
        out = x.new_zeros((D, H, W, S, R, 7 + len(self.custom_values)))       # custom values: zeros, as in the reference
        out[..., 0] = x.view(1, 1, W, 1, 1)
        out[..., 1] = y.view(1, H, 1, 1, 1)
        out[..., 2] = z.view(D, 1, 1, 1, 1)
        out[..., 3:6] = sizes.view(1, 1, 1, S, 1, 3)
        out[..., 6] = rot.view(1, 1, 1, 1, R)
        return out


@PRIOR_GENERATORS.register_module()
class AlignedAnchor3DRangeGenerator(Anchor3DRangeGenerator):
    """Anchors at the centres of the feature grid's cells (anchor_3d_generator.py:224-340): ``n + 1`` cell corners between the
    range's ends, moved by half a cell (unless ``align_corner``), the first ``n`` kept."""

    def __init__(self, align_corner=False, **kwargs):
        super().__init__(**kwargs)
        self.align_corner = align_corner

    def _centres(self, lo, hi, n, device):
        c = torch.linspace(lo, hi, n + 1, device=device)
        if not self.align_corner:
            c += (c[1] - c[0]) / 2
        return c[:n]


# ----------------------------------------------------------------------------- box coder
@BBOX_CODERS.register_module()
class DeltaXYZWLHRBBoxCoder:
    """delta_xyzwhlr_bbox_coder.py:9-91: centre offsets over the BEV diagonal (z over the height), log size ratios, yaw
    difference; extra code entries (velocities) are plain differences."""

    def __init__(self, code_size=7):
        self.code_size = code_size

    @staticmethod
    def encode(src_boxes, dst_boxes):
        xa, ya, za, wa, la, ha, ra, *cas = torch.split(src_boxes, 1, dim=-1)
        xg, yg, zg, wg, lg, hg, rg, *cgs = torch.split(dst_boxes, 1, dim=-1)
        za = za + ha / 2
        zg = zg + hg / 2
        diagonal = torch.sqrt(la**2 + wa**2)
        return torch.cat([(xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / ha, torch.log(wg / wa), torch.log(lg / la),
                          torch.log(hg / ha), rg - ra, *[g - a for g, a in zip(cgs, cas)]], dim=-1)

    @staticmethod
    def decode(anchors, deltas):
        xa, ya, za, wa, la, ha, ra, *cas = torch.split(anchors, 1, dim=-1)
        xt, yt, zt, wt, lt, ht, rt, *cts = torch.split(deltas, 1, dim=-1)
        za = za + ha / 2
        diagonal = torch.sqrt(la**2 + wa**2)
        xg = xt * diagonal + xa
        yg = yt * diagonal + ya
        zg = zt * ha + za
        lg = torch.exp(lt) * la
        wg = torch.exp(wt) * wa
        hg = torch.exp(ht) * ha
        rg = rt + ra
        zg = zg - hg / 2
        return torch.cat([xg, yg, zg, wg, lg, hg, rg, *[t + a for t, a in zip(cts, cas)]], dim=-1)


# ----------------------------------------------------------------------------- IoU, assigner, sampler
def bbox_overlaps(bboxes1, bboxes2, mode='iou', is_aligned=False, eps=1e-6):
    """mmdet.core.bbox.bbox_overlaps for (x1, y1, x2, y2) boxes: [M, 4] x [N, 4] -> [M, N] (``is_aligned``: [M])."""
    assert mode in ('iou', 'iof')
    area1 = (bboxes1[..., 2] - bboxes1[..., 0]) * (bboxes1[..., 3] - bboxes1[..., 1])
    area2 = (bboxes2[..., 2] - bboxes2[..., 0]) * (bboxes2[..., 3] - bboxes2[..., 1])
    if is_aligned:
        lt, rb = torch.max(bboxes1[..., :2], bboxes2[..., :2]), torch.min(bboxes1[..., 2:], bboxes2[..., 2:])
    else:
        lt = torch.max(bboxes1[..., :, None, :2], bboxes2[..., None, :, :2])
        rb = torch.min(bboxes1[..., :, None, 2:], bboxes2[..., None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    if mode == 'iou':
        union = area1 + area2 - overlap if is_aligned else area1[..., None] + area2[..., None, :] - overlap
    else:
        union = area1 if is_aligned else area1[..., None]
    return overlap / torch.max(union, union.new_tensor([eps]))


def nearest_bev(boxes):
    """base_box3d.py:144-162: the axis-aligned BEV box (x1, y1, x2, y2) nearest to each (x, y, z, dx, dy, dz, yaw, ...)."""
    normed = torch.abs(limit_period(boxes[:, 6], 0.5, np.pi))
    xywh = torch.where((normed > np.pi / 4)[..., None], boxes[:, [0, 1, 4, 3]], boxes[:, [0, 1, 3, 4]])
    centers, dims = xywh[:, :2], xywh[:, 2:]
    return torch.cat([centers - dims / 2, centers + dims / 2], dim=-1)


@IOU_CALCULATORS.register_module()
class BboxOverlaps2D:
    """mmdet's default calculator of ``MaxIoUAssigner``: plain (x1, y1, x2, y2) boxes."""

    def __call__(self, bboxes1, bboxes2, mode='iou', is_aligned=False):
        return bbox_overlaps(bboxes1[..., :4], bboxes2[..., :4], mode, is_aligned)


@IOU_CALCULATORS.register_module()
class BboxOverlapsNearest3D:
    def __init__(self, coordinate='lidar'):
        assert coordinate in ['camera', 'lidar', 'depth']
        if coordinate != 'lidar':
            raise NotImplementedError(f'BboxOverlapsNearest3D: coordinate={coordinate!r}; the anchor head works on LiDAR boxes')
        self.coordinate = coordinate

    def __call__(self, bboxes1, bboxes2, mode='iou', is_aligned=False):
        assert bboxes1.size(-1) == bboxes2.size(-1) >= 7
        return bbox_overlaps(nearest_bev(bboxes1), nearest_bev(bboxes2), mode=mode, is_aligned=is_aligned)

    def __repr__(self):
        return f'{self.__class__.__name__}(coordinate={self.coordinate}'


class AssignResult:
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


@BBOX_ASSIGNERS.register_module()
class MaxIoUAssigner:
    """mmdet's MaxIoUAssigner with the options the KITTI configs use. ``gt_inds``: -1 ignored, 0 negative, i + 1 = ground truth i.

    1. every box starts at -1;
    2. ``0 <= max_iou < neg_iou_thr`` -> 0;
    3. ``max_iou >= pos_iou_thr`` -> ``argmax + 1``;
    4. for each ground truth i in ascending order with ``gt_max[i] >= min_pos_iou``: every box with ``iou[i, box] == gt_max[i]``
       -> ``i + 1`` (a later ground truth overwrites an earlier one, and a step-3 assignment)."""

    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, gt_max_assign_all=True, ignore_iof_thr=-1,
                 ignore_wrt_candidates=True, match_low_quality=True, gpu_assign_thr=-1, iou_calculator=dict(type='BboxOverlaps2D')):
        for key, val, ok in (('neg_iou_thr', neg_iou_thr, isinstance(neg_iou_thr, (int, float))),
                             ('gt_max_assign_all', gt_max_assign_all, gt_max_assign_all is True),
                             ('match_low_quality', match_low_quality, match_low_quality is True),
                             ('ignore_iof_thr', ignore_iof_thr, ignore_iof_thr <= 0 if isinstance(ignore_iof_thr, (int, float)) else False),
                             ('gpu_assign_thr', gpu_assign_thr, gpu_assign_thr <= 0 if isinstance(gpu_assign_thr, (int, float)) else False)):
            if not ok:
                raise NotImplementedError(f'MaxIoUAssigner: {key}={val!r} is not supported')
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou = pos_iou_thr, float(neg_iou_thr), min_pos_iou
        self.gt_max_assign_all, self.ignore_iof_thr, self.ignore_wrt_candidates = gt_max_assign_all, ignore_iof_thr, ignore_wrt_candidates
        self.match_low_quality, self.gpu_assign_thr = match_low_quality, gpu_assign_thr
        self.iou_calculator = build_iou_calculator(iou_calculator)

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        return self.assign_wrt_overlaps(self.iou_calculator(gt_bboxes, bboxes), gt_labels)

    def assign_wrt_overlaps(self, overlaps, gt_labels=None):
        num_gts, num_bboxes = overlaps.size(0), overlaps.size(1)
        gt_inds = overlaps.new_full((num_bboxes, ), -1, dtype=torch.long)
        if num_gts == 0 or num_bboxes == 0:
            if num_gts == 0:
                gt_inds[:] = 0
            labels = None if gt_labels is None else overlaps.new_full((num_bboxes, ), -1, dtype=torch.long)
            return AssignResult(num_gts, gt_inds, overlaps.new_zeros((num_bboxes, )), labels)
        max_overlaps, argmax_overlaps = overlaps.max(dim=0)
        gt_max_overlaps = overlaps.max(dim=1)[0]
        gt_inds[(max_overlaps >= 0) & (max_overlaps < self.neg_iou_thr)] = 0
        pos = max_overlaps >= self.pos_iou_thr
        gt_inds[pos] = argmax_overlaps[pos] + 1
        for i in range(num_gts):
            if gt_max_overlaps[i] >= self.min_pos_iou:
                gt_inds[overlaps[i, :] == gt_max_overlaps[i]] = i + 1
        labels = None
        if gt_labels is not None:
            labels = gt_inds.new_full((num_bboxes, ), -1)
            pos_inds = torch.nonzero(gt_inds > 0, as_tuple=False).squeeze(-1)
            if pos_inds.numel() > 0:
                labels[pos_inds] = gt_labels[gt_inds[pos_inds] - 1]
        return AssignResult(num_gts, gt_inds, max_overlaps, labels)


class SamplingResult:
    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.num_gts = gt_bboxes.shape[0]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        self.pos_gt_bboxes = gt_bboxes[self.pos_assigned_gt_inds.long(), :] if gt_bboxes.numel() else gt_bboxes.view(-1, bboxes.shape[-1])


@BBOX_SAMPLERS.register_module()
class PseudoSampler:
    """Every assigned box is a positive and every box with index 0 a negative (mmdet's PseudoSampler)."""

    def __init__(self, **kwargs):
        pass

    def sample(self, assign_result, bboxes, gt_bboxes, **kwargs):
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        return SamplingResult(pos_inds, neg_inds, bboxes, gt_bboxes, assign_result)


def get_direction_target(anchors, reg_targets, dir_offset=0, dir_limit_offset=0, num_bins=2, one_hot=True):
    """train_mixins.py:319-349: the bin of the ground truth's yaw (anchor yaw + encoded difference) in [0, num_bins)."""
    rot_gt = reg_targets[..., 6] + anchors[..., 6]
    offset_rot = limit_period(rot_gt - dir_offset, dir_limit_offset, 2 * np.pi)
    dir_cls_targets = torch.clamp(torch.floor(offset_rot / (2 * np.pi / num_bins)).long(), min=0, max=num_bins - 1)
    if one_hot:
        return torch.nn.functional.one_hot(dir_cls_targets, num_bins).to(anchors.dtype)
    return dir_cls_targets


def images_to_levels(target, num_levels):
    """mmdet.core.images_to_levels: per-image targets -> per-level [B, n_level, ...] tensors."""
    target = torch.stack(target, 0)
    out, start = [], 0
    for n in num_levels:
        out.append(target[:, start:start + n])
        start += n
    return out


# ----------------------------------------------------------------------------- the head
@HEADS.register_module()
class Anchor3DHead(nn.Module):
    """The anchor head of SECOND / PointPillars (anchor3d_head.py:15-516): three 1x1 convolutions (``conv_cls``, ``conv_reg``,
    ``conv_dir_cls``) over the neck's map, ``n_sizes * n_rot`` anchors per cell. ``loss`` and ``get_bboxes`` take the device
    paths of this module's header where they apply (``_device_path``, ``_get_bboxes_batched``) and the reference's loops
    otherwise."""

    def __init__(self, num_classes, in_channels, train_cfg, test_cfg, feat_channels=256, use_direction_classifier=True,
                 anchor_generator=dict(type='Anchor3DRangeGenerator', range=[0, -39.68, -1.78, 69.12, 39.68, -1.78], strides=[2],
                                       sizes=[[3.9, 1.6, 1.56]], rotations=[0, 1.57], custom_values=[], reshape_out=False),
                 assigner_per_size=False, assign_per_class=False, diff_rad_by_sin=True, dir_offset=-np.pi / 2, dir_limit_offset=0,
                 bbox_coder=dict(type='DeltaXYZWLHRBBoxCoder'),
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=2.0),
                 loss_dir=dict(type='CrossEntropyLoss', loss_weight=0.2), init_cfg=None):
        super().__init__()
        self.in_channels, self.num_classes, self.feat_channels = in_channels, num_classes, feat_channels
        self.diff_rad_by_sin, self.use_direction_classifier = diff_rad_by_sin, use_direction_classifier
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.assigner_per_size, self.assign_per_class = assigner_per_size, assign_per_class
        self.dir_offset, self.dir_limit_offset = dir_offset, dir_limit_offset
        self.fp16_enabled = False
        self.anchor_generator = build_prior_generator(anchor_generator)
        self.num_anchors = self.anchor_generator.num_base_anchors
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.box_code_size = self.bbox_coder.code_size
        self.use_sigmoid_cls = loss_cls.get('use_sigmoid', False)
        self.sampling = loss_cls['type'] not in ['FocalLoss', 'GHMC']
        if not self.use_sigmoid_cls:
            self.num_classes += 1
        self.loss_cls, self.loss_bbox, self.loss_dir = build_loss(loss_cls), build_loss(loss_bbox), build_loss(loss_dir)
        self._init_layers()
        self._init_assigner_sampler()
        self.init_weights()

    def _init_assigner_sampler(self):
        if self.train_cfg is None:
            return
        self.bbox_sampler = build_sampler(_get(self.train_cfg, 'sampler')) if self.sampling else PseudoSampler()
        assigner = _get(self.train_cfg, 'assigner')
        if isinstance(assigner, dict):
            self.bbox_assigner = build_assigner(assigner)
        elif isinstance(assigner, (list, tuple)):
            self.bbox_assigner = [build_assigner(a) for a in assigner]

    def _init_layers(self):
        conv = dict(type='Conv2d')
        self.cls_out_channels = self.num_anchors * self.num_classes
        self.conv_cls = build_conv_layer(conv, self.feat_channels, self.cls_out_channels, 1)
        self.conv_reg = build_conv_layer(conv, self.feat_channels, self.num_anchors * self.box_code_size, 1)
        if self.use_direction_classifier:
            self.conv_dir_cls = build_conv_layer(conv, self.feat_channels, self.num_anchors * 2, 1)

    def init_weights(self):
        """The reference's init_cfg: Normal(std 0.01) on every conv, ``conv_cls`` with the bias of a prior probability 0.01."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, mean=0, std=0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.conv_cls.bias, float(-np.log((1 - 0.01) / 0.01)))

    def forward_single(self, x):
        return self.conv_cls(x), self.conv_reg(x), self.conv_dir_cls(x) if self.use_direction_classifier else None

    def forward(self, feats):
        return multi_apply(self.forward_single, feats)

    def get_anchors(self, featmap_sizes, input_metas, device='cuda'):
        multi_level_anchors = self.anchor_generator.grid_anchors(featmap_sizes, device=device)
        return [multi_level_anchors for _ in range(len(input_metas))]

    # ------------------------------------------------------------------ targets
    def _device_path(self, cls_scores):
        """Whether the kernels cover this head and these maps; everything else takes the eager path."""
        from .losses import CrossEntropyLoss, FocalLoss, SmoothL1Loss
        lc, lb, ld = self.loss_cls, self.loss_bbox, self.loss_dir
        return (DEVICE_TARGETS and len(cls_scores) == 1 and cls_scores[0].is_cuda and self.box_code_size == 7
                and self.use_sigmoid_cls and isinstance(getattr(self, 'bbox_sampler', None), PseudoSampler)
                and len(self.anchor_generator.custom_values) == 0
                and type(lc) is FocalLoss and not lc.activated and lc.reduction == 'mean'
                and type(lb) is SmoothL1Loss and lb.reduction == 'mean' and lb.beta > 0
                and type(ld) is CrossEntropyLoss and not ld.use_sigmoid and ld.class_weight is None and ld.reduction == 'mean'
                and self._anchor_params(2) is not None)

    def _anchor_params(self, n_rot):
        assigners = self.bbox_assigner if isinstance(self.bbox_assigner, list) else [self.bbox_assigner]
        if not all(type(a) is MaxIoUAssigner and isinstance(a.iou_calculator, BboxOverlapsNearest3D) for a in assigners) or \
                len(assigners) > F._lib.ANCHOR_MAX_GROUPS:
            return None
        return F.anchor_params([a.pos_iou_thr for a in assigners], [a.neg_iou_thr for a in assigners],
                               [a.min_pos_iou for a in assigners], n_rot, self.num_classes,
                               self.assign_per_class and isinstance(self.bbox_assigner, list), _get(self.train_cfg, 'pos_weight', -1),
                               self.dir_offset, self.dir_limit_offset)

    def pack_targets(self, gt_bboxes, gt_labels):
        """Host half of the device targets: the batch's boxes and labels as flat arrays and the frames' offsets (numpy only)."""
        boxes = [_to_np(getattr(b, 'tensor', b), np.float32).reshape(-1, 7) for b in gt_bboxes]
        labels = [_to_np(l, np.int64).reshape(-1) for l in gt_labels]
        if len(boxes) != len(labels) or any(len(b) != len(l) for b, l in zip(boxes, labels)):
            raise ValueError('Anchor3DHead.get_targets: one label per box in every frame')
        offs = np.zeros(len(boxes) + 1, np.int32)
        offs[1:] = np.cumsum([len(b) for b in boxes])
        return dict(boxes=np.concatenate(boxes) if boxes else np.zeros((0, 7), np.float32),
                    labels=np.concatenate(labels) if labels else np.zeros(0, np.int64), frame_offsets=offs)

    def get_targets(self, anchors, gt_bboxes, gt_labels, device=None, bbox_weights=False):
        """The targets of a batch on the device (train_mixins.py:12-316 for one level, PseudoSampler): ``anchors`` = the level's
        anchors ``[1, H, W, n_sizes, n_rot, 7]`` (or flat, with ``n_rot`` rotations innermost). -> the dict of
        ``functional.anchor_targets`` (``labels``, ``label_weights``, ``bbox_targets``, ``pos``, ``dir_targets``, ``dir_weights``,
        ``pos_count``); ``bbox_weights=True`` adds the reference's ``[B, A, 7]`` weights, expanded from ``pos``.

        A ground truth whose label lies outside ``[0, num_classes)`` takes no part (the reference would index out of range):
        ``KittiDataset`` removes DontCare and ``ObjectNameFilter`` the classes the head does not know."""
        n_rot = len(self.anchor_generator.rotations)
        dev = torch.device(device) if device is not None else anchors.device
        prm = self._anchor_params(n_rot) if hasattr(self, 'bbox_assigner') else None
        if not (DEVICE_TARGETS and dev.type == 'cuda' and prm is not None and anchors.size(-1) == 7
                and isinstance(self.bbox_sampler, PseudoSampler)):
            return self._get_targets_eager(anchors.to(dev), gt_bboxes, gt_labels, bbox_weights)
        if prm.n_groups > 1 and (anchors.dim() != 6 or anchors.size(-3) != prm.n_groups or anchors.size(-2) != n_rot):
            raise ValueError(f'Anchor3DHead.get_targets: {prm.n_groups} assigners need anchors [1, H, W, {prm.n_groups}, {n_rot}, 7], '
                             f'got {tuple(anchors.shape)}')
        pk = self.pack_targets(gt_bboxes, gt_labels)
        up = F.upload_many(pk, dev)
        out = F.anchor_targets(anchors.reshape(-1, 7), prm, up['boxes'], up['labels'], up['frame_offsets'], pk['frame_offsets'])
        if bbox_weights:
            out['bbox_weights'] = out['pos'].float()[..., None].expand(-1, -1, 7)
        return out

    def _get_targets_eager(self, anchors, gt_bboxes, gt_labels, bbox_weights=False):
        """``get_targets`` by the reference's loop over frames and assigners, in the dict form of the device path."""
        per_frame = [self.anchor_target_3d_single(anchors, b, None, l, None, num_classes=self.num_classes, sampling=self.sampling)
                     for b, l in zip(gt_bboxes, gt_labels)]
        stack = lambda k: torch.stack([r[k] for r in per_frame])
        weights = stack(3)
        out = dict(labels=stack(0), label_weights=stack(1), bbox_targets=stack(2), pos=(weights[..., 0] > 0).to(torch.uint8),
                   dir_targets=stack(4), dir_weights=stack(5),
                   pos_count=torch.tensor([r[6].numel() for r in per_frame], dtype=torch.int32, device=anchors.device))
        if bbox_weights:
            out['bbox_weights'] = weights
        return out

    def anchor_target_3d(self, anchor_list, gt_bboxes_list, input_metas, gt_bboxes_ignore_list=None, gt_labels_list=None,
                         label_channels=1, num_classes=1, sampling=True):
        """The eager targets (train_mixins.py:12-100): frame by frame, assigner by assigner."""
        num_imgs = len(input_metas)
        assert len(anchor_list) == num_imgs
        if isinstance(anchor_list[0][0], list):
            raise NotImplementedError('Anchor3DHead: per-class anchor lists (AlignedAnchor3DRangeGeneratorPerCls) are not supported')
        num_level_anchors = [a.view(-1, self.box_code_size).size(0) for a in anchor_list[0]]
        per_img = [levels[0] if len(levels) == 1 else torch.cat([a.reshape(-1, a.size(-1)) for a in levels]) for levels in anchor_list]
        gt_bboxes_ignore_list = gt_bboxes_ignore_list or [None] * num_imgs
        gt_labels_list = gt_labels_list or [None] * num_imgs
        (all_labels, all_label_weights, all_bbox_targets, all_bbox_weights, all_dir_targets, all_dir_weights, pos_inds_list,
         neg_inds_list) = multi_apply(self.anchor_target_3d_single, per_img, gt_bboxes_list, gt_bboxes_ignore_list, gt_labels_list,
                                      input_metas, label_channels=label_channels, num_classes=num_classes, sampling=sampling)
        num_total_pos = sum(max(inds.numel(), 1) for inds in pos_inds_list)
        num_total_neg = sum(max(inds.numel(), 1) for inds in neg_inds_list)
        return (images_to_levels(all_labels, num_level_anchors), images_to_levels(all_label_weights, num_level_anchors),
                images_to_levels(all_bbox_targets, num_level_anchors), images_to_levels(all_bbox_weights, num_level_anchors),
                images_to_levels(all_dir_targets, num_level_anchors), images_to_levels(all_dir_weights, num_level_anchors),
                num_total_pos, num_total_neg)

    def anchor_target_3d_single(self, anchors, gt_bboxes, gt_bboxes_ignore, gt_labels, input_meta, label_channels=1, num_classes=1,
                                sampling=True):
        """train_mixins.py:102-236 for anchors ``[1, H, W, n_sizes, n_rot, code]`` (a list of assigners: one per size) or flat."""
        if not isinstance(self.bbox_assigner, list):
            return self.anchor_target_single_assigner(self.bbox_assigner, anchors, gt_bboxes, gt_bboxes_ignore, gt_labels, input_meta,
                                                      num_classes, sampling)
        if anchors.dim() != 6:
            raise ValueError('Anchor3DHead: a list of assigners needs anchors [1, H, W, n_sizes, n_rot, code] (reshape_out=False)')
        feat_size = anchors.size(0) * anchors.size(1) * anchors.size(2)
        rot_angles, code = anchors.size(-2), anchors.size(-1)
        assert len(self.bbox_assigner) == anchors.size(-3)
        gt_tensor = gt_bboxes.tensor if hasattr(gt_bboxes, 'tensor') else gt_bboxes
        parts = []
        for i, assigner in enumerate(self.bbox_assigner):
            current = anchors[..., i, :, :].reshape(-1, code)
            if self.assign_per_class:
                sel = (gt_labels == i).to(gt_tensor.device)
                res = self.anchor_target_single_assigner(assigner, current, gt_tensor[sel], gt_bboxes_ignore, gt_labels[gt_labels == i],
                                                         input_meta, num_classes, sampling)
            else:
                res = self.anchor_target_single_assigner(assigner, current, gt_tensor, gt_bboxes_ignore, gt_labels, input_meta,
                                                         num_classes, sampling)
            parts.append(res)
        shape = lambda t, last=(): t.reshape(feat_size, 1, rot_angles, *last)
        cat = lambda k, dim, last=(): torch.cat([shape(p[k], last) for p in parts], dim=dim)
        return (cat(0, -2).reshape(-1), cat(1, -2).reshape(-1), cat(2, -3, (code, )).reshape(-1, code),
                cat(3, -3, (code, )).reshape(-1, code), cat(4, -2).reshape(-1), cat(5, -2).reshape(-1),
                torch.cat([p[6] for p in parts]).reshape(-1), torch.cat([p[7] for p in parts]).reshape(-1))

    def anchor_target_single_assigner(self, bbox_assigner, anchors, gt_bboxes, gt_bboxes_ignore, gt_labels, input_meta, num_classes=1,
                                      sampling=True):
        """train_mixins.py:238-316: assign, sample, encode the positives."""
        anchors = anchors.reshape(-1, anchors.size(-1))
        n = anchors.shape[0]
        bbox_targets, bbox_weights = torch.zeros_like(anchors), torch.zeros_like(anchors)
        dir_targets = anchors.new_zeros(n, dtype=torch.long)
        dir_weights = anchors.new_zeros(n, dtype=torch.float)
        labels = anchors.new_zeros(n, dtype=torch.long)
        label_weights = anchors.new_zeros(n, dtype=torch.float)
        if len(gt_bboxes) > 0:
            if not isinstance(gt_bboxes, torch.Tensor):
                gt_bboxes = gt_bboxes.tensor
            gt_bboxes = gt_bboxes.to(anchors.device)
            if gt_labels is not None:
                gt_labels = gt_labels.to(anchors.device)
            assign_result = bbox_assigner.assign(anchors, gt_bboxes, gt_bboxes_ignore, gt_labels)
            sampling_result = self.bbox_sampler.sample(assign_result, anchors, gt_bboxes)
            pos_inds, neg_inds = sampling_result.pos_inds, sampling_result.neg_inds
        else:
            pos_inds = anchors.new_zeros(0, dtype=torch.long)
            neg_inds = torch.arange(n, device=anchors.device)
        if gt_labels is not None:
            labels += num_classes
        if len(pos_inds) > 0:
            pos_bbox_targets = self.bbox_coder.encode(sampling_result.pos_bboxes, sampling_result.pos_gt_bboxes)
            bbox_targets[pos_inds, :] = pos_bbox_targets
            bbox_weights[pos_inds, :] = 1.0
            dir_targets[pos_inds] = get_direction_target(sampling_result.pos_bboxes, pos_bbox_targets, self.dir_offset,
                                                         self.dir_limit_offset, one_hot=False)
            dir_weights[pos_inds] = 1.0
            labels[pos_inds] = 1 if gt_labels is None else gt_labels[sampling_result.pos_assigned_gt_inds]
            pos_weight = _get(self.train_cfg, 'pos_weight', -1)
            label_weights[pos_inds] = 1.0 if pos_weight <= 0 else pos_weight
        if len(neg_inds) > 0:
            label_weights[neg_inds] = 1.0
        return labels, label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights, pos_inds, neg_inds

    # ------------------------------------------------------------------ losses
    @staticmethod
    def add_sin_difference(boxes1, boxes2):
        """anchor3d_head.py:280-302: sin(a - b) = sin a cos b - cos a sin b, as the pair (sin a cos b, cos a sin b)."""
        rad_pred = torch.sin(boxes1[..., 6:7]) * torch.cos(boxes2[..., 6:7])
        rad_tg = torch.cos(boxes1[..., 6:7]) * torch.sin(boxes2[..., 6:7])
        return (torch.cat([boxes1[..., :6], rad_pred, boxes1[..., 7:]], dim=-1),
                torch.cat([boxes2[..., :6], rad_tg, boxes2[..., 7:]], dim=-1))

    def loss_single(self, cls_score, bbox_pred, dir_cls_preds, labels, label_weights, bbox_targets, bbox_weights, dir_targets,
                    dir_weights, num_total_samples):
        """The eager losses of one level (anchor3d_head.py:194-278)."""
        if num_total_samples is None:
            num_total_samples = int(cls_score.shape[0])
        labels, label_weights = labels.reshape(-1), label_weights.reshape(-1)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.num_classes)
        loss_cls = self.loss_cls(cls_score, labels, label_weights, avg_factor=num_total_samples)
        code = self.box_code_size
        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, code)
        bbox_targets, bbox_weights = bbox_targets.reshape(-1, code), bbox_weights.reshape(-1, code)
        pos_inds = ((labels >= 0) & (labels < self.num_classes)).nonzero(as_tuple=False).reshape(-1)
        pos_bbox_pred, pos_bbox_targets, pos_bbox_weights = bbox_pred[pos_inds], bbox_targets[pos_inds], bbox_weights[pos_inds]
        loss_dir = None
        if self.use_direction_classifier:
            dir_cls_preds = dir_cls_preds.permute(0, 2, 3, 1).reshape(-1, 2)
            pos_dir_cls_preds = dir_cls_preds[pos_inds]
            pos_dir_targets, pos_dir_weights = dir_targets.reshape(-1)[pos_inds], dir_weights.reshape(-1)[pos_inds]
        if len(pos_inds) > 0:
            code_weight = _get(self.train_cfg, 'code_weight', None)
            if code_weight:
                pos_bbox_weights = pos_bbox_weights * bbox_weights.new_tensor(code_weight)
            if self.diff_rad_by_sin:
                pos_bbox_pred, pos_bbox_targets = self.add_sin_difference(pos_bbox_pred, pos_bbox_targets)
            loss_bbox = self.loss_bbox(pos_bbox_pred, pos_bbox_targets, pos_bbox_weights, avg_factor=num_total_samples)
            if self.use_direction_classifier:
                loss_dir = self.loss_dir(pos_dir_cls_preds, pos_dir_targets, pos_dir_weights, avg_factor=num_total_samples)
        else:
            loss_bbox = pos_bbox_pred.sum()
            if self.use_direction_classifier:
                loss_dir = pos_dir_cls_preds.sum()
        return loss_cls, loss_bbox, loss_dir

    def loss(self, cls_scores, bbox_preds, dir_cls_preds, gt_bboxes, gt_labels, input_metas, gt_bboxes_ignore=None):
        """-> ``dict(loss_cls, loss_bbox, loss_dir)``, each a list with one entry per level (anchor3d_head.py:304-374)."""
        featmap_sizes = [featmap.size()[-2:] for featmap in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        device = cls_scores[0].device
        if self._device_path(cls_scores):
            anchors = self.anchor_generator.grid_anchors(featmap_sizes, device=device)[0]
            targets = self.get_targets(anchors, gt_bboxes, gt_labels, device=device)
            lc, lb, ld = self.loss_cls, self.loss_bbox, self.loss_dir
            loss_cls, loss_bbox, loss_dir = F.anchor_losses(
                cls_scores[0], bbox_preds[0], dir_cls_preds[0] if self.use_direction_classifier else None, targets, self.num_anchors,
                self.num_classes, lc.gamma, lc.alpha, lb.beta, _get(self.train_cfg, 'code_weight', None),
                (lc.loss_weight, lb.loss_weight, ld.loss_weight), self.diff_rad_by_sin)
            return dict(loss_cls=[loss_cls], loss_bbox=[loss_bbox], loss_dir=[loss_dir if self.use_direction_classifier else None])
        anchor_list = self.get_anchors(featmap_sizes, input_metas, device=device)
        label_channels = self.cls_out_channels if self.use_sigmoid_cls else 1
        (labels_list, label_weights_list, bbox_targets_list, bbox_weights_list, dir_targets_list, dir_weights_list, num_total_pos,
         num_total_neg) = self.anchor_target_3d(anchor_list, gt_bboxes, input_metas, gt_bboxes_ignore_list=gt_bboxes_ignore,
                                                gt_labels_list=gt_labels, num_classes=self.num_classes,
                                                label_channels=label_channels, sampling=self.sampling)
        num_total_samples = num_total_pos + num_total_neg if self.sampling else num_total_pos
        losses_cls, losses_bbox, losses_dir = multi_apply(
            self.loss_single, cls_scores, bbox_preds, dir_cls_preds, labels_list, label_weights_list, bbox_targets_list,
            bbox_weights_list, dir_targets_list, dir_weights_list, num_total_samples=num_total_samples)
        return dict(loss_cls=losses_cls, loss_bbox=losses_bbox, loss_dir=losses_dir)

    # ------------------------------------------------------------------ inference
    def get_bboxes(self, cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg=None, rescale=False):
        """-> per frame ``(bboxes, scores, labels)`` (anchor3d_head.py:376-516)."""
        assert len(cls_scores) == len(bbox_preds) == len(dir_cls_preds)
        fast = self._get_bboxes_batched(cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg)
        if fast is not None:
            return fast
        num_levels = len(cls_scores)
        featmap_sizes = [cls_scores[i].shape[-2:] for i in range(num_levels)]
        mlvl_anchors = [a.reshape(-1, self.box_code_size)
                        for a in self.anchor_generator.grid_anchors(featmap_sizes, device=cls_scores[0].device)]
        result_list = []
        for img_id in range(len(input_metas)):
            pick = lambda maps: [maps[i][img_id].detach() if maps[i] is not None else None for i in range(num_levels)]
            result_list.append(self.get_bboxes_single(pick(cls_scores), pick(bbox_preds), pick(dir_cls_preds), mlvl_anchors,
                                                      input_metas[img_id], cfg, rescale))
        return result_list

    def _yaw_from_direction(self, yaw, dir_scores):
        """anchor3d_head.py:509-514: the decoded yaw folded into one half turn, plus the half turn the direction bit names."""
        dir_rot = limit_period(yaw - self.dir_offset, self.dir_limit_offset, np.pi)
        return dir_rot + self.dir_offset + np.pi * dir_scores.to(yaw.dtype)

    def get_bboxes_single(self, cls_scores, bbox_preds, dir_cls_preds, mlvl_anchors, input_meta, cfg=None, rescale=False):
        from .box3d import LiDARInstance3DBoxes
        cfg = self.test_cfg if cfg is None else cfg
        box_type = (input_meta.get('box_type_3d') if isinstance(input_meta, dict) else None) or LiDARInstance3DBoxes
        assert len(cls_scores) == len(bbox_preds) == len(mlvl_anchors)
        mlvl_bboxes, mlvl_scores, mlvl_dir_scores = [], [], []
        for cls_score, bbox_pred, dir_cls_pred, anchors in zip(cls_scores, bbox_preds, dir_cls_preds, mlvl_anchors):
            assert cls_score.size()[-2:] == bbox_pred.size()[-2:]
            if dir_cls_pred is not None:
                dir_cls_score = torch.max(dir_cls_pred.permute(1, 2, 0).reshape(-1, 2), dim=-1)[1]
            else:
                dir_cls_score = anchors.new_zeros(anchors.shape[0], dtype=torch.long)
            cls_score = cls_score.permute(1, 2, 0).reshape(-1, self.num_classes)
            scores = cls_score.sigmoid() if self.use_sigmoid_cls else cls_score.softmax(-1)
            bbox_pred = bbox_pred.permute(1, 2, 0).reshape(-1, self.box_code_size)
            nms_pre = _get(cfg, 'nms_pre', -1)
            if nms_pre > 0 and scores.shape[0] > nms_pre:
                max_scores = scores.max(dim=1)[0] if self.use_sigmoid_cls else scores[:, :-1].max(dim=1)[0]
                topk_inds = max_scores.topk(nms_pre)[1]
                anchors, bbox_pred, scores, dir_cls_score = anchors[topk_inds, :], bbox_pred[topk_inds, :], scores[topk_inds, :], dir_cls_score[topk_inds]
            mlvl_bboxes.append(self.bbox_coder.decode(anchors, bbox_pred))
            mlvl_scores.append(scores)
            mlvl_dir_scores.append(dir_cls_score)
        mlvl_bboxes = torch.cat(mlvl_bboxes)
        mlvl_bboxes_for_nms = ops.xywhr2xyxyr(box_type(mlvl_bboxes, box_dim=self.box_code_size).bev)
        mlvl_scores, mlvl_dir_scores = torch.cat(mlvl_scores), torch.cat(mlvl_dir_scores)
        if self.use_sigmoid_cls:        # a background column for box3d_multiclass_nms
            mlvl_scores = torch.cat([mlvl_scores, mlvl_scores.new_zeros(mlvl_scores.shape[0], 1)], dim=1)
        bboxes, scores, labels, dir_scores = ops.box3d_multiclass_nms(mlvl_bboxes, mlvl_bboxes_for_nms, mlvl_scores,
                                                                      _get(cfg, 'score_thr', 0), _get(cfg, 'max_num'), cfg,
                                                                      mlvl_dir_scores)
        if bboxes.shape[0] > 0:
            bboxes[..., 6] = self._yaw_from_direction(bboxes[..., 6], dir_scores)
        return box_type(bboxes, box_dim=self.box_code_size), scores, labels

    def _get_bboxes_batched(self, cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg=None):
        """All frames at once, one download: the per-frame maximum over the classes and ``topk(nms_pre)`` in torch on ``[B, A]``,
        ``functional.anchor_decode`` for the kept anchors of every frame, ``functional.multiclass_nms3d`` (scene = frame) on the
        xywhr boxes ``ops.nms_bev`` would form, ``functional.mono3d_collect`` for the ``max_num`` cut, one expression for the yaw.
        Taken only where it computes what the loop computes: one level, sigmoid scores, seven-entry boxes, rotated NMS, every
        frame's boxes ``LiDARInstance3DBoxes``, more anchors than ``nms_pre``; None otherwise."""
        from .box3d import LiDARInstance3DBoxes
        cfg = self.test_cfg if cfg is None else cfg
        nms_pre, max_num = _get(cfg, 'nms_pre', -1), _get(cfg, 'max_num')
        if not (DETECT_BATCHED and len(cls_scores) == 1 and cls_scores[0].is_cuda and self.use_sigmoid_cls and self.box_code_size == 7
                and len(self.anchor_generator.custom_values) == 0 and _get(cfg, 'use_rotate_nms') and max_num
                and self.num_classes <= F._lib.MULTICLASS_NMS_MAX_CLASSES
                and all(isinstance(m, dict) and m.get('box_type_3d') is LiDARInstance3DBoxes for m in input_metas)):
            return None
        cls_score, bbox_pred, dir_cls_pred = cls_scores[0].detach(), bbox_preds[0].detach(), dir_cls_preds[0]
        B, _, H, W = cls_score.shape
        A, nc = H * W * self.num_anchors, self.num_classes
        if not 0 < nms_pre < A or len(input_metas) != B:
            return None
        dev = cls_score.device
        anchors = self.anchor_generator.grid_anchors([(H, W)], device=dev)[0].reshape(-1, 7)
        scores = cls_score.permute(0, 2, 3, 1).reshape(B, A, nc).sigmoid()
        best = scores.max(dim=2)[0]
        topk_inds = torch.stack([best[b].topk(nms_pre)[1] for b in range(B)])      # per row on the loop's shape: the loop's order
        boxes, kept_scores, dir_bits = F.anchor_decode(topk_inds, anchors, scores, bbox_pred,
                                                       dir_cls_pred.detach() if dir_cls_pred is not None else None, self.num_anchors)
        xyxyr = ops.xywhr2xyxyr(boxes[:, [0, 1, 3, 4, 6]])
        zero = torch.zeros_like(xyxyr[:, 4])
        for_nms = torch.stack(((xyxyr[:, 0] + xyxyr[:, 2]) / 2, (xyxyr[:, 1] + xyxyr[:, 3]) / 2, zero, xyxyr[:, 2] - xyxyr[:, 0],
                               xyxyr[:, 3] - xyxyr[:, 1], zero, xyxyr[:, 4]), dim=-1)
        scene = F.const_tensor(np.repeat(np.arange(B, dtype=np.int64), nms_pre), dev, torch.int64)
        rows, classes, count = F.multiclass_nms3d(for_nms, kept_scores, scene, B, _get(cfg, 'score_thr', 0), _get(cfg, 'nms_thr'))
        packed, views_of = F.mono3d_collect(rows, classes, count, kept_scores, boxes, dir_bits, None, None, max_num)
        v = views_of(packed)
        v['boxes'][..., 6] = self._yaw_from_direction(v['boxes'][..., 6], v['dir'])     # (slots behind the count are cut below)
        host = views_of(packed.cpu())                                                   # the one wait of the batch
        out = []
        for b, n in enumerate(host['count'].tolist()):
            out.append((LiDARInstance3DBoxes(host['boxes'][b, :n], box_dim=7), host['scores'][b, :n].clone(),
                        host['labels'][b, :n].long()))
        return out
