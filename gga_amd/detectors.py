"""``MVXTwoStageDetector_GGA`` and ``GGA`` detectors — registry names, constructor keys and
``forward_train`` signature of the reference (mmdet3d/models/detectors/
mvx_two_stage_gga.py:20-295, centerpoint_gga.py:10-86), plus the ``train_step`` /
``_parse_losses`` the reference inherits from mmdet's ``BaseDetector`` (third-party;
restated: the total is the sum of every entry whose key contains ``'loss'``).

LiDAR-only: the GGA configs build no image branch (extract_img_feat returns None).
"""
import os
from collections import OrderedDict

import torch
from torch import nn

from . import dense_heads
from .registry import (DETECTORS, build_backbone, build_head, build_middle_encoder, build_neck,
                       build_voxel_encoder)
from .voxel_layer import Voxelization


def _sub(cfg, key):
    if cfg is None:
        return None
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


class PreparedInputs:
    """The point-only front of a step, computed ahead of it (``prepare_inputs``): voxels,
    per-voxel counts, coordinates (carrying the sparse encoder's index plan when there is one)."""

    def __init__(self, voxels, num_points, coors, n_frames):
        self.voxels, self.num_points, self.coors, self.n_frames = voxels, num_points, coors, n_frames

    def __len__(self):
        return self.n_frames

    def tensors(self):
        yield from (t for t in (self.voxels, self.num_points, self.coors) if t is not None)
        for extra in (getattr(self.coors, 'num_valid', None),):
            if extra is not None:
                yield extra
        vmap = getattr(self.coors, 'voxel_map', None)       # dynamic voxelization: `voxels` are the points, one coors row each
        if vmap is not None:
            yield from vmap.tensors()
        plan = getattr(self.coors, 'index_plan', None)
        if plan is not None:
            yield from plan.tensors()


@DETECTORS.register_module()
class MVXTwoStageDetector_GGA(nn.Module):
    def __init__(self, pts_voxel_layer=None, pts_voxel_encoder=None, pts_middle_encoder=None,
                 pts_fusion_layer=None, img_backbone=None, pts_backbone=None, img_neck=None, pts_neck=None,
                 pts_bbox_head=None, img_roi_head=None, img_rpn_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None, init_cfg=None):
        super().__init__()
        for name, val in (('pts_fusion_layer', pts_fusion_layer), ('img_backbone', img_backbone),
                          ('img_neck', img_neck), ('img_roi_head', img_roi_head), ('img_rpn_head', img_rpn_head)):
            if val:
                raise NotImplementedError(f'{name}: the GGA configs are LiDAR-only; the image branch is out of scope')
        self.fp16_enabled = False
        if pts_voxel_layer:
            self.pts_voxel_layer = Voxelization(**pts_voxel_layer)
        if pts_voxel_encoder:
            self.pts_voxel_encoder = build_voxel_encoder(pts_voxel_encoder)
        if pts_middle_encoder:
            self.pts_middle_encoder = build_middle_encoder(pts_middle_encoder)
        if pts_backbone:
            self.pts_backbone = build_backbone(pts_backbone)
        if pts_neck is not None:
            self.pts_neck = build_neck(pts_neck)
        if pts_bbox_head:
            pts_bbox_head = dict(pts_bbox_head)
            pts_bbox_head.update(train_cfg=_sub(train_cfg, 'pts') if train_cfg else None)
            pts_bbox_head.update(test_cfg=_sub(test_cfg, 'pts') if test_cfg else None)
            self.pts_bbox_head = build_head(pts_bbox_head)
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg

    with_pts_bbox = property(lambda self: getattr(self, 'pts_bbox_head', None) is not None)
    with_pts_neck = property(lambda self: getattr(self, 'pts_neck', None) is not None)
    with_pts_backbone = property(lambda self: getattr(self, 'pts_backbone', None) is not None)
    with_voxel_encoder = property(lambda self: getattr(self, 'pts_voxel_encoder', None) is not None)
    with_middle_encoder = property(lambda self: getattr(self, 'pts_middle_encoder', None) is not None)
    with_img_backbone = property(lambda self: False)

    def extract_img_feat(self, img, img_metas):
        return None

    def extract_pts_feat(self, pts, img_feats, img_metas):
        if not self.with_pts_bbox:
            return None
        if isinstance(pts, PreparedInputs):
            voxels, num_points, coors = pts.voxels, pts.num_points, pts.coors
        else:
            voxels, num_points, coors = self.voxelize(pts)
        if self.dynamic_voxelization:
            # DynamicVoxelNet.extract_feat (dynamic_voxelnet.py:39-50): the encoder takes the points and their cells
            # and returns the voxels' features with the voxels' coordinates
            if self._dynamic_front_is_sync_free():
                voxel_features, coors = self.pts_voxel_encoder(voxels, coors, capacity=True)
            else:
                voxel_features, coors = self.pts_voxel_encoder(voxels, coors)
        else:
            voxel_features = self.pts_voxel_encoder(voxels, num_points, coors)
        batch_size = len(pts)      # the reference reads coors[-1, 0] + 1 back from the device
        x = self.pts_middle_encoder(voxel_features, coors, batch_size)
        x = self.pts_backbone(x)
        if self.with_pts_neck:
            x = self.pts_neck(x)
        return x

    def extract_feat(self, points, img, img_metas):
        img_feats = self.extract_img_feat(img, img_metas)
        pts_feats = self.extract_pts_feat(points, img_feats, img_metas)
        return (img_feats, pts_feats)

    @torch.no_grad()
    def voxelize(self, points):
        """list of [N_b, C] -> voxels [SM,P,C], num_points [SM], coors_batch [SM,4] (b,z,y,x):
        one batched HIP call instead of the per-frame loop + cat + pad of the reference."""
        # no host read-back when both consumers take the device-side pillar count (fused PFN + scatter):
        # the buffers then keep their capacity B * max_voxels and `coors.num_valid` carries the count
        if self.dynamic_voxelization:
            # DynamicVoxelNet.voxelize (dynamic_voxelnet.py:52-72): -> points [SN,C], None, coors [SN,4] per point, which
            # carry the sorted point-to-voxel map of the batch
            cat, coors = self.pts_voxel_layer.forward_batch(points)
            return cat, None, coors
        sync = not (getattr(self.pts_voxel_encoder, 'accepts_num_valid', False)
                    and getattr(self.pts_middle_encoder, 'accepts_num_valid', False))
        voxels, num_points, coors, _ = self.pts_voxel_layer.forward_batch(points, sync=sync)
        return voxels, num_points, coors

    def _dynamic_front_is_sync_free(self):
        enc = self.pts_voxel_encoder
        return (getattr(enc, 'accepts_num_valid', False) and getattr(self.pts_middle_encoder, 'accepts_num_valid', False)
                and hasattr(enc, 'fusable_config') and enc.fusable_config())

    dynamic_voxelization = property(lambda self: getattr(getattr(self, 'pts_voxel_layer', None), 'dynamic', False))

    @property
    def front_reads_counts(self):
        """True when the point-only front of a step reads voxel / site counts back to the host
        (the sparse-conv trunk: data-dependent level sizes); the PointPillars front does not."""
        if self.dynamic_voxelization:
            # the fused pillar front hands capacity-sized rows and a device-side count on; every other dynamic encoder sizes
            # its outputs by the voxel count (one read per batch)
            return not self._dynamic_front_is_sync_free()
        return not (getattr(self.pts_voxel_encoder, 'accepts_num_valid', False)
                    and getattr(self.pts_middle_encoder, 'accepts_num_valid', False))

    @torch.no_grad()
    def prepare_inputs(self, points):
        """Voxelize ``points`` and build the sparse encoder's levels / rule books: everything of a
        step that depends on the points alone and nothing on the weights. ``forward_train`` accepts
        the result in place of ``points``; ``train.Runner`` calls this for the NEXT batch on a side
        stream, where its host reads of the counts wait only for these few kernels."""
        if isinstance(points, PreparedInputs):
            return points
        voxels, num_points, coors = self.voxelize(points)
        if self.dynamic_voxelization:
            if self.front_reads_counts:
                coors.voxel_map.host_counts()   # the one read-back of the dynamic front, taken here (on the side stream)
            return PreparedInputs(voxels, None, coors, len(points))
        if hasattr(self.pts_middle_encoder, 'build_indices'):
            coors = self.pts_middle_encoder.build_indices(coors, len(points))
        return PreparedInputs(voxels, num_points, coors, len(points))

    def forward_train(self, points=None, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None,
                      GGA_boxes_img=None, GGA_lidar2img=None, GGA_init_pseudo_labels=None, GGA_bdry_masks=None,
                      GGA_in_box_points=None, gt_labels=None, gt_bboxes=None, img=None, proposals=None,
                      gt_bboxes_ignore=None):
        img_feats, pts_feats = self.extract_feat(points, img=img, img_metas=img_metas)
        losses = dict()
        if pts_feats:
            losses.update(self.forward_pts_train(pts_feats, gt_bboxes_3d, gt_labels_3d, GGA_boxes_img,
                                                 GGA_lidar2img, GGA_init_pseudo_labels, GGA_bdry_masks,
                                                 GGA_in_box_points, img_metas, gt_bboxes_ignore))
        return losses

    def forward_pts_train(self, pts_feats, gt_bboxes_3d, gt_labels_3d, GGA_boxes_img, GGA_lidar2img,
                          GGA_init_pseudo_labels, GGA_bdry_masks, GGA_in_box_points, img_metas,
                          gt_bboxes_ignore=None):
        head = self.pts_bbox_head
        if dense_heads.FWD_CELLS and isinstance(head, dense_heads.CenterHead_GGA):
            # targets first (they depend on the ground truth alone; the SRL draws come from the CPU generator in the same
            # order), so that the head computes its regression maps only where the loss gathers them
            targets = head.get_targets(gt_bboxes_3d, gt_labels_3d, GGA_boxes_img, GGA_lidar2img, GGA_init_pseudo_labels,
                                       GGA_bdry_masks, GGA_in_box_points, img_metas, device=pts_feats[0].device)
            outs = head(pts_feats, cells=targets[2])
            return head.loss_from_targets(outs, *targets)
        outs = head(pts_feats)
        return self.pts_bbox_head.loss(gt_bboxes_3d, gt_labels_3d, outs, GGA_boxes_img, GGA_lidar2img,
                                       GGA_init_pseudo_labels, GGA_bdry_masks, GGA_in_box_points, img_metas)

    def forward(self, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(**kwargs)
        return self.forward_test(**kwargs)

    # ---- inference (mvx_two_stage_gga.py:407-423, centerpoint_gga.py:88-97, detectors/base.py:16-45)
    def forward_test(self, points, img_metas, img=None, **kwargs):
        for var, name in [(points, 'points'), (img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError(f'{name} must be a list, but got {type(var)}')
        if len(points) != len(img_metas):
            raise ValueError(f'num of augmentations ({len(points)}) != num of image meta ({len(img_metas)})')
        if len(points) == 1:
            return self.simple_test(points[0], img_metas[0], None if img is None else img[0], **kwargs)
        return self.aug_test(points, img_metas, img, **kwargs)

    @torch.no_grad()
    def simple_test_pts(self, x, img_metas, rescale=False):
        outs = self.pts_bbox_head(x)
        return self._results_to_host(self.pts_bbox_head.get_bboxes(outs, img_metas, rescale=rescale))

    @staticmethod
    def _results_to_host(bbox_list):
        from .box3d import bbox3d2result
        packed = getattr(bbox_list, 'packed', None)
        if packed is not None:
            # the batched post-processing left one set of batch tensors: three copies to the host for the whole batch
            # instead of three per frame (each a synchronisation); the per-frame results are host-side views
            boxes, scores, labels, counts = packed
            boxes, scores, labels = boxes.cpu(), scores.cpu(), labels.cpu()
            return [dict(boxes_3d=type(b)(boxes[i, :n], b.box_dim, with_yaw=b.with_yaw), scores_3d=scores[i, :n], labels_3d=labels[i, :n])
                    for i, (n, (b, _, _)) in enumerate(zip(counts, bbox_list))]
        return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in bbox_list]

    @torch.no_grad()
    def simple_test(self, points, img_metas, img=None, rescale=False):
        _, pts_feats = self.extract_feat(points, img=img, img_metas=img_metas)
        bbox_list = [dict() for _ in range(len(img_metas))]
        if pts_feats and self.with_pts_bbox:
            for result_dict, pts_bbox in zip(bbox_list, self.simple_test_pts(pts_feats, img_metas, rescale=rescale)):
                result_dict['pts_bbox'] = pts_bbox
        return bbox_list

    # ---- test-time augmentation (centerpoint_gga.py:99-208, with samples_per_gpu > 1) ---------------------------------
    # The V views of the F frames of a batch go through the front, the trunk and the head as ONE batch of V * F point clouds,
    # view-major (view v of frame f is row v * F + f). One launch then undoes the flips of every task's maps and averages them
    # per scale group (functional.tta_merge_maps), the detections of the S * F merged "frames" are decoded at once, and for
    # S > 1 the boxes of a frame's scale groups are mapped back and merged (tta.merge_aug_bboxes_3d). GGA_TTA_MERGE=0: the
    # maps are merged by the reference's per-view eager sequence instead (the fallback, and what the tests compare against).
    TTA_MERGE = os.environ.get('GGA_TTA_MERGE', '1') != '0'

    @torch.no_grad()
    def aug_test(self, points, img_metas, img=None, rescale=False):
        n_frames = len(points[0])
        for view, metas in zip(points, img_metas):
            if len(view) != n_frames or len(metas) != n_frames:
                raise ValueError('aug_test: every view must hold the same frames (points[v][f], img_metas[v][f])')
        self._tta_views(img_metas)        # a set of views that cannot be merged is refused before the trunk runs
        flat = [p for view in points for p in view]
        _, pts_feats = self.extract_feat(flat, img=None, img_metas=[m for metas in img_metas for m in metas])
        bbox_list = [dict() for _ in range(n_frames)]
        if pts_feats and self.with_pts_bbox:
            for result_dict, pts_bbox in zip(bbox_list, self.aug_test_pts(pts_feats, img_metas, rescale=rescale)):
                result_dict['pts_bbox'] = pts_bbox
        return bbox_list

    def _tta_views(self, img_metas):
        """-> (group [V], hflip [V], vflip [V], first view of every group): scale groups in order of first appearance of
        ``pcd_scale_factor``. A view's frames share one augmentation (the wrapper's loop does not depend on the frame)."""
        scales, group, hflip, vflip, first = [], [], [], [], []
        for v, metas in enumerate(img_metas):
            key = lambda m: (m['pcd_scale_factor'], bool(m.get('pcd_horizontal_flip', False)), bool(m.get('pcd_vertical_flip', False)))
            scale, h, vf = key(metas[0])
            if any(key(m) != (scale, h, vf) for m in metas[1:]):
                raise ValueError(f'aug_test: the frames of view {v} carry different augmentations')
            if scale not in scales:
                scales.append(scale)
                first.append(v)
            group.append(scales.index(scale))
            hflip.append(h)
            vflip.append(vf)
        per_scale = [group.count(s) for s in range(len(scales))]
        if len(set(per_scale)) != 1:
            raise ValueError(f'aug_test: the scale groups {scales} have {per_scale} views; every scale needs the same number')
        pcr = getattr(getattr(self, 'pts_voxel_layer', None), 'point_cloud_range', None)
        if pcr is not None:
            for flags, axis, lo, hi, name in ((hflip, 'y', pcr[1], pcr[4], 'horizontal'), (vflip, 'x', pcr[0], pcr[3], 'vertical')):
                if any(flags) and lo != -hi:
                    raise ValueError(f'aug_test: a {name} flip mirrors the {axis} axis, but point_cloud_range spans '
                                     f'[{lo}, {hi}] on {axis}: not symmetric about 0, mirroring the head maps cannot undo it')
        return group, hflip, vflip, first

    @staticmethod
    def _tta_merge_views_eager(views, group, hflip, vflip):
        """centerpoint_gga.py:123-182 on ``views[v][f]`` = the head's output of view v of frame f at batch 1: flip, channel
        fix-up, ``+=`` into the group's first view, ``/=`` views per scale; the groups' frames then form the batch
        ``get_bboxes`` takes."""
        n_groups, n_frames = max(group) + 1, len(views[0])
        sums = {}
        for v, frames in enumerate(views):
            for f, view in enumerate(frames):
                view = [[dict(task[0])] for task in view]
                for task in view:
                    for key in task[0].keys():
                        if hflip[v]:
                            task[0][key] = torch.flip(task[0][key], dims=[2])
                            if key == 'reg':
                                task[0][key][:, 1, ...] = 1 - task[0][key][:, 1, ...]
                            elif key == 'rot':
                                task[0][key][:, 0, ...] = -task[0][key][:, 0, ...]
                            elif key == 'vel':
                                task[0][key][:, 1, ...] = -task[0][key][:, 1, ...]
                        if vflip[v]:
                            task[0][key] = torch.flip(task[0][key], dims=[3])
                            if key == 'reg':
                                task[0][key][:, 0, ...] = 1 - task[0][key][:, 0, ...]
                            elif key == 'rot':
                                task[0][key][:, 1, ...] = -task[0][key][:, 1, ...]
                            elif key == 'vel':
                                task[0][key][:, 0, ...] = -task[0][key][:, 0, ...]
                slot = (group[v], f)
                if slot not in sums:        # (a copy: an unflipped first view is still the head's own tensor)
                    sums[slot] = [[{key: x.clone() for key, x in task[0].items()}] for task in view]
                else:
                    for acc, task in zip(sums[slot], view):
                        for key in task[0].keys():
                            acc[0][key] += task[0][key]
        for acc_tasks in sums.values():
            for acc in acc_tasks:
                for key in acc[0].keys():
                    acc[0][key] /= len(group) / n_groups
        first = views[0][0]
        return [[{key: torch.cat([sums[(s, f)][t][0][key] for s in range(n_groups) for f in range(n_frames)])
                  for key in first[t][0].keys()}] for t in range(len(first))]

    @classmethod
    def _tta_merge_maps_eager(cls, outs, group, hflip, vflip, n_frames):
        """The eager merge on the view-major batch: every view of every frame as its [1, C, H, W] slice."""
        views = [[[[{key: x[v * n_frames + f:v * n_frames + f + 1] for key, x in task[0].items()}] for task in outs]
                  for f in range(n_frames)] for v in range(len(group))]
        return cls._tta_merge_views_eager(views, group, hflip, vflip)

    @torch.no_grad()
    def aug_test_pts(self, feats, img_metas, rescale=False):
        from . import functional as F
        from .tta import merge_aug_bboxes_3d
        head = self.pts_bbox_head
        n_frames = len(img_metas[0])
        group, hflip, vflip, first = self._tta_views(img_metas)
        n_groups = len(first)
        outs = head(feats)
        merge = F.tta_merge_maps if self.TTA_MERGE else self._tta_merge_maps_eager
        merged = merge(outs, group, hflip, vflip, n_frames)
        bbox_list = head.get_bboxes(merged, [img_metas[v][f] for v in first for f in range(n_frames)], rescale=rescale)
        if n_groups == 1:
            return self._results_to_host(bbox_list)
        # scales are merged box by box: per frame, the detections of its S groups with the metas of each group's first view
        return [merge_aug_bboxes_3d([dict(zip(('boxes_3d', 'scores_3d', 'labels_3d'), bbox_list[s * n_frames + f]))
                                     for s in range(n_groups)], [[img_metas[v][f]] for v in first], head.test_cfg)
                for f in range(n_frames)]

    # ---- mmdet BaseDetector.train_step / _parse_losses (restated) -----------------
    def _parse_losses(self, losses):
        log_vars = OrderedDict()
        for name, value in losses.items():
            # (the mean of a 0-d tensor is the tensor: no reduce launch - and no division in backward - for the 18 scalar terms of a
            # CenterPoint-style head)
            if isinstance(value, torch.Tensor):
                log_vars[name] = value.mean() if value.dim() else value
            elif isinstance(value, list):
                log_vars[name] = sum(v.mean() if v.dim() else v for v in value)
            else:
                raise TypeError(f'{name} is not a tensor or list of tensors')
        pal = getattr(getattr(self, 'pts_bbox_head', None), 'pal_backprop', False)
        terms = [v for k, v in log_vars.items() if 'loss' in k or (pal and 'distance' in k)]
        loss = torch.stack(terms).sum()
        log_vars['loss'] = loss
        return loss, log_vars        # values stay on the device: no .item() sync per step

    def train_step(self, data, optimizer=None):
        losses = self(**data)
        loss, log_vars = self._parse_losses(losses)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data['img_metas']))


@DETECTORS.register_module()
class GGA(MVXTwoStageDetector_GGA):
    """The GGA detector (centerpoint_gga.py:10-86): CenterPoint-style single stage on top of
    ``MVXTwoStageDetector_GGA``."""

    @property
    def with_velocity(self):
        return self.pts_bbox_head is not None and self.pts_bbox_head.with_velocity


@DETECTORS.register_module()
class CenterPoint(MVXTwoStageDetector_GGA):
    """The supervised CenterPoint detector (mmdet3d/models/detectors/centerpoint.py:9-60): the machinery above - voxelise,
    encoders, trunk, ``prepare_inputs``, the test paths and TTA - trained on 3D boxes through ``dense_heads.CenterHead``."""

    def forward_train(self, points=None, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None, gt_labels=None, gt_bboxes=None,
                      img=None, proposals=None, gt_bboxes_ignore=None):
        img_feats, pts_feats = self.extract_feat(points, img=img, img_metas=img_metas)
        losses = dict()
        if pts_feats:
            losses.update(self.forward_pts_train(pts_feats, gt_bboxes_3d, gt_labels_3d, img_metas, gt_bboxes_ignore))
        return losses

    def forward_pts_train(self, pts_feats, gt_bboxes_3d, gt_labels_3d, img_metas, gt_bboxes_ignore=None):
        head = self.pts_bbox_head
        if dense_heads.FWD_CELLS and isinstance(head, dense_heads.CenterHead):
            # targets first (they depend on the ground truth alone), so that the head computes its regression maps only
            # where the loss gathers them
            targets = head.get_targets(gt_bboxes_3d, gt_labels_3d, device=pts_feats[0].device)
            outs = head(pts_feats, cells=targets[2])
            return head.loss_from_targets(outs, *targets)
        outs = head(pts_feats)
        return head.loss(gt_bboxes_3d, gt_labels_3d, outs)

    @property
    def with_velocity(self):
        return self.pts_bbox_head is not None and self.pts_bbox_head.with_velocity


def _alias(name):
    return property(lambda self: self._modules.get(name))


@DETECTORS.register_module()
class VoxelNet(MVXTwoStageDetector_GGA):
    """The single-stage LiDAR detector of SECOND and PointPillars (mmdet3d/models/detectors/voxelnet.py:14-130,
    single_stage.py:8-70): ``voxel_layer`` -> ``voxel_encoder`` -> ``middle_encoder`` -> ``backbone`` -> ``neck`` -> ``bbox_head``.
    The modules are registered under those names, so the parameters are ``voxel_encoder.*``, ``middle_encoder.*``, ``backbone.*``,
    ``neck.*`` and ``bbox_head.*`` as in the reference; the ``pts_*`` names of ``MVXTwoStageDetector_GGA`` are read-only aliases
    of them, through which its machinery (batched voxelisation, ``prepare_inputs``, the trunk, results to the host) runs
    unchanged. A frame's result is the plain ``dict(boxes_3d, scores_3d, labels_3d)``."""
    pts_voxel_layer, pts_voxel_encoder, pts_middle_encoder = _alias('voxel_layer'), _alias('voxel_encoder'), _alias('middle_encoder')
    pts_backbone, pts_neck, pts_bbox_head = _alias('backbone'), _alias('neck'), _alias('bbox_head')

    def __init__(self, voxel_layer, voxel_encoder, middle_encoder, backbone, neck=None, bbox_head=None, train_cfg=None,
                 test_cfg=None, init_cfg=None, pretrained=None):
        nn.Module.__init__(self)
        self.fp16_enabled = False
        self.voxel_layer = Voxelization(**voxel_layer)
        self.voxel_encoder = build_voxel_encoder(voxel_encoder)
        self.middle_encoder = build_middle_encoder(middle_encoder)
        self.backbone = build_backbone(backbone)
        if neck is not None:
            self.neck = build_neck(neck)
        if bbox_head is not None:
            self.bbox_head = build_head(dict(bbox_head, train_cfg=train_cfg, test_cfg=test_cfg))
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    def extract_feat(self, points, img_metas=None):
        """-> the neck's feature maps (voxelnet.py:37-48)."""
        return self.extract_pts_feat(points, None, img_metas)

    def forward_train(self, points, img_metas, gt_bboxes_3d, gt_labels_3d, gt_bboxes_ignore=None, **kwargs):
        x = self.extract_feat(points, img_metas)
        outs = self.bbox_head(x)
        return self.bbox_head.loss(*outs, gt_bboxes_3d, gt_labels_3d, img_metas, gt_bboxes_ignore=gt_bboxes_ignore)

    @torch.no_grad()
    def simple_test(self, points, img_metas, imgs=None, rescale=False):
        from .box3d import bbox3d2result
        x = self.extract_feat(points, img_metas)
        outs = self.bbox_head(x)
        bbox_list = self.bbox_head.get_bboxes(*outs, img_metas, rescale=rescale)
        return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in bbox_list]

    def aug_test(self, points, img_metas, imgs=None, rescale=False):
        raise NotImplementedError('VoxelNet.aug_test: test-time augmentation of the anchor head is not supported')
