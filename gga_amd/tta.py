"""Test-time augmentation, box side: detections of the scaled / flipped views mapped back to the frame and merged
(mmdet3d/core/bbox/transforms.py:5-24, mmdet3d/core/post_processing/merge_augs.py:8-92). A few hundred boxes per frame on
the existing rotated-NMS kernel; the map side is ``functional.tta_merge_maps``."""
import torch

from . import ops
from .box3d import bbox3d2result


def _cfg(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def bbox3d_mapping_back(bboxes, scale_factor, flip_horizontal, flip_vertical):
    """Boxes of an augmented view in the coordinates of the frame: a copy with the flips undone (horizontal first), then
    scaled by ``1 / scale_factor``."""
    new_bboxes = bboxes.clone()
    if flip_horizontal:
        new_bboxes.flip('horizontal')
    if flip_vertical:
        new_bboxes.flip('vertical')
    new_bboxes.scale(1 / scale_factor)
    return new_bboxes


def merge_aug_bboxes_3d(aug_results, img_metas, test_cfg):
    """``aug_results``: one ``dict(boxes_3d, scores_3d, labels_3d)`` per scale group; ``img_metas``: per group the metas of its
    FIRST view (a list whose entry 0 carries ``pcd_scale_factor`` and the two flip flags). The boxes are mapped back,
    concatenated and run through BEV NMS class by class (ids ``0..max(label)``; ``test_cfg.use_rotate_nms`` picks the rotated
    or the axis-aligned form, ``test_cfg.nms_thr`` the threshold - the reference's per-class loop: offsetting the boxes by
    label instead would move coordinates and change bits), then sorted by score and cut to ``min(test_cfg.max_num, number
    of boxes before NMS)``. Returns the host-side result dict; no boxes in, the empty result out."""
    assert len(aug_results) == len(img_metas), \
        f'"aug_results" should have the same length as "img_metas", got {len(aug_results)} and {len(img_metas)}'
    recovered_bboxes, recovered_scores, recovered_labels = [], [], []
    for bboxes, img_info in zip(aug_results, img_metas):
        meta = img_info[0]
        recovered_scores.append(bboxes['scores_3d'])
        recovered_labels.append(bboxes['labels_3d'])
        recovered_bboxes.append(bbox3d_mapping_back(bboxes['boxes_3d'], meta['pcd_scale_factor'], meta['pcd_horizontal_flip'],
                                                    meta['pcd_vertical_flip']))
    aug_bboxes = type(recovered_bboxes[0]).cat(recovered_bboxes)
    aug_scores = torch.cat(recovered_scores, dim=0)
    aug_labels = torch.cat(recovered_labels, dim=0)
    if len(aug_labels) == 0:
        return bbox3d2result(aug_bboxes, aug_scores, aug_labels)
    aug_bboxes_for_nms = ops.xywhr2xyxyr(aug_bboxes.bev)
    nms_func = ops.nms_bev if _cfg(test_cfg, 'use_rotate_nms') else ops.nms_normal_bev
    nms_thr = _cfg(test_cfg, 'nms_thr')

    merged_bboxes, merged_scores, merged_labels = [], [], []
    for class_id in range(int(torch.max(aug_labels).item()) + 1):
        class_inds = aug_labels == class_id
        bboxes_nms_i = aug_bboxes_for_nms[class_inds, :]
        if len(bboxes_nms_i) == 0:
            continue
        bboxes_i, scores_i, labels_i = aug_bboxes[class_inds], aug_scores[class_inds], aug_labels[class_inds]
        selected = nms_func(bboxes_nms_i, scores_i, nms_thr)
        merged_bboxes.append(bboxes_i[selected])
        merged_scores.append(scores_i[selected])
        merged_labels.append(labels_i[selected])
    merged_bboxes = type(merged_bboxes[0]).cat(merged_bboxes)
    merged_scores = torch.cat(merged_scores, dim=0)
    merged_labels = torch.cat(merged_labels, dim=0)

    order = merged_scores.sort(0, descending=True)[1]
    order = order[:min(int(_cfg(test_cfg, 'max_num')), len(aug_bboxes))]
    return bbox3d2result(merged_bboxes[order], merged_scores[order], merged_labels[order])
