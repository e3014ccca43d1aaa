"""The yardstick of the anchor-head tests: a float32 CPU torch restatement of the reference's target loop and a float64
autograd restatement of its losses, written from

* mmdet3d/core/anchor/anchor_3d_generator.py:155-221, :255-340 (generators, ``torch.linspace`` construction)
* mmdet3d/core/bbox/structures/base_box3d.py:144-162, iou_calculators/iou3d_calculator.py:99-145 (nearest-BEV IoU; mmdet's
  ``bbox_overlaps`` with eps = 1e-6 on the union)
* mmdet's MaxIoUAssigner / PseudoSampler as published (pinned by tests/test_utils/test_assigners.py:13-34 of the reference)
* mmdet3d/core/bbox/coders/delta_xyzwhlr_bbox_coder.py:20-55 (encode), models/dense_heads/train_mixins.py:319-349 (direction
  target), :126-183 (per-assigner concatenation), :238-316 (targets of one assigner)
* mmdet3d/models/dense_heads/anchor3d_head.py:194-302 (``loss_single`` in the gather-positives form)

and the fixture the CPU and GPU tests share. Nothing here imports the code under test."""
import math

import numpy as np
import torch

PI = np.pi


# ----------------------------------------------------------------------------- generators
def ref_anchors(feature_size, ranges, sizes, rotations, aligned, scale=1):
    """-> [1, H, W, n_sizes, n_rot, 7]; one range per size."""
    H, W = feature_size
    per_size = []
    for rng, size in zip(ranges, sizes):
        r = torch.tensor(rng)
        if aligned:
            axes = []
            for lo, hi, n in ((r[2], r[5], 1), (r[1], r[4], H), (r[0], r[3], W)):
                c = torch.linspace(lo, hi, n + 1)
                c += (c[1] - c[0]) / 2
                axes.append(c[:n])
            z, y, x = axes
        else:
            z, y, x = torch.linspace(r[2], r[5], 1), torch.linspace(r[1], r[4], H), torch.linspace(r[0], r[3], W)
        s = torch.tensor(size).reshape(-1, 3) * scale
        rot = torch.tensor(rotations)
        gx, gy, gz, gr = torch.meshgrid(x, y, z, rot, indexing='ij')                     # [W, H, 1, R]
        cols = [g.unsqueeze(-2).repeat(1, 1, 1, s.shape[0], 1).unsqueeze(-1) for g in (gx, gy, gz, gr)]
        ss = s.reshape(1, 1, 1, -1, 1, 3).repeat(W, H, 1, 1, len(rotations), 1)
        cols.insert(3, ss)
        per_size.append(torch.cat(cols, dim=-1).permute(2, 1, 0, 3, 4, 5))
    return torch.cat(per_size, dim=-3)


# ----------------------------------------------------------------------------- IoU
def ref_limit_period(val, offset=0.5, period=PI):
    return val - torch.floor(val / period + offset) * period


def ref_nearest_bev(boxes):
    bev = boxes[:, [0, 1, 3, 4, 6]]
    normed = torch.abs(ref_limit_period(bev[:, -1], 0.5, PI))
    cond = (normed > PI / 4)[..., None]
    xywh = torch.where(cond, bev[:, [0, 1, 3, 2]], bev[:, :4])
    centers, dims = xywh[:, :2], xywh[:, 2:]
    return torch.cat([centers - dims / 2, centers + dims / 2], dim=-1)


def ref_overlaps(b1, b2, eps=1e-6):
    area1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    area2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    lt = torch.max(b1[:, None, :2], b2[None, :, :2])
    rb = torch.min(b1[:, None, 2:], b2[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = area1[:, None] + area2[None, :] - overlap
    union = torch.max(union, union.new_tensor([eps]))
    return overlap / union


def ref_iou(gt, anchors):
    return ref_overlaps(ref_nearest_bev(gt), ref_nearest_bev(anchors))


# ----------------------------------------------------------------------------- assigner
def ref_assign(overlaps, pos_iou_thr, neg_iou_thr, min_pos_iou):
    """overlaps [G, A] -> gt_inds [A]: -1 ignored, 0 negative, i + 1 ground truth i."""
    G, A = overlaps.shape
    gt_inds = torch.full((A, ), -1, dtype=torch.long)
    if G == 0:
        gt_inds[:] = 0
        return gt_inds
    max_iou, argmax = overlaps.max(dim=0)              # CPU torch: the lowest index among equal values
    gt_max = overlaps.max(dim=1)[0]
    gt_inds[(max_iou >= 0) & (max_iou < neg_iou_thr)] = 0
    pos = max_iou >= pos_iou_thr
    gt_inds[pos] = argmax[pos] + 1
    for i in range(G):
        if gt_max[i] >= min_pos_iou:
            gt_inds[overlaps[i] == gt_max[i]] = i + 1
    return gt_inds


def ref_encode(a, g):
    xa, ya, za, wa, la, ha, ra = torch.split(a, 1, dim=-1)
    xg, yg, zg, wg, lg, hg, rg = torch.split(g, 1, dim=-1)
    za = za + ha / 2
    zg = zg + hg / 2
    diagonal = torch.sqrt(la**2 + wa**2)
    return torch.cat([(xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / ha, torch.log(wg / wa), torch.log(lg / la),
                      torch.log(hg / ha), rg - ra], dim=-1)


def ref_direction(anchors, reg, dir_offset, dir_limit_offset):
    rot_gt = reg[..., 6] + anchors[..., 6]
    offset_rot = ref_limit_period(rot_gt - dir_offset, dir_limit_offset, 2 * PI)
    return torch.clamp(torch.floor(offset_rot / (2 * PI / 2)).long(), min=0, max=1)


def ref_targets_single_assigner(anchors, gt, gt_labels, thr, num_classes, pos_weight, dir_offset, dir_limit_offset):
    """train_mixins.py:238-316 with PseudoSampler. anchors [n, 7], gt [G, 7] -> dict of per-anchor targets + gt_inds + IoU."""
    n = anchors.shape[0]
    out = dict(labels=torch.full((n, ), num_classes, dtype=torch.long), label_weights=torch.zeros(n),
               bbox_targets=torch.zeros(n, 7), pos=torch.zeros(n, dtype=torch.uint8), dir_targets=torch.zeros(n, dtype=torch.long),
               dir_weights=torch.zeros(n), bbox_targets64=torch.zeros(n, 7, dtype=torch.float64))
    iou = ref_iou(gt, anchors) if len(gt) else torch.zeros(0, n)
    gt_inds = ref_assign(iou, *thr)
    pos = torch.nonzero(gt_inds > 0).squeeze(-1)
    neg = torch.nonzero(gt_inds == 0).squeeze(-1)
    if len(pos):
        which = gt_inds[pos] - 1
        enc = ref_encode(anchors[pos], gt[which])
        out['bbox_targets'][pos] = enc
        out['bbox_targets64'][pos] = ref_encode(anchors[pos].double(), gt[which].double())
        out['pos'][pos] = 1
        out['dir_targets'][pos] = ref_direction(anchors[pos], enc, dir_offset, dir_limit_offset)
        out['dir_weights'][pos] = 1.0
        out['labels'][pos] = gt_labels[which]
        out['label_weights'][pos] = 1.0 if pos_weight <= 0 else pos_weight
    out['label_weights'][neg] = 1.0
    out['gt_inds'], out['iou'] = gt_inds, iou
    return out


def ref_targets_frame(anchors, gt, gt_labels, thresholds, assign_per_class, num_classes, pos_weight=-1, dir_offset=-PI / 2,
                      dir_limit_offset=0):
    """train_mixins.py:126-183: anchors [1, H, W, S, R, 7], one assigner (thresholds[i]) per size -> the frame's targets in
    head order (h, w, size, rot), plus per assigner the raw result (``groups``)."""
    S, R = anchors.shape[-3], anchors.shape[-2]
    cells = anchors.shape[0] * anchors.shape[1] * anchors.shape[2]
    groups = []
    for i in range(S):
        cur = anchors[..., i, :, :].reshape(-1, 7)
        sel = gt_labels == i if assign_per_class else torch.ones_like(gt_labels, dtype=torch.bool)
        groups.append(ref_targets_single_assigner(cur, gt[sel], gt_labels[sel], thresholds[i], num_classes, pos_weight, dir_offset,
                                                  dir_limit_offset))
    out = {}
    for key in ('labels', 'label_weights', 'pos', 'dir_targets', 'dir_weights'):
        out[key] = torch.cat([g[key].reshape(cells, 1, R) for g in groups], dim=-2).reshape(-1)
    for key in ('bbox_targets', 'bbox_targets64'):
        out[key] = torch.cat([g[key].reshape(cells, 1, R, 7) for g in groups], dim=-3).reshape(-1, 7)
    out['groups'] = groups
    return out


def ref_targets_batch(anchors, gt_list, label_list, thresholds, assign_per_class, num_classes, **kw):
    frames = [ref_targets_frame(anchors, g, l, thresholds, assign_per_class, num_classes, **kw) for g, l in zip(gt_list, label_list)]
    out = {k: torch.stack([f[k] for f in frames]) for k in frames[0] if k != 'groups'}
    out['pos_count'] = torch.tensor([int(f['pos'].sum()) for f in frames], dtype=torch.int32)
    out['groups'] = [f['groups'] for f in frames]
    return out


# ----------------------------------------------------------------------------- losses (float64 autograd)
def ref_losses(cls_score, bbox_pred, dir_cls_pred, t, num_classes, gamma=2.0, alpha=0.25, beta=1.0 / 9.0, code_weight=None,
               loss_weights=(1.0, 2.0, 0.2), diff_rad_by_sin=True):
    """loss_single (anchor3d_head.py:194-278): maps [B, n_a * C | 7 | 2, H, W] float64, targets ``t`` (labels, label_weights,
    bbox_targets, dir_targets, dir_weights, pos_count). -> (loss_cls, loss_bbox, loss_dir)."""
    eps = float(torch.finfo(torch.float32).eps)
    avg = float(sum(max(int(c), 1) for c in t['pos_count']))
    labels, lw = t['labels'].reshape(-1), t['label_weights'].reshape(-1).double()
    x = cls_score.permute(0, 2, 3, 1).reshape(-1, num_classes)
    onehot = (labels[:, None] == torch.arange(num_classes)[None]).double()
    p = x.sigmoid()
    pt = (1 - p) * onehot + p * (1 - onehot)
    focal = torch.nn.functional.binary_cross_entropy_with_logits(x, onehot, reduction='none') * \
        (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt.pow(gamma)
    loss_cls = loss_weights[0] * (focal * lw[:, None]).sum() / (avg + eps)
    pos = ((labels >= 0) & (labels < num_classes)).nonzero().reshape(-1)
    pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 7)[pos]
    tgt = t['bbox_targets'].reshape(-1, 7).double()[pos]
    dirs = dir_cls_pred.permute(0, 2, 3, 1).reshape(-1, 2)[pos]
    if len(pos) == 0:
        return loss_cls, pred.sum(), dirs.sum()
    w = torch.ones(len(pos), 7, dtype=torch.float64)
    if code_weight:
        w = w * torch.tensor(code_weight, dtype=torch.float64)
    if diff_rad_by_sin:
        a = torch.sin(pred[:, 6:7]) * torch.cos(tgt[:, 6:7])
        b = torch.cos(pred[:, 6:7]) * torch.sin(tgt[:, 6:7])
        pred, tgt = torch.cat([pred[:, :6], a], dim=-1), torch.cat([tgt[:, :6], b], dim=-1)
    diff = torch.abs(pred - tgt)
    sl1 = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
    loss_bbox = loss_weights[1] * (sl1 * w).sum() / (avg + eps)
    ce = torch.nn.functional.cross_entropy(dirs, t['dir_targets'].reshape(-1)[pos], reduction='none')
    loss_dir = loss_weights[2] * (ce * t['dir_weights'].reshape(-1).double()[pos]).sum() / (avg + eps)
    return loss_cls, loss_bbox, loss_dir


# ----------------------------------------------------------------------------- the fixture
FEAT = (12, 12)
RANGES = [[0, -3.84, -0.6, 7.68, 3.84, -0.6], [0, -3.84, -0.6, 7.68, 3.84, -0.6], [0, -3.84, -1.78, 7.68, 3.84, -1.78]]
SIZES = [[0.8, 0.6, 1.73], [1.76, 0.6, 1.73], [3.9, 1.6, 1.56]]
ROTATIONS = [0, 1.57]
THRESHOLDS = [(0.5, 0.35, 0.35), (0.5, 0.35, 0.35), (0.6, 0.45, 0.45)]       # PointPillars: Pedestrian, Cyclist, Car
NUM_CLASSES = 3
PED, CYC, CAR = 0, 1, 2
GT_BOXES = [
    torch.tensor([[3.52, 0.32, -1.78, 3.9, 1.6, 1.56, 0.0], [5.12, -1.6, -1.7, 3.7, 1.55, 1.5, 0.1],
                  [1.6, -1.6, -0.6, 0.8, 0.6, 1.7, 1.2], [5.0, 2.0, -0.6, 1.7, 0.6, 1.7, 3.5]]),
    torch.zeros(0, 7),
    torch.tensor([[2.0, 1.0, -1.7, 4.0, 1.7, 1.5, 1.5], [2.0, 1.0, -1.7, 4.0, 1.7, 1.5, 1.5], [6.0, -3.0, -0.6, 0.2, 0.2, 1.0, 0.0]]),
]
GT_LABELS = [torch.tensor([CAR, CAR, PED, CYC]), torch.zeros(0, dtype=torch.long), torch.tensor([CAR, CAR, PED])]


def generator_cfg(aligned):
    return dict(type='AlignedAnchor3DRangeGenerator' if aligned else 'Anchor3DRangeGenerator', ranges=RANGES, sizes=SIZES,
                rotations=ROTATIONS, reshape_out=False)


def assigner_cfgs():
    return [dict(type='MaxIoUAssigner', iou_calculator=dict(type='BboxOverlapsNearest3D'), pos_iou_thr=p, neg_iou_thr=n,
                 min_pos_iou=m, ignore_iof_thr=-1) for p, n, m in THRESHOLDS]


def head_cfg(aligned=True, assign_per_class=True, train_cfg_extra=None, **kw):
    train_cfg = dict(assigner=assigner_cfgs(), allowed_border=0, pos_weight=-1, debug=False)
    train_cfg.update(train_cfg_extra or {})
    cfg = dict(type='Anchor3DHead', num_classes=NUM_CLASSES, in_channels=16, feat_channels=16, use_direction_classifier=True,
               assign_per_class=assign_per_class, anchor_generator=generator_cfg(aligned), diff_rad_by_sin=True,
               bbox_coder=dict(type='DeltaXYZWLHRBBoxCoder'),
               loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
               loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=2.0),
               loss_dir=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.2),
               train_cfg=train_cfg,
               test_cfg=dict(use_rotate_nms=True, nms_across_levels=False, nms_thr=0.01, score_thr=0.1, min_bbox_size=0, nms_pre=20,
                             max_num=5))
    cfg.update(kw)
    return cfg


def fixture_anchors(aligned=True):
    return ref_anchors(FEAT, RANGES, SIZES, ROTATIONS, aligned)


def synth_map(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def random_boxes(n, seed, x=(0.2, 7.4), y=(-3.6, 3.6)):
    """``n`` continuous random in-range boxes of mixed classes -> (boxes [n, 7], labels [n])."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand((n, 7), generator=g)
    labels = torch.randint(0, NUM_CLASSES, (n, ), generator=g)
    base = torch.tensor(SIZES)[labels]
    boxes = torch.stack([x[0] + u[:, 0] * (x[1] - x[0]), y[0] + u[:, 1] * (y[1] - y[0]), -1.8 + u[:, 2], base[:, 0] * (0.8 + 0.4 * u[:, 3]),
                         base[:, 1] * (0.8 + 0.4 * u[:, 4]), base[:, 2] * (0.8 + 0.4 * u[:, 5]), (u[:, 6] - 0.5) * 2 * math.pi], dim=1)
    return boxes, labels
