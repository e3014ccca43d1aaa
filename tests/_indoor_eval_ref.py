"""Helpers shared by the indoor evaluation tests and their golden generator: the float64 3D IoU of Depth boxes on the
independent polygon clip of ``_kitti_eval_ref``, and the packing of the cases of tests/golden/indoor_eval.npz."""
import numpy as np

import _kitti_eval_ref as K

THRESHOLDS = (0.25, 0.5)
# every best IoU of case B / C is this far from both thresholds and, unless it is exactly 0 (no overlap with any ground truth,
# only exact zeros to tie with), from its runner-up and from 0 (float64)
MARGIN = 1e-3


def iou3d64(d, g):
    """3D IoU of two Depth boxes (x, y, z_bottom, dx, dy, dz, yaw; yaw counter-clockwise) in float64."""
    d, g = np.asarray(d, np.float64), np.asarray(g, np.float64)
    inter = K.convex_intersection_area(K.bev_corners(d[0], d[1], d[3], d[4], -d[6]), K.bev_corners(g[0], g[1], g[3], g[4], -g[6]))
    ov = inter * max(0.0, min(d[2] + d[5], g[2] + g[5]) - max(d[2], g[2]))
    return ov / max(d[3] * d[4] * d[5] + g[3] * g[4] * g[5] - ov, 1e-8)


def bottom_centre(gravity_boxes):
    """gt_boxes_upright_depth (gravity centre) -> the bottom-centre rows the box structure holds, in float32 as it does."""
    b = np.asarray(gravity_boxes, np.float32).reshape(-1, 7).copy()
    b[:, 2] += b[:, 5] * np.float32(-0.5)
    return b


def best_two64(gts, dts):
    """Per detection (frames in order, detections in order): (best float64 IoU over the ground truths of its class in its
    frame, the index of that ground truth among them, the runner-up IoU); (-inf, -1, -inf) without any."""
    out = []
    for g, d in zip(gts, dts):
        gb = bottom_centre(g['gt_boxes_upright_depth']) if g['gt_num'] else np.zeros((0, 7), np.float32)
        gc = np.asarray(g['class']) if g['gt_num'] else np.zeros(0, np.int64)
        for box, label in zip(d['boxes'], d['labels']):
            v = np.array([iou3d64(box, q) for q in gb[gc == label]])
            if len(v) == 0:
                out.append((-np.inf, -1, -np.inf))
                continue
            j = int(np.argmax(v))
            out.append((float(v[j]), j, float(np.delete(v, j).max(initial=-np.inf))))
    return out


def pack_case(prefix, gts, dts, out):
    out[f'{prefix}.gt.count'] = np.array([g['gt_num'] for g in gts], np.int64)
    out[f'{prefix}.gt.boxes'] = np.concatenate([np.asarray(g['gt_boxes_upright_depth'], np.float32).reshape(-1, 7) for g in gts if g['gt_num']] +
                                               [np.zeros((0, 7), np.float32)])
    out[f'{prefix}.gt.class'] = np.concatenate([np.asarray(g['class'], np.int64) for g in gts if g['gt_num']] + [np.zeros(0, np.int64)])
    out[f'{prefix}.dt.count'] = np.array([len(d['labels']) for d in dts], np.int64)
    out[f'{prefix}.dt.boxes'] = np.concatenate([d['boxes'] for d in dts]).astype(np.float32)
    out[f'{prefix}.dt.scores'] = np.concatenate([d['scores'] for d in dts]).astype(np.float32)
    out[f'{prefix}.dt.labels'] = np.concatenate([d['labels'] for d in dts]).astype(np.int64)


def unpack_case(prefix, z):
    g_off = np.concatenate([[0], np.cumsum(z[f'{prefix}.gt.count'])])
    d_off = np.concatenate([[0], np.cumsum(z[f'{prefix}.dt.count'])])
    gts, dts = [], []
    for f in range(len(g_off) - 1):
        a, b = g_off[f], g_off[f + 1]
        gts.append(dict(gt_num=int(b - a), gt_boxes_upright_depth=z[f'{prefix}.gt.boxes'][a:b], **{'class': z[f'{prefix}.gt.class'][a:b]})
                   if b > a else dict(gt_num=0))
        a, b = d_off[f], d_off[f + 1]
        dts.append(dict(boxes=z[f'{prefix}.dt.boxes'][a:b], scores=z[f'{prefix}.dt.scores'][a:b], labels=z[f'{prefix}.dt.labels'][a:b]))
    return gts, dts


def as_results(dts, box_cls):
    """Array detections -> the result dicts a test run hands to ``evaluate`` (boxes by bottom centre)."""
    import torch
    return [dict(boxes_3d=box_cls(torch.from_numpy(np.ascontiguousarray(d['boxes'], np.float32)).reshape(-1, 7)),
                 scores_3d=torch.from_numpy(np.ascontiguousarray(d['scores'], np.float32)),
                 labels_3d=torch.from_numpy(np.ascontiguousarray(d['labels'], np.int64))) for d in dts]
