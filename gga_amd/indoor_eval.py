"""Indoor mAP / mAR evaluation: ``mmdet3d.core.evaluation.indoor_eval`` on this repository's kernels.

Mirror of ``mmdet3d/core/evaluation/indoor_eval.py`` - the AP / AR table at IoU 0.25 and 0.5 every FCAF3D number is quoted in.
Same public names, arguments, ``ret_dict`` keys and key order:

* ``average_precision(recalls, precisions, mode='area' | '11points')``
* ``eval_map_recall(pred, gt, ovthresh)`` -> ``(recall, precision, ap)``, lists over thresholds of ``{label: array}``
* ``indoor_eval(gt_annos, dt_annos, metric, label2cat, logger, box_type_3d, box_mode_3d, device)`` -> ``ret_dict``

Where the work runs. The reference builds one box object per detection, calls the rotated-IoU native once per (class, frame) and
marks true positives in a Python double loop. Here the annos of all frames are concatenated once and sorted into (class, frame)
segments; ``gga_indoor_eval_match`` finds every detection's best ground truth (3D IoU of ``BaseInstance3DBoxes.overlaps`` in
float32, first maximum wins) and ``gga_indoor_eval_assign`` writes the TP / FP flags of all thresholds - one upload, three
launches, one download of the flags in class-major, descending-score order. Cumulative sums, recall, precision and AP stay
float64 numpy on the host as in the reference, so equal flags give bit-equal values. ``device='cpu'`` (or ``None`` on a machine
without a GPU) runs the same steps as whole-array numpy in float32: the partner of the device path in tests and A/B runs.

Score ties. Within a class the detections are ordered by a stable sort on descending score; equal scores keep the
reference's traversal order (frames ascending, detections in result order). The reference's ``np.argsort(-confidence)`` is
not stable, so for tied scores its order - and with it which of two tied detections takes a ground truth - is unspecified.

Reference edge cases, reproduced: a class with ground truths and no detections gets ``np.zeros(1)`` for recall, precision and AP;
a class met only among the detections has ``npos = 0``, hence NaN recall and AP at its keys (and NaN means).
The thresholds meet the float32 IoU as float32 values (torch compares a float32 tensor with a Python float in float32).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import functional as F
from ._lib import check

DEFAULT_DEVICE = 'cuda:0'
MAX_THRESHOLDS = 8          # GGA_INDOOR_EVAL_MAX_THRESHOLDS
_HOST_PAIR_CHUNK = 1 << 18


def average_precision(recalls, precisions, mode='area'):
    """indoor_eval.py:8-53, with its quirk that '11points' divides by 11 inside the loop over scales."""
    if recalls.ndim == 1:
        recalls = recalls[np.newaxis, :]
        precisions = precisions[np.newaxis, :]
    assert recalls.shape == precisions.shape
    assert recalls.ndim == 2
    num_scales = recalls.shape[0]
    ap = np.zeros(num_scales, dtype=np.float32)
    if mode == 'area':
        zeros = np.zeros((num_scales, 1), dtype=recalls.dtype)
        ones = np.ones((num_scales, 1), dtype=recalls.dtype)
        mrec = np.hstack((zeros, recalls, ones))
        mpre = np.hstack((zeros, precisions, zeros))
        mpre = np.maximum.accumulate(mpre[:, ::-1], axis=1)[:, ::-1]       # the running maximum from the right (NaN propagates alike)
        for i in range(num_scales):
            ind = np.where(mrec[i, 1:] != mrec[i, :-1])[0]
            ap[i] = np.sum((mrec[i, ind + 1] - mrec[i, ind]) * mpre[i, ind + 1])
    elif mode == '11points':
        for i in range(num_scales):
            for thr in np.arange(0, 1 + 1e-3, 0.1):
                precs = precisions[i, recalls[i, :] >= thr]
                prec = precs.max() if precs.size > 0 else 0
                ap[i] += prec
            ap /= 11
    else:
        raise ValueError('Unrecognized mode, only "area" and "11points" are supported')
    return ap


# ------------------------------------------------------------------------------------------------------------ host path
def _corners32(b, sx, sy):
    c, s = np.cos(b[:, 4]), np.sin(b[:, 4])
    hw, hh = b[:, 2] * np.float32(0.5), b[:, 3] * np.float32(0.5)
    cx, cy = b[:, 0] - sx, b[:, 1] - sy
    dx, dy = np.stack([-hw, hw, hw, -hw], 1), np.stack([-hh, -hh, hh, hh], 1)
    return np.stack([cx[:, None] + dx * c[:, None] - dy * s[:, None], cy[:, None] + dx * s[:, None] + dy * c[:, None]], 2)


def rotated_iou32(b1, b2):
    """Aligned rotated IoU of (x, y, w, h, angle) rows [P,5] in float32: ``rotated_iou`` of csrc/rotated_iou.h (the
    Sutherland-Hodgman clip of rectangle 1 by the half planes of rectangle 2) as whole-array numpy, pair by pair the same
    operations in the same order."""
    b1, b2 = np.ascontiguousarray(b1, np.float32).reshape(-1, 5), np.ascontiguousarray(b2, np.float32).reshape(-1, 5)
    n_pairs = len(b1)
    half = np.float32(0.5)
    rows = np.arange(n_pairs)
    with np.errstate(all='ignore'):
        a1, a2 = b1[:, 2] * b1[:, 3], b2[:, 2] * b2[:, 3]
        sx, sy = (b1[:, 0] + b2[:, 0]) * half, (b1[:, 1] + b2[:, 1]) * half
        q = _corners32(b2, sx, sy)
        poly = np.zeros((n_pairs, 10, 2), np.float32)
        poly[:, :4] = _corners32(b1, sx, sy)
        n = np.full(n_pairs, 4, np.int64)
        for e in range(4):
            a, ed = q[:, e], q[:, (e + 1) & 3] - q[:, e]
            tmp, m = np.zeros_like(poly), np.zeros(n_pairs, np.int64)
            for i in range(int(n.max(initial=0))):
                live = i < n
                p, r = poly[:, i], poly[rows, (i + 1) % np.maximum(n, 1)]
                dp = ed[:, 0] * (p[:, 1] - a[:, 1]) - ed[:, 1] * (p[:, 0] - a[:, 0])
                dr = ed[:, 0] * (r[:, 1] - a[:, 1]) - ed[:, 1] * (r[:, 0] - a[:, 0])
                keep = live & (dp >= 0)
                tmp[rows[keep], m[keep]] = p[keep]
                m += keep
                cross = live & ((dp >= 0) != (dr >= 0))
                t = dp / (dp - dr)
                tmp[rows[cross], m[cross]] = (p + t[:, None] * (r - p))[cross]
                m += cross
            poly, n = tmp, m
        area = np.zeros(n_pairs, np.float32)
        for i in range(int(n.max(initial=0))):
            p, r = poly[:, i], poly[rows, (i + 1) % np.maximum(n, 1)]
            area += np.where(i < n, p[:, 0] * r[:, 1] - p[:, 1] * r[:, 0], np.float32(0))
        inter = np.where(n >= 3, np.abs(area) * half, np.float32(0)).astype(np.float32)
        iou = inter / (a1 + a2 - inter)
        return np.where((a1 < np.float32(1e-14)) | (a2 < np.float32(1e-14)), np.float32(0), iou).astype(np.float32)


def iou3d_pairs32(d, g):
    """``BaseInstance3DBoxes.overlaps(mode='iou')`` of aligned rows [P,7] (x, y, z_bottom, dx, dy, dz, yaw) in float32."""
    d, g = np.ascontiguousarray(d, np.float32).reshape(-1, 7), np.ascontiguousarray(g, np.float32).reshape(-1, 7)
    with np.errstate(all='ignore'):
        ov_h = np.maximum(np.minimum(d[:, 2] + d[:, 5], g[:, 2] + g[:, 5]) - np.maximum(d[:, 2], g[:, 2]), np.float32(0))
        iou2d = rotated_iou32(d[:, [0, 1, 3, 4, 6]], g[:, [0, 1, 3, 4, 6]])
        a1, a2 = d[:, 3] * d[:, 4], g[:, 3] * g[:, 4]
        ov3d = iou2d * (a1 + a2) / (np.float32(1) + iou2d) * ov_h
        return (ov3d / np.maximum(a1 * d[:, 5] + a2 * g[:, 5] - ov3d, np.float32(1e-8))).astype(np.float32)


def match_host(det, det_off, gt, gt_off):
    """``gga_indoor_eval_match`` as numpy -> (iou_max [N] f32, jmax [N] i32)."""
    n = len(det)
    iou_max, jmax = np.full(n, -np.inf, np.float32), np.full(n, -1, np.int32)
    if n == 0:
        return iou_max, jmax
    seg = np.repeat(np.arange(len(det_off) - 1), np.diff(det_off))
    g0, cnt = gt_off[seg], (gt_off[seg + 1] - gt_off[seg])
    start = 0
    while start < n:
        stop = int(np.searchsorted(np.cumsum(cnt[start:]), _HOST_PAIR_CHUNK, side='right')) + start + 1
        stop = min(max(stop, start + 1), n)
        c = cnt[start:stop]
        has = np.flatnonzero(c > 0)
        if len(has):
            first = np.concatenate([[0], np.cumsum(c)[:-1]])
            pair_det = np.repeat(np.arange(start, stop), c)
            within = np.arange(int(c.sum())) - np.repeat(first, c)
            v = iou3d_pairs32(det[pair_det], gt[g0[pair_det] + within])
            best = np.fmax.reduceat(v, first[has])
            hit = np.where(v == np.repeat(best, c[has]), within, np.iinfo(np.int64).max)
            arg = np.minimum.reduceat(hit, first[has])
            ok = ~np.isnan(best)
            iou_max[start + has[ok]], jmax[start + has[ok]] = best[ok], arg[ok]
        start = stop
    return iou_max, jmax


def assign_host(iou_max, jmax, det_pos, det_off, gt_off, thresholds):
    """``gga_indoor_eval_assign`` as numpy -> tp [T, N] u8 indexed by det_pos."""
    n, n_gt = len(iou_max), int(gt_off[-1])
    tp = np.zeros((len(thresholds), n), np.uint8)
    if n == 0:
        return tp
    seg = np.repeat(np.arange(len(det_off) - 1), np.diff(det_off))
    g = np.where(jmax >= 0, gt_off[seg] + jmax, -1)
    for t, thr in enumerate(np.asarray(thresholds, np.float32)):
        cand = (g >= 0) & (iou_max > thr)
        claim = np.full(max(n_gt, 1), np.iinfo(np.int32).max, np.int64)
        np.minimum.at(claim, g[cand], det_pos[cand])
        tp[t, det_pos] = cand & (claim[np.maximum(g, 0)] == det_pos)
    return tp


# ---------------------------------------------------------------------------------------------------------- device path
def _section(sizes):
    offs, at = [], 0
    for s in sizes:
        offs.append(at)
        at += (int(s) + 7) // 8 * 8
    return offs, at


def match_and_flag(det, det_off, gt, gt_off, det_pos, thresholds, device=DEFAULT_DEVICE):
    """The raw call: host arrays in, host arrays out. det [N,7] / gt [M,7] f32 sorted into (class, frame) segments with offsets
    det_off / gt_off [S+1] i64, det_pos [N] i32 (class-major descending-score position of every detection), thresholds
    (any number; eight go into one launch) -> (iou_max [N] f32, jmax [N] i32, tp [T, N] u8 indexed by det_pos)."""
    det, gt = np.ascontiguousarray(det, np.float32).reshape(-1, 7), np.ascontiguousarray(gt, np.float32).reshape(-1, 7)
    det_off, gt_off = np.ascontiguousarray(det_off, np.int64), np.ascontiguousarray(gt_off, np.int64)
    det_pos = np.ascontiguousarray(det_pos, np.int32)
    thresholds = np.asarray(thresholds, np.float32).reshape(-1)
    n, m, s, n_thr = len(det), len(gt), len(det_off) - 1, len(thresholds)
    assert len(gt_off) == s + 1 and int(det_off[-1]) == n and int(gt_off[-1]) == m and len(det_pos) == n
    if device is None:
        device = DEFAULT_DEVICE if torch.cuda.is_available() else 'cpu'
    dev = torch.device(device)
    if dev.type != 'cuda':
        iou_max, jmax = match_host(det, det_off, gt, gt_off)
        return iou_max, jmax, assign_host(iou_max, jmax, det_pos, det_off, gt_off, thresholds)
    if n == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros((n_thr, 0), np.uint8)
    ins = [det, gt, det_off, gt_off, det_pos]
    in_off, in_bytes = _section([a.nbytes for a in ins])
    out_sizes = [n * 4, n * 4, n_thr * n]
    out_off, out_bytes = _section(out_sizes)
    host = np.zeros(max(in_bytes, 8), np.uint8)
    for a, o in zip(ins, in_off):
        host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    L = _lib.lib()
    with torch.cuda.device(dev):
        d_in = torch.from_numpy(host).to(dev)
        d_out = torch.zeros(max(out_bytes, 8), dtype=torch.uint8, device=dev)
        ws = torch.empty(int(L.gga_indoor_eval_workspace_bytes(m, MAX_THRESHOLDS)), dtype=torch.uint8, device=dev)
        pi = [C.c_void_p(d_in.data_ptr() + o) for o in in_off]
        po = [C.c_void_p(d_out.data_ptr() + o) for o in out_off]
        check(L.gga_indoor_eval_match(pi[0], pi[2], n, pi[1], pi[3], m, s, po[0], po[1], F._stream()),
              'gga_indoor_eval_match')
        for t0 in range(0, n_thr, MAX_THRESHOLDS):
            part = thresholds[t0:t0 + MAX_THRESHOLDS]
            thr = (C.c_float * MAX_THRESHOLDS)(*[float(v) for v in part])
            check(L.gga_indoor_eval_assign(po[0], po[1], pi[4], pi[2], n, pi[3], m, s, C.byref(thr), len(part),
                                           C.c_void_p(d_out.data_ptr() + out_off[2] + t0 * n), F._p(ws), ws.numel(), F._stream()),
                  'gga_indoor_eval_assign')
        back = d_out.cpu().numpy()
    cut = lambda k, dt: back[out_off[k]:out_off[k] + out_sizes[k]].view(dt)
    return cut(0, np.float32).copy(), cut(1, np.int32).copy(), cut(2, np.uint8).reshape(n_thr, n).copy()


# ------------------------------------------------------------------------------------------------------------ evaluation
class _Batch:
    """Detections and ground truths of all frames as columns, sorted into (class, frame) segments. ``labels``: the classes
    in the reference's key order (first met walking the frames, a frame's detections before its ground truths)."""

    def __init__(self, n_frames, dt_box, dt_score, dt_label, dt_frame, gt_box, gt_label, gt_frame):
        dt_label, gt_label = np.asarray(dt_label, np.int64).reshape(-1), np.asarray(gt_label, np.int64).reshape(-1)
        dt_frame, gt_frame = np.asarray(dt_frame, np.int64).reshape(-1), np.asarray(gt_frame, np.int64).reshape(-1)
        # the traversal order of the labels: (frame, detections before ground truths, position)
        walk_label = np.concatenate([dt_label, gt_label])
        walk_key = np.concatenate([dt_frame * 2, gt_frame * 2 + 1])
        walk_label = walk_label[np.argsort(walk_key, kind='stable')]
        uniq, first = np.unique(walk_label, return_index=True)
        self.labels = [int(v) for v in uniq[np.argsort(first)]]
        self.n_frames, n_cls = n_frames, len(self.labels)
        index_of = {v: k for k, v in enumerate(self.labels)}
        to_idx = lambda lab: np.array([index_of[int(v)] for v in lab], np.int64)
        dt_cls, gt_cls = to_idx(dt_label), to_idx(gt_label)
        n_seg = n_cls * n_frames
        dt_seg, gt_seg = dt_cls * n_frames + dt_frame, gt_cls * n_frames + gt_frame
        d_order, g_order = np.argsort(dt_seg, kind='stable'), np.argsort(gt_seg, kind='stable')
        self.det = np.ascontiguousarray(np.asarray(dt_box, np.float32).reshape(-1, 7)[d_order])
        self.gt = np.ascontiguousarray(np.asarray(gt_box, np.float32).reshape(-1, 7)[g_order])
        self.det_off, self.gt_off = np.zeros(n_seg + 1, np.int64), np.zeros(n_seg + 1, np.int64)
        np.cumsum(np.bincount(dt_seg, minlength=n_seg), out=self.det_off[1:])
        np.cumsum(np.bincount(gt_seg, minlength=n_seg), out=self.gt_off[1:])
        self.cls_start = self.det_off[::max(n_frames, 1)][:n_cls + 1] if n_frames else np.zeros(n_cls + 1, np.int64)
        self.npos = np.bincount(gt_cls, minlength=n_cls)
        self.has_pred = np.bincount(dt_cls, minlength=n_cls) > 0
        # the output position: class start + rank of the stable descending-score sort within the class
        score = np.asarray(dt_score).reshape(-1)[d_order]
        self.det_pos = np.zeros(len(score), np.int32)
        for c in range(n_cls):
            b, e = int(self.cls_start[c]), int(self.cls_start[c + 1])
            self.det_pos[b + np.argsort(-score[b:e], kind='stable')] = np.arange(b, e, dtype=np.int32)


def _evaluate(batch, ovthresh, device):
    """-> (recall, precision, ap) of ``eval_map_recall`` for a ``_Batch``."""
    iou_max, jmax, tp = match_and_flag(batch.det, batch.det_off, batch.gt, batch.gt_off, batch.det_pos, ovthresh, device)
    recall, precision, ap = ([{} for _ in ovthresh] for _ in range(3))
    for c, label in enumerate(batch.labels):
        b, e = int(batch.cls_start[c]), int(batch.cls_start[c + 1])
        for t in range(len(ovthresh)):
            if not batch.has_pred[c]:
                recall[t][label], precision[t][label], ap[t][label] = np.zeros(1), np.zeros(1), np.zeros(1)
                continue
            flags = tp[t, b:e].astype(np.float64)
            tps, fps = np.cumsum(flags), np.cumsum(1.0 - flags)
            with np.errstate(all='ignore'):
                rec = tps / float(batch.npos[c])
                prec = tps / np.maximum(tps + fps, np.finfo(np.float64).eps)
                recall[t][label], precision[t][label], ap[t][label] = rec, prec, average_precision(rec, prec)
    return recall, precision, ap


def eval_map_recall(pred, gt, ovthresh=None, device=None):
    """indoor_eval.py:165-202 with its data layout: ``pred[label][img_id]`` a list of (box, score), ``gt[label][img_id]`` a list
    of boxes, a box anything with a ``tensor`` of one row (x, y, z_bottom, dx, dy, dz, yaw). Classes come in ``gt``'s key order;
    one that is missing from ``pred`` gets zeros. -> (recall, precision, ap)."""
    row = lambda box: np.asarray(getattr(box, 'tensor', box), np.float32).reshape(7)
    frames = sorted({i for d in list(pred.values()) + list(gt.values()) for i in d})
    frame_of = {f: k for k, f in enumerate(frames)}
    dt, gts = [], []
    for label in gt:
        for img_id, boxes in gt[label].items():
            gts += [(row(b), label, frame_of[img_id]) for b in boxes]
        for img_id, items in pred.get(label, {}).items():
            dt += [(row(b), s, label, frame_of[img_id]) for b, s in items]
    col = lambda rows, k, dtype: np.array([r[k] for r in rows], dtype).reshape((-1, 7) if k == 0 else (-1,))
    batch = _Batch(len(frames), col(dt, 0, np.float32), col(dt, 1, np.float64), col(dt, 2, np.int64), col(dt, 3, np.int64),
                   col(gts, 0, np.float32), col(gts, 1, np.int64), col(gts, 2, np.int64))
    # the classes in gt's own key order (a class of gt without any box or detection included)
    rec, prec, ap = _evaluate(batch, ovthresh, device)
    zeros = lambda: np.zeros(1)
    order = lambda per_thr: [{label: d[label] if label in d and label in pred else zeros() for label in gt} for d in per_thr]
    return order(rec), order(prec), order(ap)


def _log(msg, logger):
    if logger is None:
        print(msg)
    elif logger == 'silent':
        pass
    elif callable(getattr(logger, 'info', None)):
        logger.info(msg)
    elif callable(logger):
        logger(msg)
    else:
        raise TypeError(f'logger should be None, "silent", a logger or a callable, got {type(logger)}')


def ascii_table(rows):
    """The grid terminaltables' ``AsciiTable`` draws with ``inner_footing_row_border``: a rule under the heading row and above
    the last row, cells left-justified with one space of padding (third-party layout, restated)."""
    width = [max(len(str(r[k])) for r in rows) for k in range(len(rows[0]))]
    rule = '+' + '+'.join('-' * (w + 2) for w in width) + '+'
    line = lambda r: '|' + '|'.join(' ' + str(v).ljust(w) + ' ' for v, w in zip(r, width)) + '|'
    out = [rule, line(rows[0]), rule] + [line(r) for r in rows[1:-1]]
    if len(rows) > 2:
        out.append(rule)
    if len(rows) > 1:
        out.append(line(rows[-1]))
    return '\n'.join(out + [rule])


def _columns(gt_annos, dt_annos, box_type_3d, box_mode_3d):
    from .fcaf3d import DepthInstance3DBoxes
    box_type_3d = box_type_3d or DepthInstance3DBoxes
    n_frames = len(dt_annos)
    dt_box, dt_score, dt_label, dt_count = [], [], [], np.zeros(n_frames, np.int64)
    gt_box, gt_label, gt_count = [], [], np.zeros(n_frames, np.int64)
    for f, (det, gta) in enumerate(zip(dt_annos, gt_annos)):
        k = len(det['labels_3d'])
        if k:
            dt_box.append(det['boxes_3d'].convert_to(box_mode_3d).tensor[:, :7].detach().to('cpu', torch.float32).numpy())
            dt_score.append(np.asarray(det['scores_3d'].detach().cpu().numpy()).reshape(-1))
            dt_label.append(np.asarray(det['labels_3d'].detach().cpu().numpy(), np.int64).reshape(-1))
            dt_count[f] = k
        if gta['gt_num'] != 0:
            raw = np.asarray(gta['gt_boxes_upright_depth'])
            gt_box.append(raw.reshape(-1, raw.shape[-1]))
            gt_label.append(np.asarray(gta['class'], np.int64).reshape(-1))
            gt_count[f] = len(gt_label[-1])
    cat = lambda parts, shape, dtype: np.concatenate(parts, 0) if parts else np.zeros(shape, dtype)
    gt_raw = cat(gt_box, (0, 7), np.float32)
    # box_type_3d(..., origin=(0.5, 0.5, 0.5)).convert_to(box_mode_3d) of the frames' boxes at once (row-wise arithmetic)
    gt7 = box_type_3d(gt_raw, box_dim=gt_raw.shape[-1], origin=(0.5, 0.5, 0.5)).convert_to(box_mode_3d).tensor[:, :7].numpy()
    return _Batch(n_frames, cat(dt_box, (0, 7), np.float32), cat(dt_score, (0,), np.float32), cat(dt_label, (0,), np.int64),
                  np.repeat(np.arange(n_frames), dt_count), gt7, cat(gt_label, (0,), np.int64), np.repeat(np.arange(n_frames), gt_count))


def indoor_eval(gt_annos, dt_annos, metric, label2cat, logger=None, box_type_3d=None, box_mode_3d=None, device=DEFAULT_DEVICE):
    """indoor_eval.py:205-309. ``gt_annos``: per frame ``gt_num``, ``gt_boxes_upright_depth`` (gravity centre), ``class``;
    ``dt_annos``: per frame ``boxes_3d`` / ``scores_3d`` / ``labels_3d``; ``metric``: the IoU thresholds. -> ``ret_dict`` with
    ``{cat}_AP_{thr:.2f}``, ``mAP_{thr:.2f}``, ``{cat}_rec_{thr:.2f}``, ``mAR_{thr:.2f}`` per threshold, in the reference's order;
    the table goes to ``logger``. ``device``: a GPU, or 'cpu' for the host path (None: the GPU when there is one)."""
    assert len(dt_annos) == len(gt_annos)
    batch = _columns(gt_annos, dt_annos, box_type_3d, box_mode_3d)
    rec, prec, ap = _evaluate(batch, list(metric), device)
    ret_dict = dict()
    header = ['classes']
    table_columns = [[label2cat[label] for label in ap[0].keys()] + ['Overall']]
    with np.errstate(all='ignore'):
        for i, iou_thresh in enumerate(metric):
            header.append(f'AP_{iou_thresh:.2f}')
            header.append(f'AR_{iou_thresh:.2f}')
            rec_list = []
            for label in ap[i].keys():
                ret_dict[f'{label2cat[label]}_AP_{iou_thresh:.2f}'] = float(ap[i][label][0])
            ret_dict[f'mAP_{iou_thresh:.2f}'] = float(np.mean(list(ap[i].values())))
            table_columns.append([float(v[0]) for v in ap[i].values()])
            table_columns[-1] += [ret_dict[f'mAP_{iou_thresh:.2f}']]
            table_columns[-1] = [f'{x:.4f}' for x in table_columns[-1]]
            for label in rec[i].keys():
                ret_dict[f'{label2cat[label]}_rec_{iou_thresh:.2f}'] = float(rec[i][label][-1])
                rec_list.append(rec[i][label][-1])
            ret_dict[f'mAR_{iou_thresh:.2f}'] = float(np.mean(rec_list))
            table_columns.append(list(map(float, rec_list)))
            table_columns[-1] += [ret_dict[f'mAR_{iou_thresh:.2f}']]
            table_columns[-1] = [f'{x:.4f}' for x in table_columns[-1]]
    _log('\n' + ascii_table([header] + list(zip(*table_columns))), logger)
    return ret_dict
