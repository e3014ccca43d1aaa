"""KITTI AP evaluation (bbox / BEV / 3D / AOS): ``mmdet3d.core.evaluation.kitti_eval`` on this repository's kernels.

Mirror of ``mmdet3d/core/evaluation/kitti_utils/eval.py`` (+ ``rotate_iou.py``), the call that follows the pseudo-label
matching in ``KittiDataset_GGA_match.evaluate`` (kitti_dataset_GGA_match.py:418-456). Same public names, arguments, result
text and ``KITTI/...`` keys:

* ``kitti_eval(gt_annos, dt_annos, current_classes, eval_types=['bbox', 'bev', '3d'])`` -> ``(str, dict)``
* ``kitti_eval_coco_style(gt_annos, dt_annos, current_classes)`` -> ``str``

Where the work runs. The annos of all frames are concatenated once on the host; ``clean_data`` / ``_prepare_data``
(name rules, MIN_HEIGHT / MAX_OCCLUSION / MAX_TRUNCATION, DontCare boxes) are whole-column numpy. Per metric there are four
launches, whatever the number of frames: the overlaps (``gga_image_box_match`` for bbox, ``gga_kitti_eval_overlaps`` for BEV
/ 3D), the first statistics pass (true-positive scores of every class x difficulty x min-overlap combination), and the
threshold pass with its reduction (``gga_kitti_eval_stats``), with one device -> host copy after each pass.
``get_thresholds`` runs on the host between them: one sort per combination. There is no CPU path for the kernels.

dtypes follow the reference where they decide a comparison: overlaps are float32 values compared in float64, the height
part of the 3D overlap and the detection-vs-DontCare overlap take the dtypes of the annos (float32 detections, float64
labels in a usual run).
"""
import numpy as np
import torch

from . import _lib
from . import functional as F
from ._lib import check

N_SAMPLE_PTS = 41
CLASS_NAMES = ['car', 'pedestrian', 'cyclist']
MIN_HEIGHT = [40, 25, 25]
MAX_OCCLUSION = [0, 1, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5]
CLASS_TO_NAME = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting'}
DEFAULT_DEVICE = 'cuda:0'


def get_thresholds(scores, num_gt, num_sample_pts=41):
    """eval.py:9-27. The reference walks the descending scores one by one; whether score i is skipped is monotone in i for a
    fixed current_recall, so each of the (at most ~num_sample_pts) kept scores is found by one vectorised test with the same
    float64 operations."""
    scores = np.sort(np.asarray(scores))[::-1]
    n = len(scores)
    if n == 0:
        return []
    i = np.arange(n)
    l_recall = (i + 1) / num_gt
    r_recall = np.where(i < n - 1, (i + 2) / num_gt, l_recall)
    not_last = i < n - 1
    current_recall, thresholds, start = 0, [], 0
    while start < n:
        skip = ((r_recall[start:] - current_recall) < (current_recall - l_recall[start:])) & not_last[start:]
        j = start + int(np.flatnonzero(~skip)[0])          # the last score is never skipped
        thresholds.append(scores[j])
        current_recall += 1 / (num_sample_pts - 1.0)
        start = j + 1
    return thresholds


def _flags(gt_name_lower, gt_bbox, gt_occluded, gt_truncated, dt_name_lower, dt_bbox, current_class, difficulty):
    """The ignore flags of clean_data (eval.py:30-82) for whole columns: 0 counted, 1 ignored, -1 other class."""
    cls = CLASS_NAMES[current_class].lower()
    valid = np.full(len(gt_name_lower), -1, np.int64)
    valid[gt_name_lower == cls] = 1
    if cls == 'pedestrian':
        valid[gt_name_lower == 'person_sitting'] = 0
    elif cls == 'car':
        valid[gt_name_lower == 'van'] = 0
    height = gt_bbox[:, 3] - gt_bbox[:, 1]
    ignore = ((gt_occluded > MAX_OCCLUSION[difficulty]) | (gt_truncated > MAX_TRUNCATION[difficulty]) |
              (height <= MIN_HEIGHT[difficulty]))
    ignored_gt = np.full(len(valid), -1, np.int8)
    ignored_gt[(valid == 0) | (ignore & (valid == 1))] = 1
    ignored_gt[(valid == 1) & ~ignore] = 0
    dt_height = np.abs(dt_bbox[:, 3] - dt_bbox[:, 1])
    ignored_dt = np.where(dt_height < MIN_HEIGHT[difficulty], 1, np.where(dt_name_lower == cls, 0, -1)).astype(np.int8)
    return ignored_gt, ignored_dt


def clean_data(gt_anno, dt_anno, current_class, difficulty):
    """eval.py:30-82 for one frame: (num_valid_gt, ignored_gt, ignored_dt, dc_bboxes)."""
    gt_name = np.asarray(gt_anno['name']).astype(str)
    dt_name = np.asarray(dt_anno['name']).astype(str)
    gt_bbox = np.asarray(gt_anno['bbox']).reshape(-1, 4)
    ignored_gt, ignored_dt = _flags(np.char.lower(gt_name), gt_bbox, np.asarray(gt_anno['occluded']),
                                    np.asarray(gt_anno['truncated']), np.char.lower(dt_name),
                                    np.asarray(dt_anno['bbox']).reshape(-1, 4), current_class, difficulty)
    dc_bboxes = [b for b in gt_bbox[gt_name == 'DontCare']]
    return int((ignored_gt == 0).sum()), ignored_gt.astype(np.int64).tolist(), ignored_dt.astype(np.int64).tolist(), dc_bboxes


def _cat(parts, width, dtype_default=np.float64):
    """Concatenate the frames' columns. Frames without objects are left out, so that the placeholder arrays they carry (often
    float64 zeros of shape [0, 4]) do not decide the dtype of the run - the reference promotes per part, where an empty frame
    meets only its own neighbours."""
    parts = [np.asarray(p).reshape(-1, width) if width else np.asarray(p).reshape(-1) for p in parts]
    parts = [p for p in parts if len(p)]
    if not parts:
        return np.zeros((0, width) if width else (0, ), dtype_default)
    return np.concatenate(parts, 0)


class _Batch:
    """The annos of all frames as whole columns, with per-frame offsets (built once per ``kitti_eval`` call)."""

    def __init__(self, gt_annos, dt_annos):
        assert len(gt_annos) == len(dt_annos)
        self.n_frames = n = len(gt_annos)
        gt_num = np.array([len(a['name']) for a in gt_annos], np.int64)
        dt_num = np.array([len(a['name']) for a in dt_annos], np.int64)
        self.gt_off, self.dt_off, self.ov_off, self.dc_off = (np.zeros(n + 1, np.int64) for _ in range(4))
        np.cumsum(gt_num, out=self.gt_off[1:])
        np.cumsum(dt_num, out=self.dt_off[1:])
        np.cumsum(gt_num * dt_num, out=self.ov_off[1:])
        self.max_dt = int(dt_num.max()) if n else 0
        self.gt_frame = np.repeat(np.arange(n), gt_num)
        self.gt_name = _cat([np.asarray(a['name']).astype(str) for a in gt_annos], 0, str).astype(str)
        self.dt_name = _cat([np.asarray(a['name']).astype(str) for a in dt_annos], 0, str).astype(str)
        self.gt_name_lower, self.dt_name_lower = np.char.lower(self.gt_name), np.char.lower(self.dt_name)
        self.gt_bbox, self.dt_bbox = _cat([a['bbox'] for a in gt_annos], 4), _cat([a['bbox'] for a in dt_annos], 4)
        self.gt_occluded = _cat([a['occluded'] for a in gt_annos], 0)
        self.gt_truncated = _cat([a['truncated'] for a in gt_annos], 0)
        self.gt_alpha, self.dt_alpha = _cat([a['alpha'] for a in gt_annos], 0), _cat([a['alpha'] for a in dt_annos], 0)
        self.dt_score = _cat([a['score'] for a in dt_annos], 0)
        box7 = lambda annos: np.concatenate([_cat([a['location'] for a in annos], 3), _cat([a['dimensions'] for a in annos], 3),
                                             _cat([a['rotation_y'] for a in annos], 0)[:, None]], 1)
        self.gt_box7, self.dt_box7 = box7(gt_annos), box7(dt_annos)
        is_dc = self.gt_name == 'DontCare'
        self.dc_boxes = self.gt_bbox[is_dc].astype(np.float64)
        np.cumsum(np.bincount(self.gt_frame[is_dc], minlength=n), out=self.dc_off[1:])
        # dt_datas of _prepare_data: bbox, alpha, score in one array, so one dtype
        self.dt_data_dtype = np.result_type(self.dt_bbox.dtype, self.dt_alpha.dtype, self.dt_score.dtype)
        self._dev = {}

    def flags(self, current_class, difficulty):
        return _flags(self.gt_name_lower, self.gt_bbox, self.gt_occluded, self.gt_truncated, self.dt_name_lower, self.dt_bbox,
                      current_class, difficulty)

    def device_arrays(self, dev):
        if dev not in self._dev:
            up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
            dt_data = np.concatenate([self.dt_bbox.astype(self.dt_data_dtype), self.dt_alpha[:, None].astype(self.dt_data_dtype),
                                      self.dt_score[:, None].astype(self.dt_data_dtype)], 1)
            self._dev[dev] = dict(gt_off=up(self.gt_off, np.int64), dt_off=up(self.dt_off, np.int64), ov_off=up(self.ov_off, np.int64),
                                  dc_off=up(self.dc_off, np.int64), dt_data=up(dt_data), gt_alpha=up(self.gt_alpha),
                                  dc_boxes=up(self.dc_boxes), gt_bbox=up(self.gt_bbox), dt_bbox=up(self.dt_bbox),
                                  gt_box7=up(self.gt_box7), dt_box7=up(self.dt_box7))
        return self._dev[dev]


def _prepare_data(gt_annos, dt_annos, current_class, difficulty):
    """eval.py:421-449 over the concatenated annos: dict of ignored_gt / ignored_dt (int8, all frames), dc_bboxes,
    total_dc_num (per frame) and total_num_valid_gt."""
    b = gt_annos if isinstance(gt_annos, _Batch) else _Batch(gt_annos, dt_annos)
    ignored_gt, ignored_dt = b.flags(current_class, difficulty)
    return dict(ignored_gt=ignored_gt, ignored_dt=ignored_dt, dc_bboxes=b.dc_boxes, total_dc_num=np.diff(b.dc_off),
                total_num_valid_gt=int((ignored_gt == 0).sum()))


def _p(t):
    return F._p(t) if t is not None and t.numel() else None


def calculate_overlaps(batch, metric, device=DEFAULT_DEVICE):
    """The per-frame [n_dt_f, n_gt_f] blocks of ``calculate_iou_partly(dt_annos, gt_annos, metric)`` as one device vector
    at ``batch.ov_off`` -> (tensor, is_float64)."""
    dev = torch.device(device)
    d = batch.device_arrays(dev)
    n_ov, n_dt, n_gt = int(batch.ov_off[-1]), int(batch.dt_off[-1]), int(batch.gt_off[-1])
    L = _lib.lib()
    F._need_cuda(d['dt_off'])
    with torch.cuda.device(dev):
        if metric == 0:
            ov = torch.zeros(n_ov, dtype=torch.float64, device=dev)
            match = torch.empty(max(n_dt, 1), dtype=torch.int64, device=dev)
            check(L.gga_image_box_match(_p(d['dt_bbox']), F._p(d['dt_off']), _p(d['gt_bbox']), F._p(d['gt_off']), batch.n_frames,
                                        n_dt, int(batch.dt_bbox.dtype == np.float32), F._p(match), None, _p(ov), F._p(d['ov_off']),
                                        F._stream()), 'gga_image_box_match')
            return ov, True
        if metric not in (1, 2):
            raise ValueError('unknown metric')
        ov = torch.zeros(n_ov, dtype=torch.float32, device=dev)
        check(L.gga_kitti_eval_overlaps(_p(d['dt_box7']), F._p(d['dt_off']), n_dt, _p(d['gt_box7']), F._p(d['gt_off']), n_gt,
                                        batch.n_frames, metric, int(batch.dt_box7.dtype == np.float32),
                                        int(batch.gt_box7.dtype == np.float32), _p(ov), F._p(d['ov_off']), n_ov, F._stream()),
              'gga_kitti_eval_overlaps')
        return ov, False


def _stats(batch, dev, ov, ov_f64, ign_gt, ign_dt, combo_cd, combo_mo, metric, compute_fp, compute_aos, thresholds=None,
           n_thresholds=None):
    d = batch.device_arrays(dev)
    n_combos, n_gt, n_dt = len(combo_cd), int(batch.gt_off[-1]), int(batch.dt_off[-1])
    L = _lib.lib()
    ws = torch.empty(int(L.gga_kitti_eval_stats_workspace_bytes(batch.n_frames, n_combos, batch.max_dt)), dtype=torch.uint8, device=dev)
    tp_det = counts = sim = d_thr = d_nthr = None
    if compute_fp:
        d_thr, d_nthr = torch.from_numpy(thresholds).to(dev), torch.from_numpy(n_thresholds).to(dev)
        counts = torch.zeros(n_combos, N_SAMPLE_PTS, 3, dtype=torch.int64, device=dev)
        sim = torch.zeros(n_combos, N_SAMPLE_PTS, dtype=torch.float64, device=dev)
    else:
        tp_det = torch.full((n_combos, n_gt), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(L.gga_kitti_eval_stats(_p(ov), int(ov_f64), F._p(d['ov_off']), ov.numel(), F._p(d['dt_off']), F._p(d['gt_off']),
                                     F._p(d['dc_off']), _p(d['dt_data']), n_dt, _p(d['gt_alpha']), n_gt, _p(d['dc_boxes']),
                                     len(batch.dc_boxes), _p(ign_gt), _p(ign_dt), ign_gt.shape[0], F._p(combo_cd), F._p(combo_mo),
                                     n_combos, batch.n_frames, batch.max_dt, metric, int(batch.dt_data_dtype == np.float32),
                                     int(compute_fp), int(compute_aos), _p(d_thr), _p(d_nthr), _p(tp_det), _p(counts), _p(sim),
                                     F._p(ws), ws.numel(), F._stream()), 'gga_kitti_eval_stats')
    if compute_fp:
        return counts.cpu().numpy(), sim.cpu().numpy()
    return tp_det.cpu().numpy()


def threshold_counts(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False,
                     device=DEFAULT_DEVICE, thresholds=None):
    """tp / fp / fn and the AOS similarity sum of every (class, difficulty, min-overlap) combination at every score threshold,
    summed over the frames: dict of ``counts`` [n_combos, 41, 3] int64, ``similarity`` [n_combos, 41], ``thresholds``
    [n_combos, 41] and ``n_thresholds`` [n_combos]; combination index = (class * n_difficulty + difficulty) * n_minoverlap + k.
    ``thresholds=(thresholds, n_thresholds)`` evaluates at given thresholds and skips the first pass that derives them.
    ``gt_annos`` may be a prepared ``_Batch``."""
    batch = gt_annos if isinstance(gt_annos, _Batch) else _Batch(gt_annos, dt_annos)
    min_overlaps = np.asarray(min_overlaps, np.float64)
    n_cls, n_diff, n_mo = len(current_classes), len(difficultys), len(min_overlaps)
    dev = torch.device(device)
    ov, ov_f64 = calculate_overlaps(batch, metric, dev)
    flags = [batch.flags(c, l) for c in current_classes for l in difficultys]
    num_valid_gt = [int((g == 0).sum()) for g, _ in flags]
    ign_gt = torch.from_numpy(np.stack([g for g, _ in flags])).to(dev)
    ign_dt = torch.from_numpy(np.stack([t for _, t in flags])).to(dev)
    cd = np.repeat(np.arange(n_cls * n_diff, dtype=np.int32), n_mo)                 # combination (m, l, k) -> flag row
    mo = np.stack([min_overlaps[:, metric, m] for m in range(n_cls)])[:, None, :].repeat(n_diff, 1).reshape(-1)
    combo_cd, combo_mo = torch.from_numpy(cd).to(dev), torch.from_numpy(np.ascontiguousarray(mo)).to(dev)
    if thresholds is None:
        # first pass: the scores of the true positives of every combination -> its score thresholds
        tp_det = _stats(batch, dev, ov, ov_f64, ign_gt, ign_dt, combo_cd, combo_mo, metric, False, False)
        thresholds = np.zeros((len(cd), N_SAMPLE_PTS), np.float64)
        n_thresholds = np.zeros(len(cd), np.int32)
        for c in range(len(cd)):
            hit = np.flatnonzero(tp_det[c] >= 0)
            scores = batch.dt_score[batch.dt_off[batch.gt_frame[hit]] + tp_det[c][hit]]
            th = get_thresholds(scores, num_valid_gt[cd[c]], N_SAMPLE_PTS)
            assert len(th) <= N_SAMPLE_PTS, len(th)
            n_thresholds[c] = len(th)
            thresholds[c, :len(th)] = th
    else:
        thresholds, n_thresholds = (np.ascontiguousarray(thresholds[0], dtype=np.float64),
                                    np.ascontiguousarray(thresholds[1], dtype=np.int32))
        assert thresholds.shape == (len(cd), N_SAMPLE_PTS) and n_thresholds.shape == (len(cd), )
    # second pass: tp / fp / fn / similarity at every threshold, summed over the frames
    counts, sim = _stats(batch, dev, ov, ov_f64, ign_gt, ign_dt, combo_cd, combo_mo, metric, True, compute_aos, thresholds,
                         n_thresholds)
    return dict(counts=counts, similarity=sim, thresholds=thresholds, n_thresholds=n_thresholds)


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, num_parts=200,
               device=DEFAULT_DEVICE):
    """eval.py:452-570: recall / precision / orientation [num_class, num_difficulty, num_minoverlap, 41]. ``gt_annos`` may be
    a prepared ``_Batch``. ``num_parts`` sized the reference's host batching and is unused."""
    batch = gt_annos if isinstance(gt_annos, _Batch) else _Batch(gt_annos, dt_annos)
    shape = [len(current_classes), len(difficultys), len(min_overlaps), N_SAMPLE_PTS]
    if batch.n_frames == 0 or 0 in shape:
        return dict(recall=np.zeros(shape), precision=np.zeros(shape), orientation=np.zeros(shape))
    st = threshold_counts(batch, None, current_classes, difficultys, metric, min_overlaps, compute_aos, device)
    tp, fp, fn = (st['counts'][..., k].astype(np.float64) for k in range(3))
    live = np.arange(N_SAMPLE_PTS)[None, :] < st['n_thresholds'][:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        rec = np.where(live, tp / (tp + fn), 0.0)
        prec = np.where(live, tp / (tp + fp), 0.0)
        ori = np.where(live, st['similarity'] / (tp + fp), 0.0) if compute_aos else np.zeros_like(prec)
    # running maximum from the right (np.max over [i:], NaN-propagating like the reference's)
    run = lambda a: np.maximum.accumulate(a[:, ::-1], axis=1)[:, ::-1].reshape(shape)
    return dict(recall=run(rec), precision=run(prec), orientation=run(ori))


def _sampled_ap(prec, first, step):
    """Mean of the curve [..., 41] over the recall sample points first, first + step, ... in percent. The points are added
    left to right (a cumulative sum), the order that fixes the last bit of the table."""
    picked = prec[..., first::step]
    return np.cumsum(picked, axis=-1)[..., -1] / picked.shape[-1] * 100


def get_mAP11(prec):
    """The 11-point interpolated AP: recall samples 0, 4, ..., 40."""
    return _sampled_ap(prec, 0, 4)


def get_mAP40(prec):
    """The 40-point AP: recall samples 1 .. 40."""
    return _sampled_ap(prec, 1, 1)


# one row per line of the AP table: label of the text line, tag of the dictionary key (None: not in the dictionary), number format
_TABLE_ROWS = (('bbox', '2D', '{:.4f}'), ('bev ', 'BEV', '{:.4f}'), ('3d  ', '3D', '{:.4f}'), ('aos ', None, '{:.2f}'))
_DICT_ROW_ORDER = (2, 1, 0)          # the dictionary lists 3D, BEV, 2D
_DIFFICULTY = ('easy', 'moderate', 'hard')
_AP_KINDS = ('AP11', 'AP40')


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, eval_types=['bbox', 'bev', '3d'], device=DEFAULT_DEVICE):
    """-> (mAP11_bbox, mAP11_bev, mAP11_3d, mAP11_aos, mAP40_bbox, mAP40_bev, mAP40_3d, mAP40_aos), each
    [num_class, 3 difficulties, num_minoverlap] or None when not asked for (the tuple of the reference's do_eval)."""
    batch = gt_annos if isinstance(gt_annos, _Batch) else _Batch(gt_annos, dt_annos)
    tables = [[None] * 4 for _ in _AP_KINDS]
    for metric, name in enumerate(('bbox', 'bev', '3d')):
        if name not in eval_types:
            continue
        with_aos = metric == 0 and 'aos' in eval_types
        ret = eval_class(batch, None, current_classes, [0, 1, 2], metric, min_overlaps, compute_aos=with_aos, device=device)
        for kind, mean in enumerate((get_mAP11, get_mAP40)):
            tables[kind][metric] = mean(ret['precision'])
            if with_aos:
                tables[kind][3] = mean(ret['orientation'])
    return tuple(tables[0] + tables[1])


_NAME_TO_CLASS = {name: index for index, name in CLASS_TO_NAME.items()}


def _class_ints(current_classes):
    """Class names or ints, one or a sequence -> list of class ints."""
    many = current_classes if isinstance(current_classes, (list, tuple)) else (current_classes, )
    return [_NAME_TO_CLASS[c] if isinstance(c, str) else c for c in many]


def _carries_alpha(annos, rule):
    """Whether the annos hold observation angles (-10 marks "none"), by the rule of the call site: 'any' - some object of
    some frame; 'first' - the first object of some frame; 'first_nonempty' - the first object of the first frame that has one."""
    alphas = [np.asarray(a['alpha']) for a in annos]
    if rule == 'any':
        return any(bool((al != -10).any()) for al in alphas)
    firsts = [al[0] for al in alphas if len(al)]
    if rule == 'first':
        return any(f != -10 for f in firsts)
    return bool(firsts) and firsts[0] != -10


def kitti_min_overlaps(current_classes):
    """[2, 3, num_class]: the strict and the loose min overlap per metric (bbox, bev, 3d) and class."""
    strict = {0: (0.7, 0.7, 0.7), 1: (0.5, 0.5, 0.5), 2: (0.5, 0.5, 0.5), 3: (0.7, 0.7, 0.7), 4: (0.5, 0.5, 0.5)}
    loose = {0: (0.7, 0.5, 0.5), 1: (0.5, 0.25, 0.25), 2: (0.5, 0.25, 0.25), 3: (0.7, 0.5, 0.5), 4: (0.5, 0.25, 0.25)}
    return np.array([[table[c] for c in current_classes] for table in (strict, loose)], np.float64).transpose(0, 2, 1)


def _table_line(label, kind, fmt, triple):
    return f'{label} {kind}:' + ', '.join(fmt.format(v) for v in triple) + '\n'


def format_kitti_results(mAPs, current_classes, min_overlaps, compute_aos):
    """The result text and the ``KITTI/...`` dictionary of kitti_eval from the eight mAP arrays of ``do_eval``
    ([num_class, 3, num_minoverlap] each, or None) - host only. ``current_classes``: class ints. Driven by _TABLE_ROWS: per
    AP kind, class and min-overlap level one header and one text line per row that was evaluated; the dictionary takes the
    rows in _DICT_ROW_ORDER per difficulty; with more than one class a block of class means at the strict level follows."""
    text, values = [], {}
    for kind, tables in zip(_AP_KINDS, (list(mAPs[:4]), list(mAPs[4:]))):
        if not compute_aos:
            tables[3] = None
        shown = [r for r in range(4) if tables[r] is not None]
        keyed = [r for r in _DICT_ROW_ORDER if tables[r] is not None]
        text.append(f'\n----------- {kind} Results ------------\n\n')
        for j, cls in enumerate(current_classes):
            for i, level in enumerate(['strict'] + ['loose'] * (min_overlaps.shape[0] - 1)):
                text.append(f'{CLASS_TO_NAME[cls]} {kind}@' + ', '.join(f'{v:.2f}' for v in min_overlaps[i, :, j]) + ':\n')
                text += [_table_line(_TABLE_ROWS[r][0], kind, _TABLE_ROWS[r][2], tables[r][j, :, i]) for r in shown]
                values.update({f'KITTI/{CLASS_TO_NAME[cls]}_{_TABLE_ROWS[r][1]}_{kind}_{diff}_{level}': tables[r][j, d, i]
                               for d, diff in enumerate(_DIFFICULTY) for r in keyed})
        if len(current_classes) > 1:
            means = [None if t is None else t.mean(axis=0) for t in tables]
            text.append(f'\nOverall {kind}@' + ', '.join(_DIFFICULTY) + ':\n')
            text += [_table_line(_TABLE_ROWS[r][0], kind, _TABLE_ROWS[r][2], means[r][:, 0]) for r in shown]
            values.update({f'KITTI/Overall_{_TABLE_ROWS[r][1]}_{kind}_{diff}': means[r][d, 0]
                           for d, diff in enumerate(_DIFFICULTY) for r in keyed})
    return ''.join(text), values


def kitti_eval(gt_annos, dt_annos, current_classes, eval_types=['bbox', 'bev', '3d'], device=DEFAULT_DEVICE):
    """-> (result text, dict of ``KITTI/...`` values), as ``mmdet3d.core.evaluation.kitti_eval``. AOS is evaluated and printed
    when some detection carries an alpha and the first label of some frame does; the caller's ``eval_types`` is not
    modified."""
    if not eval_types:
        raise AssertionError('must contain at least one evaluation type')
    if 'aos' in eval_types and 'bbox' not in eval_types:
        raise AssertionError('must evaluate bbox when evaluating aos')
    classes = _class_ints(current_classes)
    min_overlaps = kitti_min_overlaps(classes)
    compute_aos = _carries_alpha(dt_annos, 'any') and _carries_alpha(gt_annos, 'first')
    wanted = list(eval_types) + (['aos'] if compute_aos else [])
    return format_kitti_results(do_eval(gt_annos, dt_annos, classes, min_overlaps, wanted, device=device), classes, min_overlaps,
                                compute_aos)


# coco style: per class the (start, stop, count) of its ladder of min overlaps, the same for the three metrics
COCO_CLASS_TO_RANGE = {0: (0.5, 0.95, 10), 1: (0.25, 0.7, 10), 2: (0.25, 0.7, 10), 3: (0.5, 0.95, 10), 4: (0.25, 0.7, 10)}


def coco_min_overlaps(current_classes):
    """[10, 3, num_class]: every class's ladder of min overlaps, repeated over the metrics."""
    ladders = np.stack([np.linspace(*COCO_CLASS_TO_RANGE[c]) for c in current_classes], axis=1)          # [10, num_class]
    return np.repeat(ladders[:, None, :], 3, axis=1)


def format_coco_results(mAPs, current_classes, compute_aos):
    """The text of kitti_eval_coco_style from (mAPbbox, mAPbev, mAP3d, mAPaos) [num_class, 3] - host only."""
    lines = []
    for j, cls in enumerate(current_classes):
        start, stop, count = COCO_CLASS_TO_RANGE[cls]
        step = (float(stop) - float(start)) / (float(count) - 1)
        lines.append(f'{CLASS_TO_NAME[cls]} coco AP@{start:.2f}:{step:.2f}:{stop:.2f}:\n')
        for (label, _, _), table in zip(_TABLE_ROWS, mAPs):
            if table is not None and (label != 'aos ' or compute_aos):
                lines.append(_table_line(label, 'AP', '{:.2f}', table[j]))
    return ''.join(lines)


def kitti_eval_coco_style(gt_annos, dt_annos, current_classes, device=DEFAULT_DEVICE):
    """-> result text, as ``mmdet3d.core.evaluation.kitti_eval_coco_style``: the AP11 of bbox / BEV / 3D (and AOS when the first
    detection met carries an alpha) averaged over each class's ladder of ten min overlaps."""
    classes = _class_ints(current_classes)
    compute_aos = _carries_alpha(dt_annos, 'first_nonempty')
    wanted = ['bbox', 'bev', '3d'] + (['aos'] if compute_aos else [])
    ap11 = do_eval(gt_annos, dt_annos, classes, coco_min_overlaps(classes), wanted, device=device)[:4]
    return format_coco_results(tuple(None if m is None else m.mean(-1) for m in ap11), classes, compute_aos)
