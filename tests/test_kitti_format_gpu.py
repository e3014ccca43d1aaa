"""The device formatter of a test run's detections (``gga_kitti_format_dets`` / ``kitti_format.format_kitti_dets``) against

* a numpy float64 restatement of the reference's formulas (``convert_valid_bboxes`` + ``bbox2result_kitti``,
  mmdet3d/datasets/kitti_dataset_GGA_train.py:453-566,680-761; ``limit_period``, ``Box3DMode.convert`` LIDAR -> CAM,
  ``CameraInstance3DBoxes.corners``, ``points_cam2img``) - ``format_ref64`` below, on the same float32 inputs;
* the host loop (``bbox2result_kitti(device=None)``: float32 torch CPU), which sets the tolerance: two independent float32
  evaluations of one formula differ from each other by up to the sum of their errors, so the device path may be as far from
  float64 as twice the host path's worst distance (floor: one float32 ulp of the column's largest magnitude).

What is left out of a comparison, and why. A validity comparison (2D box against the image, bottom centre against the range)
within 1e-3 relative of its threshold (absolute 1e-3 where the threshold is 0: one thousandth of a pixel / millimetre) may go
either way in float32: such a detection is not required to have the float64 flag. A box with a corner closer than 0.5 m to
the camera plane has projected coordinates whose condition number is unbounded: its float columns are not compared. Both
shares are capped at 5 % and asserted (on the CPU too: tests/test_validate.py).

``test_formatter_against_float64`` and ``test_ap_tables_agree`` print every distance before they assert (run with ``-s``).
Measured on an MI355X (worst distance from float64: host loop / device / bound; EXPERIMENTS.md 6i): bbox 1.890e-04 / 1.695e-04 /
3.780e-04, location 8.086e-06 / 1.112e-05 / 1.617e-05, rotation_y 3.378e-07 / 3.378e-07 / 6.755e-07, alpha 4.841e-07 / 4.710e-07 /
9.681e-07, dimensions and score 0 / 0; left out 0.013 % (boundary) and 0 % (depth); AP tables: |device - host| 0 and
|host - float64| 0 over 126 values."""
import copy
import os

import numpy as np
import pytest
import torch

CLASSES = ('Pedestrian', 'Cyclist', 'Car')
LIMIT_RANGE = [0, -40, -3, 70.4, 40, 0.0]
NEAR = 1e-3
MIN_DEPTH = 0.5
COLUMNS = ('bbox', 'dimensions', 'location', 'rotation_y', 'alpha', 'score')


# ------------------------------------------------------------------------------------------------ float64 restatement
def limit_period64(val, offset=0.5, period=np.pi):
    return val - np.floor(val / period + offset) * period


def format_ref64(boxes, lidar2cam, p2, image_hw, limit_range=LIMIT_RANGE):
    """One frame. boxes [n,7] (x, y, z_bottom, dx, dy, dz, yaw), lidar2cam / p2 4x4, image_hw (h, w); everything is taken
    to float64 first. -> dict: ``yaw`` (limited), ``valid``, ``near`` (a validity comparison within NEAR of its threshold),
    ``min_depth`` (smallest |z_cam| of the eight corners), and the columns of every detection (valid or not): ``bbox``
    (clipped), ``bbox_raw``, ``dimensions``, ``location``, ``rotation_y``, ``alpha``."""
    b = np.asarray(boxes, np.float64).reshape(-1, 7)
    rt, pm = np.asarray(lidar2cam, np.float64), np.asarray(p2, np.float64)
    h, w = float(image_hw[0]), float(image_hw[1])
    n = len(b)
    yaw = limit_period64(b[:, 6], 0.5, 2 * np.pi)
    loc = np.concatenate([b[:, :3], np.ones((n, 1))], 1) @ rt.T
    loc = loc[:, :3]
    dims = b[:, [3, 5, 4]]
    ry = limit_period64(-yaw - np.pi / 2, 0.5, 2 * np.pi)
    idx = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]], np.float64)
    corners = dims[:, None, :] * (idx - np.array([0.5, 1.0, 0.5]))[None]
    c, s = np.cos(ry)[:, None], np.sin(ry)[:, None]
    rot = np.stack([corners[..., 0] * c + corners[..., 2] * s, corners[..., 1], -corners[..., 0] * s + corners[..., 2] * c], -1)
    rot = rot + loc[:, None, :]
    p4 = np.concatenate([rot, np.ones((n, 8, 1))], -1) @ pm.T
    uv = p4[..., :2] / p4[..., 2:3]
    raw = np.concatenate([uv.min(1), uv.max(1)], 1).reshape(n, 4)
    lim = np.asarray(limit_range, np.float64)
    values = np.concatenate([raw, b[:, :3], b[:, :3]], 1)
    thresholds = np.concatenate([[w, h, 0.0, 0.0], lim]).reshape(1, 10)
    below = np.array([1, 1, 0, 0, 0, 0, 0, 1, 1, 1], bool).reshape(1, 10)        # value < threshold, else value > threshold
    passed = np.where(below, values < thresholds, values > thresholds)
    near = (np.abs(values - thresholds) <= NEAR * np.maximum(np.abs(thresholds), 1.0)).any(1)
    bbox = raw.copy()
    bbox[:, 2:] = np.minimum(bbox[:, 2:], [w, h])
    bbox[:, :2] = np.maximum(bbox[:, :2], [0, 0])
    return dict(yaw=yaw, valid=passed.all(1), near=near, min_depth=np.abs(p4[..., 2]).min(1) if n else np.zeros(0), bbox=bbox, bbox_raw=raw,
                dimensions=dims, location=loc, rotation_y=ry, alpha=-np.arctan2(-b[:, 1], b[:, 0]) + ry)


# ------------------------------------------------------------------------------------------------------------ generator
def kitti_calib(rng):
    """KITTI-shaped calibration with a little per-frame variation (float64, as the info files hold it)."""
    p2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884], [0, 0, 0, 1]])
    p2[0, 0] = p2[1, 1] = 721.5377 + rng.uniform(-15, 15)
    p2[0, 2] += rng.uniform(-8, 8)
    p2[1, 2] += rng.uniform(-5, 5)
    ax, ay, az = rng.uniform(-0.02, 0.02, 3)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    r0 = np.eye(4)
    r0[:3, :3] = rx @ ry @ rz
    tr = np.eye(4)
    tr[:3, :3] = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]) @ rz.T @ rx
    tr[:3, 3] = [-0.004 + rng.uniform(-0.01, 0.01), -0.076 + rng.uniform(-0.01, 0.01), -0.27 + rng.uniform(-0.02, 0.02)]
    return dict(P2=p2, R0_rect=r0, Tr_velo_to_cam=tr)


_SIZES = {0: (0.8, 0.6, 1.73), 1: (1.76, 0.6, 1.73), 2: (3.9, 1.6, 1.56)}       # (dx, dy, dz) per class


def _lidar2cam32(calib):
    return calib['R0_rect'].astype(np.float32) @ calib['Tr_velo_to_cam'].astype(np.float32)


def make_run(n_frames=200, seed=7, max_dets=80):
    """-> (infos with ground-truth ``annos`` near the detections, net_outputs as ``single_gpu_test`` returns them). Frame 0 is
    empty, frame 1 holds only detections outside the range (all invalid), frame 2 has ``max_dets`` (> 64) detections; the others
    0 .. max_dets. Kinds: objects in front of the car (x 5 - 65 m; most are jittered copies of a ground truth), boxes at least
    0.5 m outside ``LIMIT_RANGE``, boxes in range but outside the camera's frustum, boxes behind the car. Scores are unique
    within a frame (the tests find a formatted row's detection by its score)."""
    from gga_amd.box3d import LiDARInstance3DBoxes
    rng = np.random.default_rng(seed)
    infos, outs = [], []
    for f in range(n_frames):
        calib = kitti_calib(rng)
        hw = np.array([rng.integers(370, 377), rng.integers(1224, 1243)], np.int32)
        n = 0 if f == 0 else (max_dets if f == 2 else (12 if f == 1 else int(rng.integers(0, max_dets + 1))))
        if f > 2 and rng.random() < 0.05:
            n = 0
        kind = rng.choice(4, n, p=[0.62, 0.14, 0.14, 0.10]) if f != 1 else np.ones(n, np.int64)
        labels = rng.integers(0, 3, n)
        boxes = np.zeros((n, 7))
        for i in range(n):
            size = np.array(_SIZES[int(labels[i])]) * rng.uniform(0.85, 1.15, 3)
            x, y, z = rng.uniform(5, 65), 0.0, rng.uniform(-2.4, -0.6)
            if kind[i] == 0:
                y = rng.uniform(-0.45, 0.45) * x
            elif kind[i] == 1:          # at least 0.5 m outside the range, on one of its faces
                face = rng.integers(0, 5)
                y = rng.uniform(-0.4, 0.4) * x
                if face == 0:
                    x = rng.uniform(70.9, 80)
                elif face == 1:
                    y = rng.uniform(40.5, 48) * rng.choice([-1, 1])
                    x = rng.uniform(45, 65)
                elif face == 2:
                    z = rng.uniform(0.5, 1.5)
                elif face == 3:
                    z = rng.uniform(-5, -3.5)
                else:
                    x = rng.uniform(-4.0, -0.5) - 5
            elif kind[i] == 2:          # in range, beside the frustum
                x = rng.uniform(5, 12)
                y = rng.uniform(2.0, 3.2) * x * rng.choice([-1, 1])
            else:                       # behind the car
                x, y = rng.uniform(-30, -5), rng.uniform(-10, 10)
            boxes[i] = [x, y, z, *size, rng.uniform(-10, 10)]
        boxes32 = boxes.astype(np.float32)
        # ground truths: most kind-0 boxes; the detection is a jittered copy
        is_gt = (kind == 0) & (rng.random(n) < 0.8)
        gt = format_ref64(boxes32[is_gt], _lidar2cam32(calib), calib['P2'].astype(np.float32), hw)
        keep = gt['valid']
        annos = dict(name=np.array([CLASSES[int(l)] for l in labels[is_gt][keep]]), truncated=np.zeros(int(keep.sum())),
                     occluded=np.zeros(int(keep.sum()), np.int64), alpha=gt['alpha'][keep], bbox=gt['bbox'][keep],
                     dimensions=gt['dimensions'][keep], location=gt['location'][keep], rotation_y=gt['rotation_y'][keep])
        det = boxes32.copy()
        jitter = rng.normal(0, 1, (n, 7)) * np.array([0.15, 0.15, 0.05, 0.1, 0.05, 0.05, 0.08]) * rng.uniform(0.2, 2.5, (n, 1))
        det[is_gt] += jitter[is_gt].astype(np.float32)
        scores = rng.permutation(np.arange(1, 4097))[:n].astype(np.float32) / 4096
        infos.append(dict(image=dict(image_idx=f, image_shape=hw), calib=calib, annos=annos))
        outs.append(dict(boxes_3d=LiDARInstance3DBoxes(torch.from_numpy(det)), scores_3d=torch.from_numpy(scores),
                         labels_3d=torch.from_numpy(labels.astype(np.int64))))
    return infos, outs


def reference_run(infos, outs):
    """``format_ref64`` of every frame of ``outs`` (before any path has limited their yaw in place)."""
    return [format_ref64(o['boxes_3d'].tensor.numpy(), _lidar2cam32(i['calib']), i['calib']['P2'].astype(np.float32), i['image']['image_shape'])
            for i, o in zip(infos, outs)]


def left_out_shares(refs):
    """(share of detections near a decision boundary, share with a corner closer than MIN_DEPTH to the camera plane)."""
    n = sum(len(r['valid']) for r in refs)
    return sum(int(r['near'].sum()) for r in refs) / n, sum(int((r['min_depth'] < MIN_DEPTH).sum()) for r in refs) / n


def ref_annos(refs, outs):
    """The float64 restatement as KITTI annos (float64 columns), for kitti_eval."""
    annos = []
    for r, o in zip(refs, outs):
        v = r['valid']
        lab = o['labels_3d'].numpy()[v]
        annos.append(dict(name=np.array([CLASSES[int(l)] for l in lab]), truncated=np.zeros(int(v.sum())), occluded=np.zeros(int(v.sum()), np.int64),
                          alpha=r['alpha'][v], bbox=r['bbox'][v], dimensions=r['dimensions'][v], location=r['location'][v],
                          rotation_y=r['rotation_y'][v], score=o['scores_3d'].numpy()[v].astype(np.float64)))
    return annos


def make_dataset(infos):
    from gga_amd.datasets import KittiDataset_GGA_train
    return KittiDataset_GGA_train('/nonexistent', infos, 'training', classes=CLASSES, modality=dict(use_lidar=True, use_camera=False),
                                  test_mode=True, pcd_limit_range=LIMIT_RANGE)


def _rows(anno, out):
    """Original detection index of every row of a formatted frame (by its score, unique within the frame)."""
    scores = out['scores_3d'].numpy()
    order = {float(s): i for i, s in enumerate(scores)}
    assert len(order) == len(scores)
    return np.array([order[float(s)] for s in anno['score']], np.int64)


def _distances(annos, refs, outs, compare):
    """Worst |column - float64| per column over the detections of ``compare`` (per frame bool masks) a path reports."""
    worst, largest = {c: 0.0 for c in COLUMNS}, {c: 0.0 for c in COLUMNS}
    for a, r, o, m in zip(annos, refs, outs, compare):
        if not len(a['score']):
            continue
        rows = _rows(a, o)
        sel = m[rows]
        for c in COLUMNS:
            want = o['scores_3d'].numpy().astype(np.float64) if c == 'score' else r[c]
            got, want = np.asarray(a[c], np.float64)[sel], want[rows][sel]
            if got.size:
                worst[c] = max(worst[c], float(np.abs(got - want).max()))
                largest[c] = max(largest[c], float(np.abs(want).max()))
    return worst, largest


@pytest.fixture(scope='module')
def run():
    infos, outs = make_run()
    refs = reference_run(infos, outs)
    ds = make_dataset(infos)
    host_outs, dev_outs = copy.deepcopy(outs), copy.deepcopy(outs)
    host = ds.bbox2result_kitti(host_outs, CLASSES, device=None)
    dev = ds.bbox2result_kitti(dev_outs, CLASSES, device='cuda:0')
    return dict(infos=infos, outs=outs, refs=refs, ds=ds, host=host, dev=dev, host_outs=host_outs, dev_outs=dev_outs)


@pytest.mark.gpu
def test_formatter_against_float64(run):
    refs, outs = run['refs'], run['outs']
    counts = [len(r['valid']) for r in refs]
    assert len(refs) == 200 and min(counts) == 0 and max(counts) > 64 and max(counts) <= 80
    near_share, depth_share = left_out_shares(refs)
    print(f'left out: near a decision boundary {near_share:.4%}, corner within {MIN_DEPTH} m of the camera plane {depth_share:.4%}')
    assert near_share <= 0.05 and depth_share <= 0.05
    # flags and counts: the valid set, in the original order, for every detection away from the decision boundaries
    for f, (a, r, o) in enumerate(zip(run['dev'], refs, outs)):
        rows = _rows(a, o) if len(a['score']) else np.zeros(0, np.int64)
        assert (np.diff(rows) > 0).all(), f'frame {f}: the valid detections are not in their original order'
        got = np.zeros(len(r['valid']), bool)
        got[rows] = True
        sure = ~r['near']
        assert np.array_equal(got[sure], r['valid'][sure]), f'frame {f}: valid set differs from float64 away from the boundaries'
    # floats: device at most twice as far from float64 as the host loop (floor: one float32 ulp of the column's largest magnitude)
    compare = [r['valid'] & ~r['near'] & (r['min_depth'] >= MIN_DEPTH) for r in refs]
    assert sum(int(m.sum()) for m in compare) > 2000
    host_worst, largest = _distances(run['host'], refs, outs, compare)
    dev_worst, _ = _distances(run['dev'], refs, outs, compare)
    bad = []
    for c in COLUMNS:
        ulp = float(np.spacing(np.float32(largest[c])))
        bound = max(2 * host_worst[c], ulp)
        print(f'{c:>11}: host loop {host_worst[c]:.3e}  device {dev_worst[c]:.3e}  bound {bound:.3e}  (ulp of {largest[c]:.4g}: {ulp:.3e})')
        if not dev_worst[c] <= bound:
            bad.append(c)
    assert not bad, f'device columns farther from float64 than allowed: {bad}'
    # the limited yaw written back into the caller's boxes
    for o_dev, r in zip(run['dev_outs'], refs):
        yaw = o_dev['boxes_3d'].tensor[:, 6].numpy().astype(np.float64)
        assert np.abs(yaw - r['yaw']).max(initial=0.0) <= 4 * float(np.spacing(np.float32(np.pi)))


@pytest.mark.gpu
def test_same_contract_as_the_host_path(run, tmp_path):
    refs = run['refs']
    assert len(run['host']) == len(run['dev']) == len(refs)
    assert len(run['dev'][0]['score']) == 0 and len(refs[1]['valid']) > 0 and not refs[1]['valid'].any()      # empty / all-invalid frames
    for f, (h, d, r) in enumerate(zip(run['host'], run['dev'], refs)):
        assert list(h) == list(d), f
        if r['near'].any():
            continue
        for k in h:
            assert h[k].dtype == d[k].dtype and h[k].shape == d[k].shape, (f, k, h[k].dtype, d[k].dtype, h[k].shape, d[k].shape)
        assert np.array_equal(h['sample_idx'], d['sample_idx']) and np.array_equal(h['name'], d['name'])
        assert np.array_equal(h['score'], d['score'])
    for a, b in zip(run['host_outs'], run['dev_outs']):           # the in-place yaw limit: the same float32 operation on both sides
        assert torch.equal(a['boxes_3d'].tensor, b['boxes_3d'].tensor)
        assert torch.equal(a['scores_3d'], b['scores_3d']) and torch.equal(a['labels_3d'], b['labels_3d'])
    # submission directories
    few = [f for f in range(len(refs)) if not refs[f]['near'].any()][:12]
    assert 0 in few and 1 in few and 2 in few
    sub_infos = [run['infos'][f] for f in few]
    ds = make_dataset(sub_infos)
    for name, device in (('host', None), ('dev', 'cuda:0')):
        ds.bbox2result_kitti(copy.deepcopy([run['outs'][f] for f in few]), CLASSES, submission_prefix=str(tmp_path / name), device=device)
    files = sorted(os.listdir(tmp_path / 'host'))
    assert files == sorted(os.listdir(tmp_path / 'dev')) and len(files) == len(few)
    lines = lambda p: len(open(p).read().splitlines())
    assert [lines(tmp_path / 'host' / f) for f in files] == [lines(tmp_path / 'dev' / f) for f in files]
    assert sum(lines(tmp_path / 'dev' / f) for f in files) > 0


@pytest.mark.gpu
def test_ap_tables_agree(run):
    from gga_amd.kitti_eval import kitti_eval
    gt = [i['annos'] for i in run['infos']]
    _, ap_host = kitti_eval(gt, run['host'], CLASSES)
    _, ap_dev = kitti_eval(gt, run['dev'], CLASSES)
    _, ap_ref = kitti_eval(gt, ref_annos(run['refs'], run['outs']), CLASSES)
    assert set(ap_host) == set(ap_dev) == set(ap_ref) and len(ap_dev) > 0
    assert any(0.0 < v < 100.0 for v in ap_dev.values()), ap_dev
    worst_dev = worst_host = 0.0
    bad = []
    for k in ap_host:
        d_host, d_dev = abs(ap_host[k] - ap_ref[k]), abs(ap_dev[k] - ap_host[k])
        worst_dev, worst_host = max(worst_dev, d_dev), max(worst_host, d_host)
        if not d_dev <= max(2 * d_host, 1e-4):
            bad.append((k, ap_host[k], ap_dev[k], ap_ref[k]))
    print(f'AP tables: worst |device - host| {worst_dev:.3e}, worst |host - float64| {worst_host:.3e} over {len(ap_host)} values')
    assert not bad, bad


@pytest.mark.gpu
def test_environment_switch_routes_evaluate_to_the_host_loop(run, monkeypatch):
    from gga_amd import kitti_format
    few = list(range(3, 9))
    ds = make_dataset([run['infos'][f] for f in few])
    outs = [run['outs'][f] for f in few]
    calls = []
    real = kitti_format.format_kitti_dets
    monkeypatch.setattr(kitti_format, 'format_kitti_dets', lambda *a, **k: calls.append(1) or real(*a, **k))
    on = ds.evaluate(copy.deepcopy(outs), device='cuda:0')
    assert calls == [1]
    monkeypatch.setenv('GGA_KITTI_FORMAT', '0')
    off = ds.evaluate(copy.deepcopy(outs), device='cuda:0')
    assert calls == [1], 'GGA_KITTI_FORMAT=0 must keep evaluate on the host loop'
    assert set(on) == set(off) and any(k.startswith('KITTI/') for k in on)
    with pytest.raises(NotImplementedError):
        ds.evaluate(copy.deepcopy(outs), show=True)
