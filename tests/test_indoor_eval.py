"""Indoor mAP / mAR evaluation and the SUN RGB-D dataset on the CPU: ``gga_amd/indoor_eval.py`` (host path) against
tests/golden/indoor_eval.npz (the reference's own indoor_eval.py, tools_dev/make_golden.py::golden_indoor_eval),
``SUNRGBDDataset`` on a synthetic tree, ``PointSample`` and ``LoadPointsFromFile(coord_type='DEPTH')``."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from gga_amd import Config, synthetic
from gga_amd import indoor_eval as IE
from gga_amd import loader as LD
from gga_amd.fcaf3d import DepthInstance3DBoxes
from gga_amd.indoor_datasets import SUNRGBDDataset
from gga_amd.pipelines import IndoorPointSample, LoadPointsFromFile, PointSample
from gga_amd.points import DepthPoints

import _indoor_eval_ref as R

CFG = os.path.join(REPO, 'configs', 'fcaf3d', 'fcaf3d_8x2_sunrgbd-3d-10class.py')
LABEL2CAT = dict(enumerate(synthetic.INDOOR_CLASSES))


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'indoor_eval.npz'))


def same_values(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def test_average_precision_on_hand_worked_curves():
    rec, prec = np.array([0.25, 0.5, 0.5, 0.75]), np.array([1.0, 1.0, 2 / 3, 0.75])
    # area: the precision envelope is 1, 1, .75, .75 (then 0 up to recall 1): .25 * 1 + .25 * 1 + .25 * .75
    assert IE.average_precision(rec, prec)[0] == np.float32(0.6875)
    # 11 points: recalls 0 .. .5 see precision 1 (6 points), .6 and .7 see .75, .8 .. 1 nothing
    assert IE.average_precision(rec, prec, '11points')[0] == pytest.approx((6 * 1.0 + 2 * 0.75) / 11, rel=1e-6)
    # two scales: the reference divides by 11 inside the loop over scales, so the first scale is divided twice
    two = IE.average_precision(np.stack([rec, rec]), np.stack([prec, prec]), '11points')
    assert two[0] == pytest.approx(7.5 / 121, rel=1e-6) and two[1] == pytest.approx(7.5 / 11, rel=1e-6)
    assert IE.average_precision(np.zeros(1), np.zeros(1))[0] == 0
    assert np.isnan(IE.average_precision(np.array([np.nan, np.nan]), np.array([0.0, 0.0]))[0])
    with pytest.raises(ValueError):
        IE.average_precision(rec, prec, 'other')


@pytest.mark.parametrize('case', ['B', 'C'])
def test_host_path_equals_the_reference(golden, case):
    gts, dts = R.unpack_case(case, golden)
    lines = []
    ret = IE.indoor_eval(gts, R.as_results(dts, DepthInstance3DBoxes), R.THRESHOLDS, LABEL2CAT, logger=lines.append, device='cpu')
    assert list(ret.keys()) == [str(k) for k in golden[f'{case}.ret_keys']]
    assert same_values(list(ret.values()), golden[f'{case}.ret_values'])
    assert np.isnan(list(ret.values())).any() == (case == 'C')
    batch = IE._columns(gts, R.as_results(dts, DepthInstance3DBoxes), None, None)
    assert batch.labels == [int(v) for v in golden[f'{case}.labels']]
    rec, prec, ap = IE._evaluate(batch, list(R.THRESHOLDS), 'cpu')
    for t in range(2):
        for label in batch.labels:
            assert same_values(rec[t][label], golden[f'{case}.rec.{t}.{label}']), (t, label)
            assert same_values(prec[t][label], golden[f'{case}.prec.{t}.{label}']), (t, label)
    table = lines[0].strip('\n').split('\n')
    assert table[1].split('|')[1:-1] == [' classes' + ' ' * (len(table[1].split('|')[1]) - 8), ' AP_0.25 ', ' AR_0.25 ', ' AP_0.50 ', ' AR_0.50 ']
    assert table[0] == table[2] == table[-3] == table[-1] and table[-2].startswith('| Overall')
    assert len(table) == len(batch.labels) + 6


def test_eval_map_recall_takes_the_reference_layout(golden):
    gts, dts = R.unpack_case('B', golden)
    pred, gt = {}, {}
    for f, (g, d) in enumerate(zip(gts, dts)):
        for box, score, label in zip(d['boxes'], d['scores'], d['labels']):
            pred.setdefault(int(label), {}).setdefault(f, []).append((DepthInstance3DBoxes(box[None]), score))
            gt.setdefault(int(label), {}).setdefault(f, [])
        if g['gt_num']:
            for box, label in zip(R.bottom_centre(g['gt_boxes_upright_depth']), g['class']):
                gt.setdefault(int(label), {}).setdefault(f, []).append(DepthInstance3DBoxes(box[None]))
    rec, prec, ap = IE.eval_map_recall(pred, gt, list(R.THRESHOLDS), device='cpu')
    assert list(ap[0].keys()) == [int(v) for v in golden['B.labels']]
    for t in range(2):
        for label in gt:
            assert same_values(rec[t][label], golden[f'B.rec.{t}.{label}'])


def test_case_b_keeps_its_margins(golden):
    """What lets the flags be compared exactly: distinct scores, and in float64 every best IoU at least MARGIN from both
    thresholds, from its runner-up and - unless it is exactly 0 - from 0. The share of detections left out of a comparison is 0."""
    assert float(golden['A.ref_err']) * 100 <= R.MARGIN
    for case in ('B', 'C'):
        gts, dts = R.unpack_case(case, golden)
        scores = np.concatenate([d['scores'] for d in dts])
        assert len(np.unique(scores)) == len(scores)
        stats = np.array(R.best_two64(gts, dts))
        best, second = stats[:, 0], stats[:, 2]
        for thr in R.THRESHOLDS:
            assert np.abs(best - thr).min() >= R.MARGIN
        pos = best > 0
        assert (best[pos] - second[pos]).min() >= R.MARGIN and best[pos].min() >= R.MARGIN
        assert (best[~pos & np.isfinite(best)] == 0).all()
    gts, dts = R.unpack_case('B', golden)
    assert gts[3]['gt_num'] == 0 and len(dts[5]['labels']) == 0
    assert 9 in np.concatenate([g['class'] for g in gts if g['gt_num']]) and 9 not in np.concatenate([d['labels'] for d in dts])
    # the two detections on one ground truth: both far above 0.5, the lower-scored one a false positive in the golden
    twins = np.array(R.best_two64(gts[:1], dts[:1]))[-2:]
    assert (twins[:, 0] > 0.6).all() and twins[0, 1] == twins[1, 1] == 0


def test_host_overlaps_of_case_a(golden):
    got = IE.iou3d_pairs32(golden['A.det'], golden['A.gt'])
    deg = golden['A.degenerate']
    assert np.abs(got.astype(np.float64) - golden['A.iou64'])[~deg].max() <= float(golden['A.ref_err'])
    assert np.array_equal(got, golden['A.iou32'])
    # single-ground-truth segments: the matcher's maximum is the pair's IoU
    n = len(got)
    iou_max, jmax = IE.match_host(golden['A.det'], np.arange(n + 1), golden['A.gt'], np.arange(n + 1))
    assert np.array_equal(iou_max, got) and (jmax == 0).all()


# ------------------------------------------------------------------------------------------------------------- dataset
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('sunrgbd'))
    train, val = synthetic.write_sunrgbd_tree(root, 5, n_points=300)
    return root, train, val


def val_cfg(root, val, n_points=200):
    cfg = Config.fromfile(CFG)
    d = cfg.data['val']
    d.update(data_root=root, ann_file=val)
    d['pipeline'][1]['transforms'][2]['num_points'] = n_points
    return cfg, d


def test_config_builds_its_val_dataset(tree):
    root, train, val = tree
    cfg, d = val_cfg(root, val)
    assert cfg.data['test']['type'] == 'SUNRGBDDataset' and cfg.evaluation['interval'] == 1
    ds = LD.build_dataset(d)
    assert isinstance(ds, SUNRGBDDataset) and len(ds) == 5 and ds.test_mode and tuple(ds.CLASSES) == SUNRGBDDataset.CLASSES
    sample = ds[0]
    # the layout single_gpu_test expects: every key a list over augmentations
    assert set(sample) == {'img_metas', 'points'} and len(sample['points']) == 1
    pts, meta = sample['points'][0].data, sample['img_metas'][0].data
    assert pts.shape == (200, 6) and pts.dtype == torch.float32
    assert meta['box_type_3d'] is DepthInstance3DBoxes and meta['sample_idx'] == 0 and meta['pcd_horizontal_flip'] is False
    assert 'ann_info' not in ds.get_data_info(0)


def test_ann_info_and_empty_frames(tree):
    root, train, val = tree
    ds = SUNRGBDDataset(root, train, pipeline=[dict(type='LoadPointsFromFile', coord_type='DEPTH', load_dim=6, use_dim=[0, 1, 2, 3, 4, 5]),
                                               dict(type='LoadAnnotations3D'), dict(type='PointSample', num_points=100),
                                               dict(type='DefaultFormatBundle3D', class_names=SUNRGBDDataset.CLASSES),
                                               dict(type='Collect3D', keys=['points', 'gt_bboxes_3d', 'gt_labels_3d'])],
                        modality=dict(use_camera=False, use_lidar=True))
    assert (ds.flag == 0).all() and ds.flag.dtype == np.uint8
    raw = ds.data_infos[0]['annos']['gt_boxes_upright_depth'].astype(np.float32)
    ann = ds.get_ann_info(0)
    want = raw.copy()
    want[:, 2] = raw[:, 2] + raw[:, 5] * np.float32(-0.5)          # origin (0.5, 0.5, 0.5) -> the bottom centre
    assert np.array_equal(ann['gt_bboxes_3d'].tensor.numpy(), want) and ann['gt_labels_3d'].dtype == np.int64
    empty = ds.get_ann_info(1)
    assert ds.data_infos[1]['annos']['gt_num'] == 0 and empty['gt_bboxes_3d'].tensor.shape == (0, 7) and empty['gt_labels_3d'].shape == (0,)
    assert ds.get_data_info(1) is None and ds.prepare_train_data(1) is None
    np.random.seed(3)
    state = np.random.get_state()
    sample = ds[1]                                                 # filter_empty_gt: another frame is drawn
    np.random.set_state(state)
    drawn = int(np.random.choice(np.arange(5)))
    assert drawn != 1 and sample['img_metas'].data['sample_idx'] == drawn
    assert isinstance(sample['gt_bboxes_3d'].data, DepthInstance3DBoxes) and sample['points'].data.shape == (100, 6)
    keep = SUNRGBDDataset(root, train, modality=dict(use_camera=True, use_lidar=True), filter_empty_gt=False)
    info = keep.get_data_info(1)
    assert info['depth2img'].shape == (3, 3) and info['img_info']['filename'].endswith('sunrgbd_trainval/image/000001.jpg')
    assert keep.get_ann_info(1)['bboxes'].shape == (0, 4)


def test_evaluate_on_the_host(tree):
    root, train, val = tree
    ds = LD.build_dataset(val_cfg(root, val)[1])
    results = []
    for i in range(len(ds)):          # the ground truths themselves as detections, one frame's first box moved away
        b = ds.get_ann_info(i)['gt_bboxes_3d'].tensor.clone()
        if i == 0:
            b[0, 0] += 10
        lab = ds.get_ann_info(i)['gt_labels_3d']
        results.append(dict(boxes_3d=DepthInstance3DBoxes(b), scores_3d=torch.linspace(0.9, 0.5, len(b)), labels_3d=torch.from_numpy(lab)))
    lines = []
    ret = ds.evaluate(results, logger=lines.append, device='cpu')
    n_gt = sum(i['annos']['gt_num'] for i in ds.data_infos)
    missed = SUNRGBDDataset.CLASSES[int(ds.data_infos[0]['annos']['class'][0])]
    assert ret[f'{missed}_rec_0.25'] < 1 and all(v == 1 for k, v in ret.items() if '_rec_' in k and not k.startswith(missed))
    assert 0 < ret['mAP_0.50'] < 1 and n_gt > 5 and 'Overall' in lines[0]
    out, tmp = ds.format_results(results)
    assert out is results and os.path.exists(os.path.join(tmp.name, 'results.pkl'))
    with pytest.raises(NotImplementedError):
        ds.evaluate([np.zeros((0, 5))] * len(ds))
    with pytest.raises(NotImplementedError):
        ds.evaluate(results, show=True, device='cpu', logger='silent')


# ----------------------------------------------------------------------------------------------------------- transforms
def test_point_sample_draws_like_the_reference():
    """The draws of transforms_3d.py:1043-1089, replayed from the same ``np.random`` state."""
    pts = DepthPoints(torch.arange(50 * 3, dtype=torch.float32).reshape(50, 3) / 50, points_dim=3)
    np.random.seed(11)
    out = PointSample(80)(dict(points=pts))['points']           # fewer points than asked: with replacement
    np.random.seed(11)
    want = np.random.choice(range(50), 80, replace=True)
    assert isinstance(out, DepthPoints) and torch.equal(out.tensor, pts.tensor[want]) and len(np.unique(want)) < 80
    np.random.seed(12)
    mask = np.arange(50)
    got = PointSample(20, sample_range=4.0)(dict(points=pts, pts_semantic_mask=mask))
    dist = np.linalg.norm(pts.tensor.numpy(), axis=1)
    far, near = np.where(dist >= 4.0)[0], np.where(dist < 4.0)[0]
    assert 0 < len(far) < 20
    np.random.seed(12)
    want = np.concatenate((far, np.random.choice(near, 20 - len(far), replace=False)))
    np.random.shuffle(want)
    assert torch.equal(got['points'].tensor, pts.tensor[want]) and np.array_equal(got['pts_semantic_mask'], want)
    np.random.seed(13)
    got = PointSample(10, sample_range=1.0)(dict(points=pts))['points']          # more far points than asked: they are drawn first
    far, near = np.where(dist >= 1.0)[0], np.where(dist < 1.0)[0]
    np.random.seed(13)
    far_kept = np.random.choice(far, 10, replace=False)
    want = np.concatenate((far_kept, np.random.choice(near, 0, replace=False)))
    np.random.shuffle(want)
    assert len(far) > 10 and torch.equal(got.tensor, pts.tensor[want])
    with pytest.warns(UserWarning, match='deprecated'):
        assert isinstance(IndoorPointSample(5), PointSample)


def test_load_points_depth(tmp_path):
    pts = np.random.default_rng(0).uniform(-1, 1, (7, 6)).astype(np.float32)
    path = str(tmp_path / 'a.bin')
    pts.tofile(path)
    out = LoadPointsFromFile(coord_type='DEPTH', load_dim=6, use_dim=[0, 1, 2, 3, 4, 5])(dict(pts_filename=path))['points']
    assert type(out) is DepthPoints and np.array_equal(out.tensor.numpy(), pts) and out.rotation_axis == 2
    out = LoadPointsFromFile(coord_type='DEPTH', load_dim=6, use_dim=3)(dict(pts_filename=path))['points']
    assert out.tensor.shape == (7, 3)
    with pytest.raises(AssertionError):
        LoadPointsFromFile(coord_type='CAMERA')
    with pytest.raises(AssertionError):
        LoadPointsFromFile(coord_type='DEPTH', shift_height=True)


def test_depth_boxes_accessors():
    b = DepthInstance3DBoxes(torch.tensor([[0., 0, 1, 2, 4, 6, 0.3], [1., 1, 0, 1, 1, 1, 0]]), origin=(0.5, 0.5, 0.5))
    assert torch.equal(b.bottom_height, torch.tensor([-2., -0.5])) and torch.equal(b.top_height, torch.tensor([4., 0.5]))
    assert torch.equal(b.bev, b.tensor[:, [0, 1, 3, 4, 6]]) and len(b[0]) == 1 and len(b[torch.tensor([True, True])]) == 2
    assert b.convert_to(None) is b and b.convert_to('Depth') is b and isinstance(b.new_box([[0., 0, 0, 1, 1, 1, 0]]), DepthInstance3DBoxes)
    with pytest.raises(NotImplementedError):
        b.convert_to('LiDAR')
    assert torch.equal(DepthInstance3DBoxes.height_overlaps(b, b), torch.tensor([[6., 1.], [1., 1.]]))
