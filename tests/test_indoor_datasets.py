"""``ScanNetDataset`` / ``S3DISDataset``, ``GlobalAlignment`` / ``NormalizePointsColor`` / ``LoadPointsFromFile(use_color=True)``,
``ConcatDataset`` and the two FCAF3D configs that use them, on the CPU: against tests/golden/indoor_datasets.npz (a run of the
reference's classes on the same synthetic trees, tools_dev/make_golden.py::golden_indoor_datasets) and
tests/golden/reference_configs_indoor.json (the reference's two configs, resolved); ``evaluate`` against a float64 restatement
on the IoU of tests/_indoor_eval_ref.py; the argument checks of ``gga_multiclass_nms3d``."""
import ctypes as C
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from gga_amd import Config, _lib, build_model, synthetic
from gga_amd import loader as LD
from gga_amd.fcaf3d import DepthInstance3DBoxes
from gga_amd.indoor_datasets import Indoor3DDataset, S3DISDataset, ScanNetDataset, SUNRGBDDataset
from gga_amd.pipelines import GlobalAlignment, LoadPointsFromFile, NormalizePointsColor
from gga_amd.points import DepthPoints

import _indoor_eval_ref as R

sys.path.insert(0, os.path.join(REPO, 'tools_dev'))
SCANNET_CFG = os.path.join(REPO, 'configs', 'fcaf3d', 'fcaf3d_8x2_scannet-3d-18class.py')
S3DIS_CFG = os.path.join(REPO, 'configs', 'fcaf3d', 'fcaf3d_8x2_s3dis-3d-5class.py')
LOAD = dict(type='LoadPointsFromFile', coord_type='DEPTH', shift_height=False, use_color=True, load_dim=6, use_dim=[0, 1, 2, 3, 4, 5])
# The golden points come from the same torch CPU operations in the same order (a [n,3] @ [3,3] product, an add, a division).
# Bounds from the float32 rounding of those operations at the trees' magnitudes: an aligned coordinate is three products of
# |x| <= 8 and |r| <= 1 summed and shifted by |t| <= 3, each of the four roundings at most half an ulp of 16 (9.5e-7 each);
# a colour is one division (half an ulp of 1: 6e-8, relative).
ALIGN_ATOL, COLOUR_RTOL = 4e-6, 1.2e-7


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'indoor_datasets.npz'))


@pytest.fixture(scope='module')
def tree_sizes():
    from make_golden import INDOOR_TREE          # the sizes the golden run wrote its trees with
    return INDOOR_TREE


@pytest.fixture(scope='module')
def scannet_tree(tmp_path_factory, tree_sizes):
    root = str(tmp_path_factory.mktemp('scannet'))
    train, val = synthetic.write_scannet_tree(root, **tree_sizes['scannet'])
    return root, train, val


@pytest.fixture(scope='module')
def s3dis_tree(tmp_path_factory, tree_sizes):
    root = str(tmp_path_factory.mktemp('s3dis'))
    return root, synthetic.write_s3dis_tree(root, **tree_sizes['s3dis'])


# ----------------------------------------------------------------------------------------------------------------- configs
@pytest.mark.parametrize('path, n_classes', [(SCANNET_CFG, 18), (S3DIS_CFG, 5)])
def test_configs_equal_the_reference_and_build(path, n_classes):
    from make_golden import plain_config
    with open(os.path.join(GOLDEN, 'reference_configs_indoor.json')) as f:
        ref = json.load(f)['configs/fcaf3d/' + os.path.basename(path)]
    cfg = Config.fromfile(path)
    for key in ('model', 'optimizer', 'optimizer_config', 'lr_config', 'runner', 'custom_hooks', 'train_pipeline', 'test_pipeline',
                'checkpoint_config'):
        assert plain_config(cfg[key]) == ref[key], key
    assert cfg.data['samples_per_gpu'] == ref['data']['samples_per_gpu'] == 8
    assert plain_config(cfg.data['val']) == ref['data']['val'] and plain_config(cfg.data['test']) == ref['data']['test']
    assert cfg.evaluation == dict(interval=1)
    if n_classes == 18:
        assert plain_config(cfg.data) == ref['data']
    else:           # (the reference's merged train entry also carries the keys of the ScanNet dataset it was derived from)
        inner, want = cfg.data['train']['dataset'], ref['data']['train']['dataset']
        assert cfg.data['train']['times'] == ref['data']['train']['times'] == 13
        assert inner['type'] == want['type'] == 'ConcatDataset' and plain_config(inner['datasets']) == want['datasets']
        assert inner['separate_eval'] is want['separate_eval'] is False and len(inner['datasets']) == 5
    torch.manual_seed(0)
    model = build_model(cfg.model)
    assert tuple(model.head.conv_cls.kernel.shape) == (1, 128, n_classes)
    assert tuple(model.head.conv_reg.kernel.shape) == (1, 128, 6)
    assert model.head.test_cfg.nms_pre == 1000


# ---------------------------------------------------------------------------------------------------------------- datasets
def _check_against_golden(golden, tag, train, test, root, with_matrix):
    assert [str(c) for c in golden[f'{tag}.classes']] == list(train.CLASSES) and len(train) == int(golden[f'{tag}.n'])
    kept = []
    for i in range(len(train)):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ann, info, sample = train.get_ann_info(i), train.get_data_info(i), test.prepare_test_data(i)
        assert isinstance(ann['gt_bboxes_3d'], DepthInstance3DBoxes) and not ann['gt_bboxes_3d'].with_yaw and ann['gt_bboxes_3d'].box_dim == 7
        assert np.array_equal(ann['gt_bboxes_3d'].tensor.numpy(), golden[f'{tag}.{i}.boxes']), (tag, i)
        assert np.array_equal(ann['gt_labels_3d'], golden[f'{tag}.{i}.labels']) and ann['gt_labels_3d'].dtype == np.int64
        assert [os.path.relpath(ann[k], root) for k in ('pts_instance_mask_path', 'pts_semantic_mask_path')] == \
            [str(p) for p in golden[f'{tag}.{i}.mask_paths']]
        if with_matrix:
            assert ann['axis_align_matrix'].dtype == np.float32 and np.array_equal(ann['axis_align_matrix'], golden[f'{tag}.{i}.matrix'])
        else:
            assert 'axis_align_matrix' not in ann
        kept.append(info is not None)
        if info is not None:
            assert sorted(info) == [str(k) for k in golden[f'{tag}.{i}.info_keys']]
            assert os.path.relpath(info['pts_filename'], root) == str(golden[f'{tag}.{i}.pts_filename'])
            if with_matrix:
                assert info['sample_idx'] == str(golden[f'{tag}.{i}.sample_idx']) and info['file_name'] == info['pts_filename']
        assert sorted(k for k in sample if k != 'points') == [str(k) for k in golden[f'{tag}.{i}.test_keys']]
        got, want = sample['points'].tensor.numpy(), golden[f'{tag}.{i}.test_points']
        assert isinstance(sample['points'], DepthPoints) and sample['points'].attribute_dims == dict(color=[3, 4, 5])
        np.testing.assert_allclose(got[:, :3], want[:, :3], rtol=0, atol=ALIGN_ATOL)
        np.testing.assert_allclose(got[:, 3:], want[:, 3:], rtol=COLOUR_RTOL, atol=0)
    assert kept == golden[f'{tag}.kept'].tolist()
    return kept


def test_scannet_dataset_equals_the_reference(golden, scannet_tree):
    root, train, val = scannet_tree
    steps = [LOAD, dict(type='GlobalAlignment', rotation_axis=2), dict(type='NormalizePointsColor', color_mean=None)]
    ds_train, ds_test = ScanNetDataset(root, train, pipeline=steps), ScanNetDataset(root, val, pipeline=steps, test_mode=True)
    assert isinstance(ds_train, Indoor3DDataset) and issubclass(SUNRGBDDataset, Indoor3DDataset)
    assert len(ScanNetDataset.CLASSES) == 18 and ScanNetDataset.CLASSES == synthetic.SCANNET_CLASSES
    kept = _check_against_golden(golden, 'scannet', ds_train, ds_test, root, True)
    assert kept == [True, False, True, True]                      # frame 1 has no objects: filter_empty_gt drops it
    assert ds_train.prepare_train_data(1) is None and ScanNetDataset(root, train, filter_empty_gt=False).get_data_info(1) is not None
    # frame 2 was written without a matrix: the identity, with the reference's warning - in train and in test mode
    assert 'axis_align_matrix' not in ds_train.data_infos[2]['annos']
    with pytest.warns(UserWarning, match='axis_align_matrix is not found'):
        assert np.array_equal(ds_train.get_ann_info(2)['axis_align_matrix'], np.eye(4, dtype=np.float32))
    with pytest.warns(UserWarning, match='axis_align_matrix is not found'):
        ds_test.prepare_test_data(2)
    m = ds_train.get_ann_info(0)['axis_align_matrix']
    assert abs(m[0, 1]) > 0.1 and np.abs(m[:3, 3]).max() > 0.1           # a real rotation about z and a real shift
    assert 'ann_info' not in ds_test.get_data_info(0) and not hasattr(ds_test, 'flag') and (ds_train.flag == 0).all()
    with pytest.raises(NotImplementedError):
        ScanNetDataset(root, train, modality=dict(use_camera=True, use_depth=True)).get_data_info(0)
    with pytest.raises(NotImplementedError):
        ds_train.show([], None)
    with pytest.raises(NotImplementedError):
        ScanNetDataset(root, train, box_type_3d='LiDAR')
    with pytest.raises(AssertionError):
        ScanNetDataset(root, train, modality=dict(use_camera=False, use_lidar=True))


def test_s3dis_dataset_equals_the_reference(golden, s3dis_tree):
    root, paths = s3dis_tree
    assert sorted(paths) == golden['s3dis.areas'].tolist() and S3DISDataset.CLASSES == synthetic.S3DIS_CLASSES
    steps = [LOAD, dict(type='NormalizePointsColor', color_mean=None)]
    for area, path in paths.items():
        assert os.path.basename(path) == f's3dis_infos_Area_{area}.pkl'
        kept = _check_against_golden(golden, f's3dis{area}', S3DISDataset(root, path, pipeline=steps),
                                     S3DISDataset(root, path, pipeline=steps, test_mode=True), root, False)
        assert kept == [True, area != 1]                            # room (1, 1) has no objects
    ds = S3DISDataset(root, paths[1])
    assert ds.modality is None and set(ds.get_data_info(0)) == {'pts_filename', 'ann_info'}
    assert ds.get_ann_info(1)['gt_bboxes_3d'].tensor.shape == (0, 7)


def _with_tree(cfg_path, root, n_points):
    cfg = Config.fromfile(cfg_path)

    def walk(node):
        if isinstance(node, dict):
            if node.get('type') == 'PointSample':
                node['num_points'] = n_points
            if 'data_root' in node:
                node['ann_file'] = os.path.join(root, os.path.basename(node['ann_file']))
                node['data_root'] = root
            for v in node.values():
                walk(v)
        elif isinstance(node, (list, tuple)):
            for v in node:
                walk(v)

    walk(cfg.data)
    return cfg


def test_a_train_sample_through_the_full_pipeline(scannet_tree, s3dis_tree):
    np.random.seed(5)
    ds = LD.build_dataset(_with_tree(SCANNET_CFG, scannet_tree[0], 150).data['train'])
    assert isinstance(ds, LD.RepeatDataset) and len(ds) == 10 * 4 and isinstance(ds.dataset, ScanNetDataset)
    sample = ds[0]
    assert set(sample) == {'img_metas', 'points', 'gt_bboxes_3d', 'gt_labels_3d'}
    pts, boxes, labels = sample['points'].data, sample['gt_bboxes_3d'].data, sample['gt_labels_3d'].data
    n_gt = ds.dataset.data_infos[0]['annos']['gt_num']
    assert pts.shape == (150, 6) and pts.dtype == torch.float32 and 0 <= float(pts[:, 3:].min()) and float(pts[:, 3:].max()) <= 1
    assert isinstance(boxes, DepthInstance3DBoxes) and boxes.tensor.shape == (n_gt, 7) and not boxes.with_yaw
    assert labels.shape == (n_gt,) and labels.dtype == torch.long
    # the boxes moved with the points: the object points (half of the scene) still lie in the augmented, enclosing boxes
    lo, hi = boxes.tensor[:, :3] - boxes.tensor[:, 3:6] * torch.tensor([.5, .5, 0]), boxes.tensor[:, :3] + boxes.tensor[:, 3:6] * torch.tensor([.5, .5, 1])
    inside = ((pts[:, None, :3] >= lo - 1e-4) & (pts[:, None, :3] <= hi + 1e-4)).all(-1).any(-1)
    assert inside.float().mean() > 0.35
    meta = sample['img_metas'].data
    assert meta['box_type_3d'] is DepthInstance3DBoxes and 'pcd_rotation' in meta and meta['transformation_3d_flow'][-3:] == ['R', 'S', 'T']
    # the test split: every key a list over augmentations, the points aligned and normalised
    test = LD.build_dataset(_with_tree(SCANNET_CFG, scannet_tree[0], 150).data['test'])
    one = test[0]
    assert set(one) == {'img_metas', 'points'} and one['points'][0].data.shape == (150, 6) and float(one['points'][0].data[:, 3:].max()) <= 1
    s3 = LD.build_dataset(_with_tree(S3DIS_CFG, s3dis_tree[0], 150).data['test'])
    assert isinstance(s3, S3DISDataset) and len(s3) == 2 and s3[0]['points'][0].data.shape == (150, 6)


# ------------------------------------------------------------------------------------------------------------ pipeline steps
def test_global_alignment_and_colour_normalisation_equal_the_reference(golden, scannet_tree):
    """Observed on the CPU: the largest difference to the reference's output is 0 for the aligned coordinates and 0 for the
    colours, with and without a colour mean (the same float32 operations in the same order)."""
    root = scannet_tree[0]
    path = os.path.join(root, 'points', 'scene0000_00.bin')
    load = LoadPointsFromFile(**{k: v for k, v in LOAD.items() if k != 'type'})
    d = load(dict(pts_filename=path))
    assert np.array_equal(d['points'].tensor.numpy(), golden['align.in']) and d['points'].attribute_dims == dict(color=[3, 4, 5])
    assert np.array_equal(d['points'].color.numpy(), golden['align.in'][:, 3:]) and float(d['points'].color.max()) > 200
    d['ann_info'] = dict(axis_align_matrix=golden['align.matrix'])
    out = GlobalAlignment(rotation_axis=2)(d)['points'].tensor.numpy()
    print('alignment: max |difference|', np.abs(out - golden['align.out']).max())
    np.testing.assert_allclose(out[:, :3], golden['align.out'][:, :3], rtol=0, atol=ALIGN_ATOL)
    assert np.array_equal(out[:, 3:], golden['align.in'][:, 3:])                 # colours untouched
    # what the step computes: rows times R^T, plus t
    m = golden['align.matrix'].astype(np.float64)
    np.testing.assert_allclose(out[:, :3], golden['align.in'][:, :3].astype(np.float64) @ m[:3, :3].T + m[:3, 3], atol=1e-5)
    for mean, key in ((None, 'color.out'), (golden['color.mean'].tolist(), 'color.out_mean')):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                                     # (colours below the mean: the setter's range warning)
            got = NormalizePointsColor(color_mean=mean)(load(dict(pts_filename=path)))['points'].tensor.numpy()
        print(key, 'max |difference|', np.abs(got - golden[key]).max())
        np.testing.assert_allclose(got[:, 3:], golden[key][:, 3:], rtol=COLOUR_RTOL, atol=0)
        assert np.array_equal(got[:, :3], golden['align.in'][:, :3])
    assert repr(GlobalAlignment(2)) == 'GlobalAlignment(rotation_axis=2)' and repr(NormalizePointsColor(None)) == 'NormalizePointsColor(color_mean=None)'


def test_invalid_matrices_and_missing_colour_are_refused(scannet_tree):
    path = os.path.join(scannet_tree[0], 'points', 'scene0000_00.bin')
    plain = LoadPointsFromFile(coord_type='DEPTH', load_dim=6, use_dim=[0, 1, 2, 3, 4, 5])
    with pytest.raises(AssertionError, match='Expect points have color attribute'):
        NormalizePointsColor(None)(plain(dict(pts_filename=path)))
    with pytest.raises(AssertionError):
        LoadPointsFromFile(coord_type='DEPTH', load_dim=6, use_dim=[0, 1, 2], use_color=True)(dict(pts_filename=path))
    align = GlobalAlignment(rotation_axis=2)
    c, s = np.cos(0.4), np.sin(0.4)
    tilt = np.eye(4, dtype=np.float32)
    tilt[:3, :3] = [[1, 0, 0], [0, c, -s], [0, s, c]]                           # a rotation, but about x
    mirror = np.diag([1, -1, 1, 1]).astype(np.float32)                          # determinant -1
    for bad in (tilt, mirror):
        with pytest.raises(AssertionError, match='invalid rotation matrix'):
            align(dict(plain(dict(pts_filename=path)), ann_info=dict(axis_align_matrix=bad)))
    with pytest.raises(AssertionError, match='invalid shape'):
        align(dict(plain(dict(pts_filename=path)), ann_info=dict(axis_align_matrix=np.eye(3, dtype=np.float32))))
    with pytest.raises(AssertionError, match='not provided'):
        align(dict(plain(dict(pts_filename=path)), ann_info=dict()))
    # points without colour gain the columns through the setter
    p = DepthPoints(torch.zeros(4, 3), points_dim=3)
    assert p.color is None
    p.color = np.full((4, 3), 7.0)
    assert p.tensor.shape == (4, 6) and p.points_dim == 6 and p.attribute_dims == dict(color=[3, 4, 5]) and float(p.color.sum()) == 84
    with pytest.raises(ValueError):
        p.color = np.zeros((4, 2))


def test_depth_boxes_move_with_the_points():
    yawed = DepthInstance3DBoxes(torch.tensor([[1., 2, 0, 2, 1, 1, 0.3]]))
    flat = DepthInstance3DBoxes(torch.tensor([[1., 2, 0, 2, 1, 1]]), box_dim=6, with_yaw=False)
    a = 0.5
    rot_t = torch.tensor([[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=torch.float32)
    for b in (yawed, flat):
        b.rotate(rot_t)
        torch.testing.assert_close(b.tensor[0, :2], torch.tensor([1 * np.cos(a) - 2 * np.sin(a), 1 * np.sin(a) + 2 * np.cos(a)], dtype=torch.float32))
    assert float(yawed.tensor[0, 6]) == pytest.approx(0.8) and torch.equal(yawed.tensor[0, 3:6], torch.tensor([2., 1, 1]))
    # the axis-aligned box that encloses the turned one
    torch.testing.assert_close(flat.tensor[0, 3:5], torch.tensor([2 * np.cos(a) + np.sin(a), 2 * np.sin(a) + np.cos(a)], dtype=torch.float32))
    assert float(flat.tensor[0, 6]) == 0
    flat.flip('horizontal'), flat.scale(2.0), flat.translate([1, 1, 1])
    yawed.flip('horizontal'), yawed.flip('vertical')
    assert float(yawed.tensor[0, 6]) == pytest.approx(0.8 - np.pi) and float(flat.tensor[0, 5]) == 2 and float(flat.tensor[0, 2]) == 1


# ------------------------------------------------------------------------------------------------------------ ConcatDataset
def test_concat_dataset(s3dis_tree):
    root, paths = s3dis_tree
    cfg = _with_tree(S3DIS_CFG, root, 100)
    inner = cfg.data['train']['dataset']
    inner['datasets'] = [d for d in inner['datasets'] if d['ann_file'].endswith(('Area_1.pkl', 'Area_2.pkl'))]
    cfg.data['train']['times'] = 3
    rep = LD.build_dataset(cfg.data['train'])
    cat = rep.dataset
    assert isinstance(rep, LD.RepeatDataset) and isinstance(cat, LD.ConcatDataset) and cat.separate_eval is False
    assert len(cat) == 4 and len(rep) == 12 and cat.cumulative_sizes == [2, 4] and tuple(cat.CLASSES) == S3DISDataset.CLASSES == tuple(rep.CLASSES)
    assert cat.flag.shape == (4,) and cat.flag.dtype == np.uint8 and rep.flag.shape == (12,)
    # item routing: index 2 is room 0 of the second area (room (1, 1) is empty and would be redrawn)
    np.random.seed(0)
    for idx, (which, room) in {0: (0, 0), 2: (1, 0), 3: (1, 1), -1: (1, 1), 6: (1, 0)}.items():
        sample = (rep if idx == 6 else cat)[idx]
        want = cat.datasets[which].data_infos[room]
        assert sample['img_metas'].data['pts_filename'] == os.path.join(root, want['pts_path']), idx
        assert len(sample['gt_labels_3d'].data) == want['annos']['gt_num']
    with pytest.raises(ValueError):
        cat[-5]
    with pytest.raises(NotImplementedError):
        cat.evaluate([])
    assert len(LD.ConcatDataset([cat.datasets[0]])) == 2
    with pytest.raises(NotImplementedError):
        LD.build_dataset(dict(type='CBGSDataset', dataset=dict()))


# ------------------------------------------------------------------------------------------------------------------ evaluate
def _average_precision64(rec, prec):
    """Area under the precision envelope (indoor_eval.py ``average_precision``, mode 'area') in float64."""
    mrec, mpre = np.concatenate([[0.0], rec, [1.0]]), np.concatenate([[0.0], prec, [0.0]])
    for i in range(len(mpre) - 1, 0, -1):
        mpre[i - 1] = max(mpre[i - 1], mpre[i])
    ind = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[ind + 1] - mrec[ind]) * mpre[ind + 1]))


def _evaluate64(gt_boxes, gt_labels, dets, thresholds, class_names):
    """The indoor protocol in float64 on ``R.iou3d64``: per class the detections of all frames by descending score; one is a
    true positive when its best ground truth of that class in its frame overlaps by more than the threshold and is not taken.
    -> (ret_dict in the reference's key order, the smallest distance of a best IoU to a threshold)."""
    order = []          # the reference's dictionaries meet the classes frame by frame: a frame's detections first, then its ground truths
    for (_, _, det_labels), lab in zip(dets, gt_labels):
        for c in list(det_labels) + list(lab):
            if int(c) not in order:
                order.append(int(c))
    ret, margin = {}, np.inf
    for thr in thresholds:
        aps, recs = {}, {}
        for c in order:
            items = sorted(((float(s), f, b) for f, (bs, ss, ls) in enumerate(dets) for b, s, l in zip(bs, ss, ls) if int(l) == c), key=lambda t: -t[0])
            taken = {f: np.zeros(int((lab == c).sum()), bool) for f, lab in enumerate(gt_labels)}
            n_gt = sum(len(v) for v in taken.values())
            tp = np.zeros(len(items))
            for k, (_, f, b) in enumerate(items):
                v = np.array([R.iou3d64(b, g) for g in gt_boxes[f][gt_labels[f] == c]])
                if len(v):
                    j = int(np.argmax(v))
                    margin = min(margin, abs(v[j] - thr))
                    if v[j] > thr and not taken[f][j]:
                        taken[f][j] = True
                        tp[k] = 1
            ctp, cfp = np.cumsum(tp), np.cumsum(1 - tp)
            rec, prec = ctp / n_gt, ctp / np.maximum(ctp + cfp, np.finfo(np.float64).eps)
            aps[c], recs[c] = _average_precision64(rec, prec) if len(items) else 0.0, rec[-1] if len(items) else 0.0
        for c in order:
            ret[f'{class_names[c]}_AP_{thr:.2f}'] = aps[c]
        ret[f'mAP_{thr:.2f}'] = float(np.mean(list(aps.values())))
        for c in order:
            ret[f'{class_names[c]}_rec_{thr:.2f}'] = recs[c]
        ret[f'mAR_{thr:.2f}'] = float(np.mean(list(recs.values())))
    return ret, margin


EVAL_SEED = 78          # a seed for which no best IoU lies within R.MARGIN of a threshold (asserted below)


def test_scannet_evaluate_equals_the_float64_protocol(tmp_path):
    root = str(tmp_path)
    _, val = synthetic.write_scannet_tree(root, 16, n_points=20)
    ds = ScanNetDataset(root, val, test_mode=True)
    rng = np.random.default_rng(EVAL_SEED)
    gt_boxes, gt_labels, dets, results = [], [], [], []
    for i in range(len(ds)):
        ann = _quiet(ds.get_ann_info, i)
        g, lab = ann['gt_bboxes_3d'].tensor.numpy(), ann['gt_labels_3d']
        # detections: every ground truth twice, jittered (weakly and strongly), axis-aligned, with its class; some with another class
        src = np.concatenate([np.arange(len(g)), np.arange(len(g))])
        b = g[src].astype(np.float64)
        b[:, :6] += rng.normal(0, 1, (len(src), 6)) * np.array([.12, .12, .05, .1, .1, .05]) * rng.uniform(0.1, 2.0, (len(src), 1))
        b[:, 3:6] = np.maximum(b[:, 3:6], 0.1)
        l = lab[src].copy()
        wrong = rng.random(len(src)) < 0.15
        l[wrong] = (l[wrong] + 1) % 18
        b, s = b.astype(np.float32), rng.uniform(0.05, 1, len(src)).astype(np.float32)
        gt_boxes.append(g), gt_labels.append(lab), dets.append((b, s, l))
        results.append(dict(boxes_3d=DepthInstance3DBoxes(torch.from_numpy(b[:, :6].copy()), box_dim=6, with_yaw=False, origin=(.5, .5, 0)),
                            scores_3d=torch.from_numpy(s), labels_3d=torch.from_numpy(l)))
    assert len({int(c) for lab in gt_labels for c in lab}) == 18
    want, margin = _evaluate64(gt_boxes, gt_labels, dets, R.THRESHOLDS, ScanNetDataset.CLASSES)
    assert margin > R.MARGIN, margin                      # no best IoU near a threshold: float32 and float64 decide alike
    lines = []
    ret = ds.evaluate(results, logger=lines.append, device='cpu')
    assert len(ret) == 18 * 2 * 2 + 4 and list(ret) == list(want)
    got, exp = np.array(list(ret.values())), np.array(list(want.values()))
    print('evaluate: max |difference| to float64', np.abs(got - exp).max())
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-6)          # values in [0, 1] carried in float32 (half an ulp: 6e-8), summed over < 20 recall steps
    assert 0.2 < ret['mAP_0.25'] < 1 and ret['mAP_0.50'] < ret['mAP_0.25'] and 'Overall' in lines[0]
    out, tmp = ds.format_results(results)
    assert out is results and os.path.exists(os.path.join(tmp.name, 'results.pkl'))
    with pytest.raises(AssertionError):
        ds.evaluate([np.zeros((0, 5))] * len(ds))


def _quiet(fn, *args):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return fn(*args)


# ------------------------------------------------------------------------------------------------- the new entry point's checks
def test_multiclass_nms3d_argument_validation_without_gpu():
    L = _lib.lib()
    assert L.gga_abi_version() == _lib.ABI_VERSION >= 36 and _lib.MULTICLASS_NMS_MAX_CLASSES >= 64
    some = C.c_void_p(64)          # never dereferenced: every call below is refused before a launch

    def rejected(boxes=some, scores=some, scene=some, n=4, nc=3, ns=2, rows=some, classes=some, count=some, ws=some, ws_bytes=1 << 30):
        rc = L.gga_multiclass_nms3d(boxes, scores, scene, n, nc, ns, 0.1, 0.5, rows, classes, count, ws, ws_bytes, None)
        msg = L.gga_last_error().decode()
        assert rc == -1 and msg.startswith('gga_multiclass_nms3d:'), (rc, msg)
        return msg

    assert 'bad sizes' in rejected(n=-1)
    for nc in (0, -2, _lib.MULTICLASS_NMS_MAX_CLASSES + 1):
        assert 'bad sizes' in rejected(nc=nc)
    for ns in (0, -1):
        assert 'bad sizes' in rejected(ns=ns)
    assert 'bad sizes' in rejected(n=1 << 30, nc=4)                 # n * classes >= 2^31
    for name in ('boxes', 'scores', 'scene', 'rows', 'classes', 'ws'):
        assert 'null pointer' in rejected(**{name: None})
    assert 'out_count' in rejected(count=None) and 'out_count' in rejected(count=None, n=0)
    need = L.gga_multiclass_nms3d_workspace_bytes(4, 3, 2)
    assert need > 0 and 'workspace' in rejected(ws_bytes=need - 1) and 'workspace' in rejected(ws_bytes=0)
    assert L.gga_multiclass_nms3d_workspace_bytes(-1, 3, 2) == 0 and L.gga_multiclass_nms3d_workspace_bytes(4, 0, 2) == 0
    assert L.gga_multiclass_nms3d_workspace_bytes(4, 3, 0) == 0 and L.gga_multiclass_nms3d_workspace_bytes(0, 3, 2) > 0
    assert L.gga_multiclass_nms3d_workspace_bytes(8000, 18, 8) > L.gga_multiclass_nms3d_workspace_bytes(4000, 18, 8)


def test_functional_wrapper_refuses_cpu_tensors_and_bad_shapes():
    from gga_amd import functional as F
    with pytest.raises(RuntimeError, match='GPU only'):
        F.multiclass_nms3d(torch.zeros(4, 7), torch.zeros(4, 3), torch.zeros(4, dtype=torch.long), 2, 0.1, 0.5)
