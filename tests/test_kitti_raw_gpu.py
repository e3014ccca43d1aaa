"""Step 1 of the recipe on the device, from a raw KITTI tree (``synthetic.write_kitti_raw_tree``): the one-pass per-frame
point stage against the per-call form (``GGA_PREP_ONE_PASS=0``), and ``tools/create_data_gga.py`` end to end.

Seeds: tree seed 7100 (frame i is ``make_rga_scene(7100 + i)``) with ``seed=0`` for the ground fit (frame i draws from
``np.random.seed(i)``). On these frames the per-call ``calculate_rga`` runs to its end - neither the ``NameError`` (no ground
plane accepted) nor the ``IndexError`` (first non-empty region not at the smallest threshold) path that the function shares
with the reference is met; the choice was checked beforehand with the CPU oracle's region growing, ground fit and polyhedron
test standing in for the kernels."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from gga_amd import synthetic

pytestmark = pytest.mark.gpu

TREE = dict(n_train=4, n_val=2, n_test=2, seed=7100, n_points=3000)
FILES = ['kitti_infos_train_GGA.pkl', 'kitti_infos_val_GGA.pkl', 'kitti_infos_trainval_GGA.pkl', 'kitti_infos_test.pkl',
         'kitti_dbinfos_train_GGA.pkl']


def _equal(a, b, where=''):
    """Nested dicts / lists / arrays / scalars: same structure, dtypes, shapes and bits."""
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _equal(a[k], b[k], f'{where}.{k}')
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, f'{where}[{i}]')
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    else:
        assert a == b, where


def _bins(root, sub):
    d = os.path.join(root, sub)
    return {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}


def _prepare(root):
    from gga_amd import gt_database as GD
    from gga_amd import kitti_converter as KC
    quiet = lambda s: None
    ids = synthetic.write_kitti_raw_tree(root, **TREE)
    KC.create_kitti_info_file(root, 'kitti', seed=0, logger=quiet)
    KC.create_reduced_point_cloud(root, 'kitti')
    GD.create_groundtruth_database('KittiDataset_GGA', root, 'kitti', info_path=os.path.join(root, 'kitti_infos_train_GGA.pkl'),
                                   logger=quiet)
    return ids


def test_one_pass_driver_equals_the_per_call_driver(tmp_path, monkeypatch):
    from oracle import oracle as O
    one, per_call = str(tmp_path / 'one_pass'), str(tmp_path / 'per_call')
    monkeypatch.delenv('GGA_PREP_ONE_PASS', raising=False)
    ids = _prepare(one)
    monkeypatch.setenv('GGA_PREP_ONE_PASS', '0')
    _prepare(per_call)
    for name in FILES:
        a, b = (pickle.load(open(os.path.join(r, name), 'rb')) for r in (one, per_call))
        _equal(a, b, name)
    infos = pickle.load(open(os.path.join(one, 'kitti_infos_trainval_GGA.pkl'), 'rb'))
    assert [i['image']['image_idx'] for i in infos] == ids['train'] + ids['val']
    grown = sum(len(p) for i in infos for p in i['annos']['GGA_in_box_points'])
    assert grown > 500 and sum(int(i['annos']['GGA_mask_valid'].sum()) for i in infos) >= 10       # clusters grew
    assert all(i['annos']['num_points_in_gt'].dtype == np.int32 for i in infos)
    empty = [i for i in infos if i['image']['image_idx'] == 1][0]['annos']                          # only a DontCare line
    assert empty['num_points_in_gt'].tolist() == [-1] and empty['GGA_boxes_img'].shape == (1, 4) and empty['GGA_in_box_points'][0].size == 0
    for split, n in (('training', 6), ('testing', 2)):
        a, b = _bins(one, f'{split}/velodyne_reduced'), _bins(per_call, f'{split}/velodyne_reduced')
        assert len(a) == n and a == b
    a, b = _bins(one, 'kitti_gt_database_GGA'), _bins(per_call, 'kitti_gt_database_GGA')
    assert len(a) >= 8 and a == b and sum(len(v) for v in a.values()) > 0
    # the reduced clouds are the points inside the image frustum, by the CPU oracle, in file order
    tests = pickle.load(open(os.path.join(one, 'kitti_infos_test.pkl'), 'rb'))
    assert all('annos' in i for i in infos) and not any('annos' in i for i in tests) and len(tests) == 2
    for info in infos + tests:
        pts = np.fromfile(os.path.join(one, info['point_cloud']['velodyne_path']), np.float32).reshape(-1, 4)
        c, shape = info['calib'], info['image']['image_shape']
        inside = O.points_in_frustm_indices(pts.astype(np.float64), c['R0_rect'], c['Tr_velo_to_cam'], c['P2'], [0, 0, shape[1], shape[0]])
        want = pts[inside.reshape(-1)]
        rel = info['point_cloud']['velodyne_path'].replace('velodyne', 'velodyne_reduced')
        assert 0 < len(want) < len(pts) and open(os.path.join(one, rel), 'rb').read() == want.tobytes()


def test_create_data_tool_end_to_end(tmp_path):
    root = str(tmp_path / 'kitti')
    synthetic.write_kitti_raw_tree(root, **TREE)
    env = {k: v for k, v in os.environ.items() if k != 'GGA_PREP_ONE_PASS'}
    cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.join(REPO, 'tools', 'create_data_gga.py'), 'kitti', '--root-path', root,
           '--out-dir', root, '--seed', '0']
    done = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    for name in FILES + [f'kitti_infos_{s}_mono3d.coco.json' for s in ('train_GGA', 'val_GGA', 'trainval_GGA', 'test')]:
        assert os.path.getsize(os.path.join(root, name)) > 0, name
    assert len(os.listdir(os.path.join(root, 'training', 'velodyne_reduced'))) == 6
    assert len(os.listdir(os.path.join(root, 'testing', 'velodyne_reduced'))) == 2
    assert len(os.listdir(os.path.join(root, 'kitti_gt_database_GGA'))) >= 8
    import json
    coco = json.load(open(os.path.join(root, 'kitti_infos_trainval_GGA_mono3d.coco.json')))
    assert len(coco['images']) == 6 and len(coco['annotations']) >= 10
    assert json.load(open(os.path.join(root, 'kitti_infos_test_mono3d.coco.json')))['annotations'] == []
    # the train dataset of configs/gga/gga_kitti_config.py on this root: the reference's train_pipeline, database sampling included
    from gga_amd import Config
    from gga_amd import loader as LD
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_config.py'))
    d = cfg.data['train']
    d['dataset'].update(data_root=root + '/', ann_file=os.path.join(root, 'kitti_infos_trainval_GGA.pkl'))
    assert d['dataset']['pts_prefix'] == 'velodyne_reduced'
    for t in d['dataset']['pipeline']:
        if t['type'] == 'ObjectSample_GGA':
            t['db_sampler'].update(data_root=root + '/', info_path=os.path.join(root, 'kitti_dbinfos_train_GGA.pkl'))
    ds = LD.build_dataset(d)
    np.random.seed(0), torch.manual_seed(0)
    sample = ds[0]
    own = pickle.load(open(os.path.join(root, 'kitti_infos_trainval_GGA.pkl'), 'rb'))[0]['annos']
    assert len(sample['gt_labels_3d'].data) > int(own['GGA_mask_valid'].sum())             # database objects were pasted
    batch = LD.collate([sample], samples_per_gpu=1)
    assert {'points', 'gt_bboxes_3d', 'gt_labels_3d', 'GGA_boxes_img', 'GGA_in_box_points'} <= set(batch)
    # a second run with --resume rewrites no per-frame pickle
    split = os.path.join(root, 'kitti_GGA_split_file')
    before = {f: os.stat(os.path.join(split, f)).st_mtime_ns for f in os.listdir(split)}
    assert len(before) == 6
    done = subprocess.run(cmd + ['--resume'], env=env, capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert before == {f: os.stat(os.path.join(split, f)).st_mtime_ns for f in os.listdir(split)}
