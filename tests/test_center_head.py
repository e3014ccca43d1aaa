"""Supervised CenterPoint on KITTI infos, the parts that need no device: registry names and the two configs, the option
checks of ``CenterHead``, ``KittiDataset`` on a pseudo-label-style and on a GGA info list, the host half of ``get_targets``,
and the box side of ``GlobalRotScaleTrans`` / ``RandomFlip3D``."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from gga_amd import Config, build_model
from gga_amd import loader as LD
from gga_amd.box3d import LiDARInstance3DBoxes
from gga_amd.datasets import camera_boxes_to_lidar
from gga_amd.pipelines import Compose
from gga_amd.points import LiDARPoints
from gga_amd.registry import DATASETS, DETECTORS, HEADS, PIPELINES, build_head

RETRAIN = os.path.join(REPO, 'configs', 'gga', 'gga_kitti_retrain_centerpoint.py')
SUPERVISED = os.path.join(REPO, 'configs', 'gga', 'gga_kitti_supervised_centerpoint.py')
GGA = os.path.join(REPO, 'configs', 'gga', 'gga_kitti_config.py')
CLASSES = ['Pedestrian', 'Cyclist', 'Car']


def gga_infos():
    return pickle.load(open(os.path.join(GOLDEN, 'gt_database_infos.pkl'), 'rb'))


def pseudo_infos():
    """The info list a pseudo-label run writes: the same frames, ``annos`` without any ``GGA_*`` field and without the
    DontCare entries (gga_amd.pseudo_labels.pseudo_label_matching_kitti)."""
    out = []
    for info in gga_infos():
        info = copy.deepcopy(info)
        annos = info['annos']
        keep = np.array([n != 'DontCare' for n in annos['name']])
        info['annos'] = {k: v[keep] for k, v in annos.items() if not k.startswith('GGA_')}
        out.append(info)
    return out


# ----------------------------------------------------------------------------- registry and configs
def test_registry_names():
    assert HEADS.get('CenterHead') is not None and DETECTORS.get('CenterPoint') is not None
    assert DATASETS.get('KittiDataset') is not None
    assert PIPELINES.get('ObjectRangeFilter') is not None and PIPELINES.get('ObjectNameFilter') is not None


@pytest.mark.parametrize('path,ann', [(RETRAIN, 'data/kitti/kitti_infos_trainval_GGA_pseudo.pkl'),
                                      (SUPERVISED, 'data/kitti/kitti_infos_train_GGA.pkl')])
def test_configs_build(path, ann, tmp_path):
    """Fails without the feature: ``CenterHead`` is not registered."""
    cfg = Config.fromfile(path)
    assert cfg.model['type'] == 'CenterPoint' and cfg.model['pts_bbox_head']['type'] == 'CenterHead'
    assert list(cfg.model['train_cfg']['pts']['code_weights']) == [1.0] * 8
    assert cfg.data['train']['dataset']['ann_file'] == ann and cfg.data['val']['ann_file'] == 'data/kitti/kitti_infos_val_GGA.pkl'
    model = build_model(cfg.model)
    assert type(model).__name__ == 'CenterPoint' and type(model.pts_bbox_head).__name__ == 'CenterHead'
    # the same parameters and buffers, under the same names, as the GGA model on this trunk
    gga = build_model(Config.fromfile(GGA).model)
    assert list(model.state_dict()) == list(gga.state_dict())
    assert [tuple(v.shape) for v in model.state_dict().values()] == [tuple(v.shape) for v in gga.state_dict().values()]
    # datasets and pipelines (the info lists stand in for the files)
    train = copy.deepcopy(cfg.data['train'])
    train['dataset'].update(ann_file=pseudo_infos(), data_root=str(tmp_path))
    ds = LD.build_dataset(train)
    assert type(ds.dataset).__name__ == 'KittiDataset' and len(ds) == 3 and ds.CLASSES == tuple(CLASSES)
    names = [type(t).__name__ for t in ds.dataset.pipeline.transforms]
    assert 'ObjectRangeFilter' in names and 'ObjectNameFilter' in names and not any('ObjectSample' in n or 'ObjectNoise' in n for n in names)
    val = LD.build_dataset(dict(copy.deepcopy(cfg.data['val']), ann_file=gga_infos(), data_root=str(tmp_path)))
    assert type(val).__name__ == 'KittiDataset' and val.test_mode and hasattr(val, 'evaluate') and hasattr(val, 'format_results')


def head_cfg(**over):
    cfg = copy.deepcopy(Config.fromfile(RETRAIN).model['pts_bbox_head'])
    cfg = dict(cfg, train_cfg=Config.fromfile(RETRAIN).model['train_cfg']['pts'], test_cfg=None)
    cfg.update(over)
    return cfg


def test_refused_options_say_why():
    heads = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2))
    with pytest.raises(AssertionError, match='with_velocity'):
        build_head(head_cfg(common_heads=dict(heads, vel=(2, 2))))
    with pytest.raises(AssertionError, match='norm_bbox'):
        build_head(head_cfg(norm_bbox=False))
    with pytest.raises(NotImplementedError, match="CenterHead: loss_bbox.reduction='none'"):
        build_head(head_cfg(loss_bbox=dict(type='L1Loss', reduction='none', loss_weight=0.25)))
    with pytest.raises(NotImplementedError, match="loss_cls.reduction='sum'"):
        build_head(head_cfg(loss_cls=dict(type='GaussianFocalLoss', reduction='sum')))
    with pytest.raises(TypeError):                     # a key of the GGA head only (centerpoint_head.py:274-292 has none)
        build_head(head_cfg(loss_center=dict(type='MarginL1Loss', reduction='mean')))
    head = build_head(head_cfg())
    tc = dict(head.train_cfg, code_weights=[0.5] * 5)
    head.train_cfg = tc
    with pytest.raises(ValueError, match='8 entries'):
        head.loss_from_targets([[dict()]], [None], [None], [None], [None])


def test_gga_head_is_what_it_was():
    """The common base moved no parameter and changed no message of ``CenterHead_GGA``."""
    gga = Config.fromfile(GGA).model
    cfg = dict(copy.deepcopy(gga['pts_bbox_head']), train_cfg=gga['train_cfg']['pts'], test_cfg=gga['test_cfg']['pts'])
    head = build_head(cfg)
    assert type(head).__name__ == 'CenterHead_GGA' and head.pal_backprop is False
    assert list(head.state_dict())[:3] == ['shared_conv.conv.weight', 'shared_conv.bn.weight', 'shared_conv.bn.bias']
    for name in ('get_targets', 'pack_targets', 'loss', 'loss_from_targets', 'get_bboxes', 'forward_single', 'draw_srl'):
        assert callable(getattr(head, name))
    with pytest.raises(AssertionError, match='GGA does not support velocity'):
        build_head(dict(cfg, common_heads=dict(cfg['common_heads'], vel=(2, 2))))
    with pytest.raises(NotImplementedError, match='CenterHead_GGA: loss_bbox.reduction'):
        build_head(dict(cfg, loss_bbox=dict(type='L1Loss', reduction='none')))


def test_entry_points_validate_without_gpu():
    import ctypes as C
    from gga_amd import _lib
    from gga_amd import functional as F
    L = _lib.lib()
    p = 4096                    # a non-null, aligned stand-in for a device pointer: nothing here dereferences it
    tc = Config.fromfile(RETRAIN).model['train_cfg']['pts']
    prm = F.center_params(tc, [1, 1, 1])
    assert (prm.K, prm.H, prm.W, prm.n_tasks, prm.n_classes) == (500, 200, 176, 3, 3)
    assert list(prm.class_task)[:3] == [0, 1, 2] and list(prm.class_index)[:3] == [0, 0, 0]
    prm2 = F.center_params(dict(tc), [2, 1])
    assert list(prm2.class_task)[:3] == [0, 0, 1] and list(prm2.class_index)[:3] == [0, 1, 0] and list(prm2.task_class_base)[:2] == [0, 2]

    def targets(prm, B=2, max_radius=16, boxes=p):
        return L.gga_center_targets(boxes, p, p, B, C.byref(prm) if prm is not None else None, p, p, p, p, p, p, max_radius, None)

    def refused(word):
        msg = L.gga_last_error().decode()
        return msg.startswith('gga_center_targets:') and word in msg

    assert targets(None) == -1 and refused('null params')
    assert targets(prm, B=0) == -1 and refused('B 0')
    assert targets(prm, boxes=None) == -1 and refused('null pointer')
    assert targets(prm, max_radius=1) == -1 and refused('max_radius')
    bad = copy.deepcopy(prm)
    bad.K = _lib.CENTER_MAX_K + 1
    assert targets(bad) == -1 and refused('K 513')
    bad = copy.deepcopy(prm)
    bad.class_task[1] = 7
    assert targets(bad) == -1 and refused('outside the table')
    bad = copy.deepcopy(prm)
    bad.task_classes[0] = 2
    assert targets(bad) == -1 and refused('task 1')
    w = F.center_loss_weights([1.0] * 8, 0.25)
    with pytest.raises(ValueError, match='8 entries'):
        F.center_loss_weights([1.0] * 5, 0.25)
    for name in ('gga_center_reg_loss_fwd', 'gga_center_reg_loss_bwd'):
        fn = getattr(L, name)
        assert fn(None, 2, 4, C.byref(w), None) == -1 and L.gga_last_error().decode().startswith(name + ': null task table')
        tb = _lib.CenterLossTable()
        for n in (0, _lib.MAX_TASKS + 1):
            tb.n_tasks = n
            assert fn(C.byref(tb), 2, 4, C.byref(w), None) == -1
            assert L.gga_last_error().decode().startswith(f'{name}: n_tasks {n} not in 1..{_lib.MAX_TASKS}')
        tb.n_tasks = 1
        assert fn(C.byref(tb), 2, 4, C.byref(w), None) == -1 and 'null pointer (task 0)' in L.gga_last_error().decode()
        assert fn(C.byref(tb), 0, 4, C.byref(w), None) == -1 and 'bad B' in L.gga_last_error().decode()


def test_pack_targets_is_flat_and_bounds_the_radius():
    head = build_head(head_cfg())
    boxes = [LiDARInstance3DBoxes(torch.tensor([[10., 1., -1., 3.9, 1.6, 1.5, 0.3], [20., -3., -1., 0.8, 0.6, 1.7, 1.0]])),
             LiDARInstance3DBoxes(torch.zeros(0, 7)), torch.tensor([[30., 5., -1., 12.0, 2.5, 3.0, -2.0]])]
    labels = [torch.tensor([2, 0]), torch.zeros(0, dtype=torch.int64), torch.tensor([2])]
    pk = head.pack_targets(boxes, labels)
    assert pk['boxes'].shape == (3, 7) and pk['boxes'].dtype == np.float32 and pk['labels'].tolist() == [2, 0, 2]
    assert pk['frame_offsets'].tolist() == [0, 2, 2, 3] and pk['frame_offsets'].dtype == np.int32
    from gga_amd.dense_heads import gaussian_radius_np
    r = gaussian_radius_np(np.array([2.5 / 0.4]), np.array([12.0 / 0.4]), 0.1)[0]
    assert int(r) <= pk['max_radius'] <= int(r) + 2
    assert head.pack_targets([torch.zeros(0, 7)], [torch.zeros(0, dtype=torch.int64)])['max_radius'] == 2      # min_radius
    with pytest.raises(ValueError, match='one label per box'):
        head.pack_targets(boxes, labels[:2])


# ----------------------------------------------------------------------------- dataset
@pytest.mark.parametrize('style', ['pseudo', 'gga'])
def test_kitti_dataset_reads_both_info_styles(style, tmp_path):
    infos = pseudo_infos() if style == 'pseudo' else gga_infos()
    assert any(k.startswith('GGA_') for k in infos[0]['annos']) == (style == 'gga')
    ds = DATASETS.get('KittiDataset')(data_root=str(tmp_path), ann_file=infos, split='training', classes=CLASSES,
                                      modality=dict(use_lidar=True, use_camera=False))
    assert len(ds) == 3
    for i, info in enumerate(infos):
        ann = ds.get_ann_info(i)
        a = info['annos']
        keep = np.array([n != 'DontCare' for n in a['name']])
        cam = np.concatenate([a['location'][keep], a['dimensions'][keep], a['rotation_y'][keep][:, None]], 1).astype(np.float32)
        rect, trv2c = info['calib']['R0_rect'].astype(np.float32), info['calib']['Tr_velo_to_cam'].astype(np.float32)
        want = camera_boxes_to_lidar(cam, np.linalg.inv(rect @ trv2c))
        assert isinstance(ann['gt_bboxes_3d'], LiDARInstance3DBoxes) and torch.equal(ann['gt_bboxes_3d'].tensor, want)
        names = a['name'][keep]
        assert ann['gt_names'].tolist() == names.tolist() and 'DontCare' not in ann['gt_names']
        assert ann['gt_labels_3d'].tolist() == [CLASSES.index(n) if n in CLASSES else -1 for n in names]
        assert ann['gt_labels_3d'].dtype == np.int64 and ann['bboxes'].dtype == np.float32 and len(ann['bboxes']) == keep.sum()
        assert not any(k.startswith('GGA_') for k in ann)
    other = DATASETS.get('KittiDataset')(data_root=str(tmp_path), ann_file=infos, split='training', classes=['Car'],
                                         modality=dict(use_lidar=True, use_camera=False))
    assert set(other.get_ann_info(0)['gt_labels_3d'].tolist()) == {0, -1}          # a class that is not trained: -1


def test_kitti_dataset_and_gga_dataset_agree_on_the_boxes(tmp_path):
    kw = dict(data_root=str(tmp_path), ann_file=gga_infos(), split='training', classes=CLASSES, modality=dict(use_lidar=True, use_camera=False))
    a, b = DATASETS.get('KittiDataset')(**kw), DATASETS.get('KittiDataset_GGA_train')(**kw)
    for i in range(3):
        x, y = a.get_ann_info(i), b.get_ann_info(i)
        assert torch.equal(x['gt_bboxes_3d'].tensor, y['gt_bboxes_3d'].tensor) and (x['gt_labels_3d'] == y['gt_labels_3d']).all()


# ----------------------------------------------------------------------------- pipeline
def _scene(seed, n_boxes=5, n_points=4000):
    """Boxes in a 40 m square and points of which a good share lies inside them; points closer than 2 mm to a box face are
    dropped so that float32 rounding of the transforms cannot move one across it."""
    rng = np.random.RandomState(seed)
    boxes = np.stack([rng.uniform(5, 45, n_boxes), rng.uniform(-20, 20, n_boxes), rng.uniform(-2, -1, n_boxes), rng.uniform(1, 5, n_boxes),
                      rng.uniform(1, 3, n_boxes), rng.uniform(1, 2, n_boxes), rng.uniform(-3.1, 3.1, n_boxes)], 1).astype(np.float32)
    near = boxes[rng.randint(0, n_boxes, n_points // 2), :3] + rng.uniform(-3, 3, (n_points // 2, 3))
    far = np.stack([rng.uniform(0, 50, n_points // 2), rng.uniform(-25, 25, n_points // 2), rng.uniform(-3, 1, n_points // 2)], 1)
    pts = np.concatenate([near, far]).astype(np.float32)
    m = _margins(pts, boxes)
    pts = pts[(np.abs(m) > 2e-3).all(1)]
    return boxes, np.concatenate([pts, rng.rand(len(pts), 1).astype(np.float32)], 1)


def _margins(points, boxes):
    """[n_points, n_boxes] signed distance to the nearest face (positive inside), float64."""
    p, b = points[:, None, :3].astype(np.float64), boxes[None].astype(np.float64)
    d = p[..., :2] - b[..., :2]
    c, s = np.cos(b[..., 6]), np.sin(b[..., 6])
    lx, ly = d[..., 0] * c + d[..., 1] * s, -d[..., 0] * s + d[..., 1] * c
    lz = p[..., 2] - (b[..., 2] + b[..., 5] / 2)
    return np.minimum(np.minimum(b[..., 3] / 2 - np.abs(lx), b[..., 4] / 2 - np.abs(ly)), b[..., 5] / 2 - np.abs(lz))


def _sample(boxes, pts):
    d = dict(points=LiDARPoints(torch.from_numpy(pts.copy()), points_dim=4), bbox3d_fields=[], img_fields=[])
    if boxes is not None:
        d.update(gt_bboxes_3d=LiDARInstance3DBoxes(torch.from_numpy(boxes.copy())), gt_labels_3d=np.zeros(len(boxes), np.int64),
                 bbox3d_fields=['gt_bboxes_3d'])
    return d


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_boxes_follow_the_points(seed):
    boxes, pts = _scene(seed)
    inside = _margins(pts, boxes) > 0
    assert inside.any(0).all() and inside.sum() > 50          # (the scene is worth testing on)
    aug = Compose([dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
                   dict(type='GlobalRotScaleTrans', rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.9, 1.1],
                        translation_std=[0.5, 0.5, 0.2])])
    np.random.seed(seed)
    d = aug(_sample(boxes, pts))
    assert d['pcd_rotation_angle'] != 0 and d['pcd_scale_factor'] != 1 and np.any(d['pcd_trans'] != 0)
    assert seed not in (1, 2) or d['pcd_horizontal_flip'] or d['pcd_vertical_flip']
    moved = d['gt_bboxes_3d'].tensor.numpy()
    assert not np.allclose(moved, boxes)
    after = _margins(d['points'].tensor.numpy(), moved)
    assert (np.abs(after) > 1e-4).all() and ((after > 0) == inside).all()            # the same points in every box
    np.testing.assert_allclose(moved[:, 3:6], boxes[:, 3:6] * d['pcd_scale_factor'], rtol=1e-6)
    state = np.random.get_state()[1].copy()
    # without boxes the points come out bit for bit the same and the generator stands where it stood: the boxes draw nothing
    np.random.seed(seed)
    e = aug(_sample(None, pts))
    assert torch.equal(e['points'].tensor, d['points'].tensor) and (np.random.get_state()[1] == state).all()


def test_box_moves_one_by_one():
    b = LiDARInstance3DBoxes(torch.tensor([[1., 2., -1., 4., 2., 1.5, 0.25]]))
    b.rotate(0.5)
    c, s = np.cos(0.5), np.sin(0.5)
    np.testing.assert_allclose(b.tensor[0, :3].numpy(), [1 * c - 2 * s, 1 * s + 2 * c, -1], rtol=1e-6)
    assert abs(float(b.tensor[0, 6]) - 0.75) < 1e-6
    m = b.clone()
    m.rotate(torch.tensor([[c, s, 0.], [-s, c, 0.], [0., 0., 1.]], dtype=torch.float32))     # the matrix the points are multiplied by
    assert abs(float(m.tensor[0, 6]) - 1.25) < 1e-6
    b.translate([1.0, -1.0, 0.5])
    np.testing.assert_allclose(b.tensor[0, :3].numpy(), [1 * c - 2 * s + 1, 1 * s + 2 * c - 1, -0.5], rtol=1e-6)
    assert b.in_range_bev([0, 0, 10, 10]).tolist() == [True] and b.in_range_bev([0, 3, 10, 10]).tolist() == [False]
    v = LiDARInstance3DBoxes(torch.tensor([[1., 2., -1., 4., 2., 1.5, 0.25, 1.0, 0.0]]), box_dim=9)
    v.rotate(np.pi / 2)
    np.testing.assert_allclose(v.tensor[0, 7:].numpy(), [0.0, 1.0], atol=1e-6)


def test_object_filters():
    rng = [0, -40, -3, 70.4, 40, 1]
    boxes = torch.tensor([[10., 0., -1., 4., 2., 1.5, 4.0], [80., 0., -1., 4., 2., 1.5, 0.], [10., -41., -1., 4., 2., 1.5, 0.],
                          [30., 5., -1., 1., 1., 1.7, -0.5], [0., 5., -1., 1., 1., 1.7, -0.5]])
    d = dict(gt_bboxes_3d=LiDARInstance3DBoxes(boxes), gt_labels_3d=np.array([2, 2, 0, -1, 1]))
    d = PIPELINES.get('ObjectRangeFilter')(point_cloud_range=rng)(d)
    assert d['gt_labels_3d'].tolist() == [2, -1] and len(d['gt_bboxes_3d']) == 2              # x = 0 is ON the edge: out
    assert abs(float(d['gt_bboxes_3d'].tensor[0, 6]) - (4.0 - 2 * np.pi)) < 1e-6              # yaw to [-pi, pi)
    d = PIPELINES.get('ObjectNameFilter')(classes=CLASSES)(d)
    assert d['gt_labels_3d'].tolist() == [2] and torch.equal(d['gt_bboxes_3d'].tensor[:, :3], boxes[:1, :3])
    one = dict(gt_bboxes_3d=LiDARInstance3DBoxes(boxes[:1]), gt_labels_3d=np.array([1]))        # a single object stays a [1, 7] box
    one = PIPELINES.get('ObjectNameFilter')(classes=CLASSES)(PIPELINES.get('ObjectRangeFilter')(point_cloud_range=rng)(one))
    assert one['gt_bboxes_3d'].tensor.shape == (1, 7) and one['gt_labels_3d'].tolist() == [1]


def test_train_pipeline_carries_boxes_to_the_batch(tmp_path):
    """``LoadAnnotations3D`` -> ... -> ``Collect3D`` -> collate on the three-frame tree: LiDAR boxes and labels of every frame
    arrive at ``forward_train``'s keywords, one entry per frame, filtered alike."""
    from test_loader import kitti_tree
    kitti_tree(str(tmp_path))
    cfg = Config.fromfile(RETRAIN)
    pipe = copy.deepcopy(list(cfg.data['train']['dataset']['pipeline']))
    rng = [0, -39.68, -3, 69.12, 39.68, 1]
    for t in pipe:
        if 'point_cloud_range' in t:
            t['point_cloud_range'] = rng
    ds = DATASETS.get('KittiDataset')(data_root=str(tmp_path), ann_file=pseudo_infos(), split='training', pts_prefix='velodyne',
                                      pipeline=pipe, classes=CLASSES, modality=dict(use_lidar=True, use_camera=False))
    np.random.seed(3)
    loader = LD.build_dataloader(ds, samples_per_gpu=3, workers_per_gpu=0, dist=False, shuffle=False)
    batch = next(iter(loader))
    assert set(batch) >= {'points', 'img_metas', 'gt_bboxes_3d', 'gt_labels_3d'} and not any(k.startswith('GGA_') for k in batch)
    unwrap = lambda v: v.data[0] if hasattr(v, 'data') and isinstance(v.data, list) else v
    boxes, labels = unwrap(batch['gt_bboxes_3d']), unwrap(batch['gt_labels_3d'])
    assert len(boxes) == len(labels) == 3
    for b, l in zip(boxes, labels):
        assert isinstance(b, LiDARInstance3DBoxes) and len(b) == len(l) > 0 and (torch.as_tensor(l) >= 0).all()


def test_gga_train_pipeline_draws_what_it_drew(tmp_path, monkeypatch):
    """The GGA train pipeline has no transform that moves a box: with and without the LiDAR boxes' new ability its samples
    and the generator's state afterwards are the same."""
    from test_loader import dataset_cfg, kitti_tree
    infos = kitti_tree(str(tmp_path))
    got = []
    for moves in (True, False):
        monkeypatch.setattr(LiDARInstance3DBoxes, 'MOVES_WITH_POINTS', moves)
        ds = LD.build_dataset(dataset_cfg(str(tmp_path), infos, times=1))
        np.random.seed(5), torch.manual_seed(5)
        s = ds[0]
        got.append((s['points'].data.clone(), s['gt_bboxes_3d'].data.tensor.clone(), np.random.get_state()[1].copy()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and (got[0][2] == got[1][2]).all()
