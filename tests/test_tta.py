"""Test-time augmentation without a GPU: box mapping against the reference's golden, argument validation of the merge
kernel's entry point, the TTA configs, and the 6-view layout from the test pipeline through collate to the detector's inputs."""
import copy
import ctypes as C
import os

import numpy as np
import torch

from conftest import REPO
from gga_amd import Config, _lib
from gga_amd import loader as LD
from gga_amd.box3d import LiDARInstance3DBoxes
from gga_amd.pipelines import DataContainer as DC
from gga_amd.tta import bbox3d_mapping_back
from test_loader import PP_RANGE, SEEDS, kitti_tree

CFG_DIR = os.path.join(REPO, 'configs', 'gga')


# ------------------------------------------------------------------------------------------------------------------ boxes
def test_flip_scale_and_mapping_back_equal_the_reference_bit_for_bit(golden):
    d = golden('tta')
    scales = d['back_scales'].tolist()
    assert scales == [0.95, 1, 1.05]
    for dim in (7, 9):
        src = torch.from_numpy(d[f'box{dim}'])
        for h in (False, True):
            for v in (False, True):
                for si, scale in enumerate(scales):
                    boxes = LiDARInstance3DBoxes(src, box_dim=dim)
                    back = bbox3d_mapping_back(boxes, scale, h, v)
                    assert torch.equal(boxes.tensor, src), 'mapping back works on a copy'
                    want = torch.from_numpy(d[f'back{dim}.{int(h)}{int(v)}.{si}'])
                    assert back.tensor.shape == want.shape and torch.equal(back.tensor, want), (dim, h, v, scale)
        # the two in-place pieces on their own: flips (1.0 is an exact scale) and the scale alone
        for direction, key in (('horizontal', '10'), ('vertical', '01')):
            b = LiDARInstance3DBoxes(src, box_dim=dim)
            b.flip(direction)
            assert torch.equal(b.tensor, torch.from_numpy(d[f'back{dim}.{key}.1']))
        b = LiDARInstance3DBoxes(src, box_dim=dim)
        b.scale(1 / 0.95)
        assert torch.equal(b.tensor, torch.from_numpy(d[f'back{dim}.00.0']))
        assert torch.equal(b.tensor[:, 6], src[:, 6]), 'the yaw is not scaled'


def test_box_cat_and_indexing():
    a = LiDARInstance3DBoxes(torch.arange(14.).reshape(2, 7))
    b = LiDARInstance3DBoxes(torch.arange(21.).reshape(3, 7) + 100)
    c = LiDARInstance3DBoxes.cat([a, b])
    assert len(c) == 5 and torch.equal(c.tensor, torch.cat([a.tensor, b.tensor])) and c.box_dim == 7
    c.tensor[0, 0] = -1
    assert a.tensor[0, 0] == 0, 'cat does not share storage'
    assert len(LiDARInstance3DBoxes.cat([])) == 0
    mask = torch.tensor([True, False, True, False, True])
    assert torch.equal(c[mask].tensor, c.tensor[mask])
    idx = torch.tensor([4, 0])
    assert torch.equal(c[idx].tensor, c.tensor[idx]) and len(c[3]) == 1
    nine = LiDARInstance3DBoxes.cat([LiDARInstance3DBoxes(torch.zeros(2, 9), box_dim=9)])
    assert nine.box_dim == 9


# ------------------------------------------------------------------------------------------------------------- validation
def _table(n_maps=1, group=(0,), kind=_lib.TTA_PLAIN, channels=1, n_groups=None):
    tb = _lib.TtaTable()
    tb.n_maps, tb.n_views = n_maps, len(group)
    tb.n_groups = max(group, default=0) + 1 if n_groups is None else n_groups
    for v, g in enumerate(group[:_lib.TTA_MAX_VIEWS]):
        tb.group[v] = g
    for m in range(max(0, min(n_maps, _lib.TTA_MAX_MAPS))):
        tb.map[m].src, tb.map[m].dst, tb.map[m].channels, tb.map[m].kind = 4096, 8192, channels, kind     # never dereferenced
    return tb


def test_merge_maps_argument_validation_without_gpu():
    L = _lib.lib()

    def rejected(tb, F=1, H=5, W=7):
        rc = L.gga_tta_merge_maps(None if tb is None else C.byref(tb), F, H, W, None)
        msg = L.gga_last_error().decode()
        assert rc == -1 and msg.startswith('gga_tta_merge_maps:'), (rc, msg)
        return msg

    assert 'null table' in rejected(None)
    for n in (0, _lib.TTA_MAX_MAPS + 1):
        assert 'n_maps' in rejected(_table(n_maps=n))
    assert 'n_views' in rejected(_table(group=()))
    assert 'n_views' in rejected(_table(group=(0,) * (_lib.TTA_MAX_VIEWS + 1)))
    for bad in (dict(H=0), dict(H=-3), dict(W=0), dict(F=0)):
        assert 'must be positive' in rejected(_table(), **bad)
    assert 'group -1 of view 1' in rejected(_table(group=(0, -1), n_groups=1))
    assert 'group 2 of view 1' in rejected(_table(group=(0, 2), n_groups=2))
    assert 'group 1 has no view' in rejected(_table(group=(0, 2, 0), n_groups=3))
    assert 'unknown kind' in rejected(_table(kind=4))
    assert 'unknown kind' in rejected(_table(kind=-1))
    for kind in (_lib.TTA_REG, _lib.TTA_ROT, _lib.TTA_VEL):
        assert 'channels' in rejected(_table(kind=kind, channels=1))
    assert 'channels' in rejected(_table(channels=0))
    assert _lib.TTA_MAX_MAPS == _lib.MAX_TASKS * 6 and _lib.TTA_MAX_VIEWS == 16


def test_functional_wrapper_refuses_cpu_tensors():
    import pytest
    from gga_amd import functional as F
    outs = [[dict(heatmap=torch.zeros(2, 1, 5, 7), reg=torch.zeros(2, 2, 5, 7))]]
    with pytest.raises(RuntimeError, match='GPU only'):
        F.tta_merge_maps(outs, [0, 0], [False, True], [False, False], 1)


# ---------------------------------------------------------------------------------------------------------------- configs
def test_tta_configs_load_and_keep_the_model_and_train_sections():
    for name, base in (('gga_kitti_tta_config.py', 'gga_kitti_config.py'),
                       ('gga_kitti_matching_tta_config.py', 'gga_kitti_matching_config.py')):
        cfg, ref = Config.fromfile(os.path.join(CFG_DIR, name)), Config.fromfile(os.path.join(CFG_DIR, base))
        wrapper = cfg.data.test.pipeline[1]
        assert wrapper['type'] == 'MultiScaleFlipAug3D' and list(wrapper['pts_scale_ratio']) == [0.95, 1.0, 1.05]
        assert wrapper['flip'] is True and wrapper['pcd_horizontal_flip'] is True and wrapper['pcd_vertical_flip'] is False
        flips = [t for t in wrapper['transforms'] if t['type'] == 'RandomFlip3D']
        assert len(flips) == 1 and flips[0]['sync_2d'] is False
        assert cfg.data.val.pipeline == cfg.data.test.pipeline
        tc = cfg.model.test_cfg.pts
        assert tc['use_rotate_nms'] is True and tc['max_num'] == tc['max_per_img'] == 500
        # the model but for the two keys the box merge reads, and everything of the training run
        model = copy.deepcopy(cfg.model.to_dict() if hasattr(cfg.model, 'to_dict') else dict(cfg.model))
        want = ref.model.to_dict() if hasattr(ref.model, 'to_dict') else dict(ref.model)
        for k in ('use_rotate_nms', 'max_num'):
            del model['test_cfg']['pts'][k]
        assert model == want
        for section in ('train_pipeline', 'optimizer', 'optimizer_config', 'lr_config', 'momentum_config', 'runner'):
            assert cfg[section] == ref[section], section
        assert cfg.data.train == ref.data.train and cfg.data.samples_per_gpu == ref.data.samples_per_gpu
    assert Config.fromfile(os.path.join(CFG_DIR, 'gga_kitti_matching_tta_config.py')).data.test.type == 'KittiDataset_GGA_match'


# ----------------------------------------------------------------------------------------------------- pipeline and loader
def _tta_dataset(root):
    infos = kitti_tree(root)
    cfg = Config.fromfile(os.path.join(CFG_DIR, 'gga_kitti_matching_tta_config.py'))
    test = dict(cfg.data['test'])
    pipe = copy.deepcopy(list(test['pipeline']))
    for t in pipe[1]['transforms']:
        if t['type'] == 'PointsRangeFilter':
            t['point_cloud_range'] = PP_RANGE
    test.update(data_root=root, ann_file=infos, pts_prefix='velodyne', pipeline=pipe, pcd_limit_range=PP_RANGE)
    return LD.build_dataset(dict(test, test_mode=True))


def _expected_view(raw, scale, hflip):
    """The inner transforms in float32 as the pipeline runs them: scale, flip y, range filter (open interval)."""
    pts = raw.clone()
    if scale != 1:
        pts[:, :3] *= scale
    if hflip:
        pts[:, 1] = -pts[:, 1]
    lo, hi = torch.tensor(PP_RANGE[:3]), torch.tensor(PP_RANGE[3:])
    return pts[((pts[:, :3] > lo) & (pts[:, :3] < hi)).all(1)]


VIEWS = [(s, h) for s in (0.95, 1.0, 1.05) for h in (False, True)]      # scale outer, horizontal flip inner


def test_tta_pipeline_delivers_six_views_through_collate(tmp_path):
    ds = _tta_dataset(str(tmp_path))
    assert len(ds) == 3
    raws = [torch.from_numpy(np.fromfile(os.path.join(str(tmp_path), 'training', 'velodyne', f'{seed:06d}.bin'),
                                         dtype=np.float32).reshape(-1, 4)) for seed in SEEDS]
    samples = [ds[i] for i in range(3)]
    for seed, raw, s in zip(SEEDS, raws, samples):
        assert isinstance(s['points'], list) and len(s['points']) == len(s['img_metas']) == 6
        for (scale, hflip), pts, meta in zip(VIEWS, s['points'], s['img_metas']):
            assert isinstance(pts, DC) and isinstance(meta, DC)
            m = meta.data
            assert m['pcd_scale_factor'] == scale and m['pcd_horizontal_flip'] is hflip and m['pcd_vertical_flip'] is False
            assert m['sample_idx'] == seed
            want = _expected_view(raw, scale, hflip)
            assert len(want) > 100 and torch.equal(pts.data, want), (seed, scale, hflip)
        # a flipped view is the mirror image of the plain one of its scale
        plain, flipped = s['points'][2].data, s['points'][3].data
        assert torch.equal(flipped[:, 1], -plain[:, 1]) and torch.equal(flipped[:, [0, 2, 3]], plain[:, [0, 2, 3]])
    for packed in (False, True):
        batch = LD.collate(samples[:2], samples_per_gpu=2, packed=packed)
        assert LD.chunks_in(batch) == 1
        data = LD.to_step_inputs(batch, torch.device('cpu'), 0)
        points, metas = data['points'], data['img_metas']
        assert len(points) == len(metas) == 6
        for v, (scale, hflip) in enumerate(VIEWS):
            assert len(points[v]) == len(metas[v]) == 2
            for f in range(2):
                assert torch.equal(points[v][f], samples[f]['points'][v].data), (packed, v, f)
                assert metas[v][f]['sample_idx'] == SEEDS[f] and metas[v][f]['pcd_scale_factor'] == scale
                assert metas[v][f]['pcd_horizontal_flip'] is hflip


def test_single_gpu_test_hands_the_views_to_the_model(tmp_path):
    from gga_amd.apis import single_gpu_test
    ds = _tta_dataset(str(tmp_path))
    seen = []

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, return_loss=True, rescale=False, points=None, img_metas=None):
            assert not return_loss and rescale and len(points) == len(img_metas) == 6
            assert [(m[0]['pcd_scale_factor'], m[0]['pcd_horizontal_flip']) for m in img_metas] == VIEWS
            seen.append([[m['sample_idx'] for m in view] for view in img_metas])
            return [dict(pts_bbox=dict(n=[len(view[f]) for view in points])) for f in range(len(points[0]))]

    loader = LD.build_dataloader(ds, samples_per_gpu=2, workers_per_gpu=0, dist=False, shuffle=False)
    out = single_gpu_test(Stub(), loader, torch.device('cpu'))
    assert seen == [[[SEEDS[0], SEEDS[1]]] * 6, [[SEEDS[2]]] * 6]
    assert len(out) == 3 and all(len(o['pts_bbox']['n']) == 6 and min(o['pts_bbox']['n']) > 100 for o in out)


# --------------------------------------------------------------------------------------------------------------- detector
def test_detector_refuses_views_it_cannot_merge():
    """The guards run before anything touches the device."""
    import pytest
    from gga_amd import build_model
    model = build_model(Config.fromfile(os.path.join(CFG_DIR, 'gga_kitti_pointpillars_config.py')).model).eval()
    meta = lambda s, h=False, v=False: [dict(pcd_scale_factor=s, pcd_horizontal_flip=h, pcd_vertical_flip=v)]
    pts = [torch.zeros(4, 4)]
    with pytest.raises(ValueError, match='x axis'):          # KITTI's x range is [0, 69.12]
        model.forward_test([pts, pts], [meta(1.0), meta(1.0, v=True)])
    with pytest.raises(ValueError, match='same number'):
        model.forward_test([pts, pts, pts], [meta(1.0), meta(1.0, h=True), meta(0.95)])
    assert type(model).TTA_MERGE is (os.environ.get('GGA_TTA_MERGE', '1') != '0')
