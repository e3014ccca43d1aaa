"""Test-time augmentation on the device: the one-launch map merge against the reference's per-view loop restated here on CPU
tensors, against the reference's own merged maps (golden), and against known answers; the box merge; the detector's fused
path against its eager one; the view-major batch against the views run alone."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from gga_amd import Config, build_model, synthetic
from gga_amd import functional as F
from gga_amd.box3d import LiDARInstance3DBoxes
from gga_amd.tta import merge_aug_bboxes_3d

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# (scale, horizontal flip, vertical flip) per view
VIEW_SETS = {
    'plain': [(1.0, 0, 0)],
    'h': [(1.0, 0, 0), (1.0, 1, 0)],
    'double_flip': [(1.0, 0, 0), (1.0, 1, 0), (1.0, 0, 1), (1.0, 1, 1)],
    'three_scales': [(s, h, 0) for s in (0.95, 1.0, 1.05) for h in (0, 1)],
    'three_views': [(1.0, 0, 0), (1.0, 1, 0), (1.0, 0, 1)],                              # division by 3
    'interleaved': [(1.0, 0, 0), (0.95, 0, 1), (1.0, 1, 0), (0.95, 1, 1)],               # groups not contiguous in view order
}
COMMON = dict(reg=2, height=1, dim=3, rot=2)
TASK_SETS = {
    'one': [dict(COMMON, heatmap=1)],
    'three': [dict(COMMON, heatmap=1), dict(COMMON, heatmap=1), dict(COMMON, heatmap=1)],
    'vel': [dict(COMMON, heatmap=1), dict(COMMON, vel=2, heatmap=2)],
    'heatmap3': [dict(COMMON, heatmap=3)],
}


def groups_of(views):
    scales = []
    for s, _, _ in views:
        if s not in scales:
            scales.append(s)
    return [scales.index(s) for s, _, _ in views], [bool(h) for _, h, _ in views], [bool(v) for _, _, v in views]


def reference_merge(outs, views, n_frames):
    """The reference's loop (centerpoint_gga.py:123-182) on CPU float32 tensors: ``outs`` is the head's structure for the
    view-major batch; a view's rows go through the loop together (its operations leave the batch dimension alone).
    -> the structure ``get_bboxes`` receives, the scale groups' frames one behind the other."""
    outs_list, metas = [], []
    for v, (scale, hflip, vflip) in enumerate(views):
        view = [[{k: x[v * n_frames:(v + 1) * n_frames].clone() for k, x in task[0].items()}] for task in outs]
        for task_id, out in enumerate(view):
            for key in out[0].keys():
                if hflip:
                    view[task_id][0][key] = torch.flip(view[task_id][0][key], dims=[2])
                    if key == 'reg':
                        view[task_id][0][key][:, 1, ...] = 1 - view[task_id][0][key][:, 1, ...]
                    elif key == 'rot':
                        view[task_id][0][key][:, 0, ...] = -view[task_id][0][key][:, 0, ...]
                    elif key == 'vel':
                        view[task_id][0][key][:, 1, ...] = -view[task_id][0][key][:, 1, ...]
                if vflip:
                    view[task_id][0][key] = torch.flip(view[task_id][0][key], dims=[3])
                    if key == 'reg':
                        view[task_id][0][key][:, 0, ...] = 1 - view[task_id][0][key][:, 0, ...]
                    elif key == 'rot':
                        view[task_id][0][key][:, 1, ...] = -view[task_id][0][key][:, 1, ...]
                    elif key == 'vel':
                        view[task_id][0][key][:, 0, ...] = -view[task_id][0][key][:, 0, ...]
        outs_list.append(view)
        metas.append(scale)
    preds_dicts = dict()
    for scale, view in zip(metas, outs_list):
        if scale not in preds_dicts:
            preds_dicts[scale] = view
        else:
            for task_id, out in enumerate(view):
                for key in out[0].keys():
                    preds_dicts[scale][task_id][0][key] += out[0][key]
    for preds_dict in preds_dicts.values():
        for task_id, pred_dict in enumerate(preds_dict):
            for key in pred_dict[0].keys():
                preds_dict[task_id][0][key] /= len(outs_list) / len(preds_dicts.keys())
    groups = list(preds_dicts.values())
    return [[{k: torch.cat([g[t][0][k] for g in groups]) for k in outs[t][0].keys()}] for t in range(len(outs))]


_pool = {}


def random_maps(tasks, batch, H, W, seed):
    """Head-shaped random maps, cut from one pool of normal draws per size (drawing 26 M values per case would be the test)."""
    n = sum(sum(t.values()) for t in tasks) * batch * H * W
    key = (H, W)
    if key not in _pool or _pool[key].numel() < n + 64:
        _pool[key] = torch.randn(n + 64, generator=torch.Generator().manual_seed(H * 1000 + W))
    pool, at, outs = _pool[key], seed % 61, []
    for t in tasks:
        d = {}
        for k, c in t.items():
            m = batch * c * H * W
            d[k] = pool[at:at + m].reshape(batch, c, H, W).clone()
            at += m
        outs.append([d])
    return outs


def to_dev(outs):
    return [[{k: x.to(DEV) for k, x in task[0].items()}] for task in outs]


def assert_same(got, want, what):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert list(g[0].keys()) == list(w[0].keys())
        for k in w[0]:
            assert g[0][k].shape == w[0][k].shape, (what, t, k, g[0][k].shape, w[0][k].shape)
            assert torch.equal(g[0][k].cpu(), w[0][k]), (what, t, k, float((g[0][k].cpu() - w[0][k]).abs().max()))


# ------------------------------------------------------------------------------------------------- kernel vs restatement
@pytest.mark.parametrize('tasks', list(TASK_SETS))
@pytest.mark.parametrize('n_frames', [1, 3])
@pytest.mark.parametrize('hw', [(5, 7), (6, 10), (1, 4), (248, 216)])
def test_merge_kernel_equals_the_reference_loop(hw, n_frames, tasks):
    H, W = hw
    for i, (name, views) in enumerate(VIEW_SETS.items()):
        outs = random_maps(TASK_SETS[tasks], len(views) * n_frames, H, W, seed=i + 7 * n_frames)
        group, hflip, vflip = groups_of(views)
        got = F.tta_merge_maps(to_dev(outs), group, hflip, vflip, n_frames)
        assert got[0][0]['heatmap'].shape[0] == (max(group) + 1) * n_frames
        assert_same(got, reference_merge(outs, views, n_frames), (name, hw, n_frames, tasks))


def test_merge_kernel_on_unaligned_rows():
    """A map that does not start on a 16-byte boundary takes the element-wise form although W is a multiple of 4."""
    views, n_frames, H, W = VIEW_SETS['double_flip'], 2, 6, 8
    outs = random_maps(TASK_SETS['vel'], len(views) * n_frames, H, W, seed=3)
    dev = []
    for task in outs:
        d = {}
        for k, x in task[0].items():
            buf = torch.empty(x.numel() + 1, device=DEV)
            buf[1:] = x.reshape(-1).to(DEV)
            d[k] = buf[1:].view(x.shape)
            assert d[k].data_ptr() % 16 == 4 and d[k].is_contiguous()
        dev.append([d])
    assert_same(F.tta_merge_maps(dev, *groups_of(views), n_frames), reference_merge(outs, views, n_frames), 'unaligned')


def test_merge_kernel_reproduces_the_reference_maps(golden):
    d = golden('tta')
    views = [tuple(r) for r in d['views'].tolist()]
    keys = [[k.split('.')[3] for k in d.files if k.startswith(f'in.0.{t}.')] for t in range(2)]
    assert len(views) == 8 and 'vel' in keys[1] and 'vel' not in keys[0]
    outs = [[{k: torch.cat([torch.from_numpy(d[f'in.{v}.{t}.{k}']) for v in range(len(views))]) for k in keys[t]}] for t in range(2)]
    got = F.tta_merge_maps(to_dev(outs), *groups_of(views), 1)
    for t in range(2):
        for k in keys[t]:
            want = torch.cat([torch.from_numpy(d[f'out.{s}.{t}.{k}']) for s in range(2)])
            assert torch.equal(got[t][0][k].cpu(), want), (t, k)
    assert_same(got, reference_merge(outs, views, 1), 'golden case')       # and the restatement is the reference's loop


# ------------------------------------------------------------------------------------------------------------ known answer
def forward_view(base, hflip, vflip):
    """What the head would see of ``base`` in a flipped view (the flips are involutions: forward = backward)."""
    out = []
    for task in base:
        d = {}
        for k, x in task[0].items():
            y = x.clone()
            for on, dim, reg_ch, rot_ch, vel_ch in ((hflip, 2, 1, 0, 1), (vflip, 3, 0, 1, 0)):
                if not on:
                    continue
                y = torch.flip(y, dims=[dim])
                if k == 'reg':
                    y[:, reg_ch] = 1 - y[:, reg_ch]
                elif k == 'rot':
                    y[:, rot_ch] = -y[:, rot_ch]
                elif k == 'vel':
                    y[:, vel_ch] = -y[:, vel_ch]
            d[k] = y
        out.append([d])
    return out


@pytest.mark.parametrize('hw', [(5, 7), (7, 12), (31, 20)])
def test_merged_views_of_one_scene_give_the_scene_back(hw):
    H, W = hw
    n_frames = 2
    g = torch.Generator().manual_seed(H)
    # values k / 1024 in [0, 1]: 1 - x, x + x (+ x + x), 3 x and the divisions by 2, 3, 4 are all exact
    base = [[{k: torch.randint(0, 1025, (n_frames, c, H, W), generator=g).float() / 1024 for k, c in t.items()}]
            for t in TASK_SETS['vel']]
    for name in ('h', 'double_flip', 'three_views', 'three_scales', 'interleaved'):
        views = VIEW_SETS[name]
        per_view = [forward_view(base, h, v) for _, h, v in views]
        outs = [[{k: torch.cat([pv[t][0][k] for pv in per_view]) for k in base[t][0]}] for t in range(len(base))]
        group, hflip, vflip = groups_of(views)
        got = F.tta_merge_maps(to_dev(outs), group, hflip, vflip, n_frames)
        n_groups = max(group) + 1
        want = [[{k: torch.cat([x] * n_groups) for k, x in task[0].items()}] for task in base]
        assert_same(got, want, name)
    # the direction of the mirror itself: a map holding its row (column) index, seen through one flipped view
    assert H % 2 == 1          # the middle row maps to itself
    rows = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).expand(1, 1, H, W).contiguous()
    cols = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(1, 1, H, W).contiguous()
    for hflip, vflip in ((True, False), (False, True), (True, True)):
        got = F.tta_merge_maps(to_dev([[dict(heatmap=rows, height=cols)]]), [0], [hflip], [vflip], 1)
        assert torch.equal(got[0][0]['heatmap'].cpu(), H - 1 - rows if hflip else rows)
        assert torch.equal(got[0][0]['height'].cpu(), W - 1 - cols if vflip else cols)


# --------------------------------------------------------------------------------------------------------------- box merge
def base_boxes():
    """12 boxes of 0.7 m x 0.5 m on a 4 x 3 grid 1 m apart (their half diagonal is 0.43 m: no two overlap at any yaw, at scale
    0.95 against 1.05 either), three classes. A copy scaled by 0.95 lies at most 0.18 m from the one scaled by 1.05: their IoU
    stays far above the threshold. Every coordinate is within +-2 m: mapping a scaled box back (x * s * (1 / s): two float32
    roundings, and 1 / s held in double) moves a coordinate by less than 2 ulp(2) = 4.8e-7 < 1e-6."""
    g = torch.Generator().manual_seed(5)
    xy = torch.tensor([[-1.5 + 1.0 * i, -1.0 + 1.0 * j] for i in range(4) for j in range(3)])
    boxes = torch.cat([xy, torch.full((12, 1), -1.0), torch.tensor([[0.7, 0.5, 0.6]]).expand(12, 3),
                       torch.rand(12, 1, generator=g) * 3 - 1.5], dim=1)
    return boxes, torch.linspace(0.3, 0.85, 12)[torch.randperm(12, generator=g)], torch.arange(12) % 3


@pytest.mark.parametrize('use_rotate_nms', [True, False])
def test_merge_aug_bboxes_known_answer(use_rotate_nms):
    boxes, scores, labels = base_boxes()
    scales = (0.95, 1.0, 1.05)
    aug, metas = [], []
    for k, s in enumerate(scales):
        b = LiDARInstance3DBoxes(boxes.to(DEV))
        b.scale(s)
        aug.append(dict(boxes_3d=b, scores_3d=(scores + 0.01 * k).to(DEV), labels_3d=labels.int().to(DEV)))
        metas.append([dict(pcd_scale_factor=s, pcd_horizontal_flip=False, pcd_vertical_flip=False)])
    best = scores + 0.01 * (len(scales) - 1)
    order = torch.argsort(best, descending=True)
    for max_num in (500, 7):
        cfg = dict(use_rotate_nms=use_rotate_nms, nms_thr=0.2, max_num=max_num)
        res = merge_aug_bboxes_3d(aug, metas, cfg)
        n = min(max_num, 12)
        assert not res['boxes_3d'].tensor.is_cuda and not res['scores_3d'].is_cuda and not res['labels_3d'].is_cuda
        assert len(res['scores_3d']) == n                                    # one box per base box, then the cut
        assert torch.equal(res['scores_3d'], best[order][:n])                  # the highest-scored copy, by descending score
        assert torch.equal(res['labels_3d'].long(), labels[order][:n])
        err = (res['boxes_3d'].tensor - boxes[order][:n]).abs().max()
        print(f'mapped-back error {float(err):.3e}')
        assert err <= 1e-6
    # flips come back too: the views of one scale, flipped, merge to the base boxes
    flipped = LiDARInstance3DBoxes(boxes.to(DEV))
    flipped.flip('horizontal')
    res = merge_aug_bboxes_3d([aug[1], dict(aug[1], boxes_3d=flipped, scores_3d=aug[1]['scores_3d'] + 0.001)],
                              [metas[1], [dict(pcd_scale_factor=0.5 + 0.5, pcd_horizontal_flip=True, pcd_vertical_flip=False)]],
                              dict(use_rotate_nms=use_rotate_nms, nms_thr=0.2, max_num=500))
    assert len(res['scores_3d']) == 12 and torch.equal(res['boxes_3d'].tensor, boxes[torch.argsort(scores, descending=True)])
    empty = dict(boxes_3d=LiDARInstance3DBoxes(torch.zeros(0, 7, device=DEV)), scores_3d=torch.zeros(0, device=DEV),
                 labels_3d=torch.zeros(0, dtype=torch.int32, device=DEV))
    res = merge_aug_bboxes_3d([empty, empty], metas[:2], cfg)
    assert len(res['boxes_3d']) == 0 and res['boxes_3d'].tensor.shape == (0, 7) and len(res['scores_3d']) == 0
    assert not res['boxes_3d'].tensor.is_cuda


# ---------------------------------------------------------------------------------------------------------------- detector
@pytest.fixture(scope='module')
def detector():
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_pointpillars_config.py'))
    torch.manual_seed(0)
    model = build_model(cfg.model).to(DEV).eval()
    with torch.no_grad():
        for th in model.pts_bbox_head.task_heads:
            for name in ('reg', 'height', 'dim', 'rot'):
                getattr(th, name)[-1].weight.mul_(0.05)
            th.dim[-1].bias.fill_(1.0)
    model.pts_bbox_head.test_cfg['use_rotate_nms'] = True
    model.pts_bbox_head.test_cfg['max_num'] = 500
    return model


@pytest.fixture(scope='module')
def frames():
    return synthetic.make_batch(2, n_points=6000, pc_range=synthetic.RANGE_PP)


def make_views(frames, views, n_frames=2):
    """points[v][f], img_metas[v][f] through the test pipeline's inner transforms."""
    from gga_amd.pipelines import GlobalRotScaleTrans, PointsRangeFilter, RandomFlip3D
    from gga_amd.points import LiDARPoints
    inner = [GlobalRotScaleTrans(rot_range=[0, 0], scale_ratio_range=[1., 1.], translation_std=[0, 0, 0]),
             RandomFlip3D(sync_2d=False), PointsRangeFilter(point_cloud_range=list(synthetic.RANGE_PP))]
    points, metas = [], []
    for scale, hflip, vflip in views:
        pv, mv = [], []
        for f in range(n_frames):
            d = dict(points=LiDARPoints(frames['points'][f].cpu().clone(), points_dim=4), flip=True, pcd_scale_factor=scale,
                     pcd_horizontal_flip=bool(hflip), pcd_vertical_flip=bool(vflip))
            for t in inner:
                d = t(d)
            pv.append(d['points'].tensor.to(DEV))
            mv.append(dict(frames['img_metas'][f], box_type_3d=LiDARInstance3DBoxes, pcd_scale_factor=d['pcd_scale_factor'],
                           pcd_horizontal_flip=d['pcd_horizontal_flip'], pcd_vertical_flip=d['pcd_vertical_flip']))
        points.append(pv)
        metas.append(mv)
    return points, metas


def assert_results_equal(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        x, y = ra['pts_bbox'], rb['pts_bbox']
        for r in (x, y):
            assert not r['boxes_3d'].tensor.is_cuda and not r['scores_3d'].is_cuda and not r['labels_3d'].is_cuda
        assert x['boxes_3d'].tensor.shape == y['boxes_3d'].tensor.shape
        assert torch.equal(x['boxes_3d'].tensor, y['boxes_3d'].tensor) and torch.equal(x['scores_3d'], y['scores_3d'])
        assert torch.equal(x['labels_3d'].int(), y['labels_3d'].int())


@pytest.mark.parametrize('batched', [True, False])
def test_aug_test_fused_equals_eager(detector, frames, monkeypatch, batched):
    from gga_amd.dense_heads import CenterHead_GGA
    monkeypatch.setattr(CenterHead_GGA, 'BATCHED', batched)

    def run(views, n_frames, fused):
        monkeypatch.setattr(type(detector), 'TTA_MERGE', fused)
        points, metas = make_views(frames, views, n_frames)
        return detector.forward_test(points, metas, rescale=True)

    scales = VIEW_SETS['three_scales']
    for n_frames in (2, 1):
        fused, eager = run(scales, n_frames, True), run(scales, n_frames, False)
        assert len(fused) == n_frames
        assert_results_equal(fused, eager)
        # one scale (flips only): no box merge, the group's detections go to the host
        per_scale = []
        for s in (0.95, 1.0, 1.05):
            one = [v for v in scales if v[0] == s]
            a, b = run(one, n_frames, True), run(one, n_frames, False)
            assert_results_equal(a, b)
            per_scale.append([len(r['pts_bbox']['scores_3d']) for r in a])
        for f in range(n_frames):
            merged, parts = len(fused[f]['pts_bbox']['scores_3d']), sum(c[f] for c in per_scale)
            print(f'frame {f}: {merged} merged detections of {parts} over the scales')
            assert 1 <= merged < parts


def test_forward_test_degenerate_cases(detector, frames):
    points, metas = make_views(frames, VIEW_SETS['plain'])
    one = detector.forward_test(points, metas, rescale=True)
    assert_results_equal(one, detector.simple_test(points[0], metas[0], rescale=True))
    assert sum(len(r['pts_bbox']['scores_3d']) for r in one) > 0
    # KITTI's x range is [0, 69.12]: a vertical flip (x -> -x) cannot be undone by mirroring the map
    points, metas = make_views(frames, [(1.0, 0, 0), (1.0, 0, 1)])
    with pytest.raises(ValueError, match='x axis'):
        detector.forward_test(points, metas)
    points, metas = make_views(frames, [(1.0, 0, 0), (1.0, 1, 0), (0.95, 0, 0)])
    with pytest.raises(ValueError, match='same number'):
        detector.forward_test(points, metas)


@pytest.mark.parametrize('channels_last', [True, False])
def test_view_major_batch_equals_the_views_run_alone(detector, frames, channels_last):
    """In eval mode nothing couples the frames of a batch: the head maps of the V * F point clouds run as one batch are those of
    each run alone at batch 1 (the reference's form). The reference here is the run alone.
    - channels-last trunk (what apis.generate_pseudo_labels and tools/test.py build): every convolution runs on the project's
      kernels, whose result for a frame does not depend on the batch: bit for bit.
    - default layout: the convolutions go to the vendor library, which picks its algorithm by problem size, the batch included
      (EXPERIMENTS.md: the first difference is at the first 64 -> 128 stride-2 convolution, 5e-7, and the heat-map ends 2.6e-6
      apart): the bound of forward parity, 1e-4 in |a - b| / max(|b|, 1)."""
    model = detector
    if channels_last:
        from gga_amd.cnn import to_channels_last
        cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_pointpillars_config.py'))
        cfg.model.pts_middle_encoder['channels_last'] = True
        torch.manual_seed(0)
        model = to_channels_last(build_model(cfg.model).to(DEV)).eval()
    points, metas = make_views(frames, VIEW_SETS['three_scales'])
    flat = [p for view in points for p in view]
    worst, same = 0.0, True
    with torch.no_grad():
        together = model.pts_bbox_head(model.extract_feat(flat, None, None)[1])
        for i, p in enumerate(flat):
            alone = model.pts_bbox_head(model.extract_feat([p], None, None)[1])
            for t, task in enumerate(alone):
                for k, b in task[0].items():
                    a = together[t][0][k][i:i + 1]
                    assert a.shape == b.shape
                    worst = max(worst, float(((a - b).abs() / b.abs().clamp(min=1)).max()))
                    same = same and torch.equal(a, b)
    print(f'batched vs alone (channels_last={channels_last}): worst |a-b| / max(|b|, 1) = {worst:.3e}, identical: {same}')
    if channels_last:
        assert same and worst == 0.0
    else:
        assert worst <= 1e-4


# ------------------------------------------------------------------------------------------------------------------ tools
def test_pseudo_label_run_with_the_tta_config(tmp_path):
    """The flow of tools/test.py / tools/generate_pseudo_labels_gga.py on the TTA matching config's test section (6 views per
    frame, two frames per batch), pointed at the on-disk tree with the PointPillars model: detections for every frame, fewer
    than the single-view run's three scales would add up to, and the dataset's evaluation accepts them."""
    import copy
    import pickle
    from gga_amd.apis import generate_pseudo_labels
    from test_loader import PP_RANGE, kitti_tree
    infos = kitti_tree(str(tmp_path))
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_matching_tta_config.py'))
    model_cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_pointpillars_config.py'))
    extra = {k: cfg.model.test_cfg.pts[k] for k in ('use_rotate_nms', 'max_num')}
    cfg.model, cfg.test_cfg = model_cfg.model, None
    cfg.model.test_cfg.pts.update(extra)
    test = dict(cfg.data['test'])
    pipe = copy.deepcopy(list(test['pipeline']))
    for t in pipe[1]['transforms']:
        if t['type'] == 'PointsRangeFilter':
            t['point_cloud_range'] = PP_RANGE
    test.update(data_root=str(tmp_path), ann_file=infos, pts_prefix='velodyne', pipeline=pipe, pcd_limit_range=PP_RANGE)
    cfg.data = dict(samples_per_gpu=2, workers_per_gpu=0, test=test, test_dataloader=dict(samples_per_gpu=2, workers_per_gpu=0))
    torch.manual_seed(0)
    model = build_model(Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_pointpillars_config.py')).model)
    with torch.no_grad():
        for th in model.pts_bbox_head.task_heads:
            for name in ('reg', 'height', 'dim', 'rot'):
                getattr(th, name)[-1].weight.mul_(0.05)
            th.heatmap[-1].bias.fill_(0.5)
    ck = str(tmp_path / 'epoch_1.pth')
    torch.save(dict(meta=dict(epoch=1, iter=3, CLASSES=('Pedestrian', 'Cyclist', 'Car')),
                    state_dict={'module.' + k: v for k, v in model.state_dict().items()}), ck)
    out_file = str(tmp_path / 'pseudo.pkl')
    outputs, res = generate_pseudo_labels(cfg, ck, eval_metrics=('mAP',), eval_options=dict(pseudo_label_file=out_file))
    assert len(outputs) == 3 and all(set(o['pts_bbox']) >= {'boxes_3d', 'scores_3d', 'labels_3d'} for o in outputs)
    assert all(0 < len(o['pts_bbox']['scores_3d']) <= 500 and not o['pts_bbox']['boxes_3d'].tensor.is_cuda for o in outputs)
    for o in outputs:
        s = o['pts_bbox']['scores_3d']
        assert torch.equal(s, s.sort(descending=True)[0])            # the box merge's order
    assert res['pseudo_labels/frames'] == 3.0 and len(pickle.load(open(out_file, 'rb'))) == 3
