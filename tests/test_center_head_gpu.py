"""Supervised CenterPoint on the device: ``gga_center_targets`` against the reference's ``get_targets``
(tests/golden/center_head.npz, tools_dev/make_golden_center_head.py), ``gga_center_reg_loss_fwd/bwd`` and the whole loss
against float64 autograd (tests/_center_head_ref.py), and two iterations of ``train_detector`` with ``CenterPoint``."""
import copy
import os

import numpy as np
import pytest
import torch

import _center_head_ref as R
from conftest import GOLDEN, REPO
from gga_amd import Config
from gga_amd import functional as F
from gga_amd import loader as LD
from gga_amd.box3d import LiDARInstance3DBoxes
from gga_amd.registry import build_head

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(GOLDEN, 'center_head.npz')))


def make_head(layout, train_cfg=None):
    tasks = [dict(num_class=len(n), class_names=n) for n in R.LAYOUTS[layout]]
    cfg = dict(type='CenterHead', in_channels=16, tasks=tasks, common_heads=dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2)),
               share_conv_channel=16, loss_cls=dict(type='GaussianFocalLoss', reduction='mean', **R.LOSS_CLS[layout]),
               loss_bbox=dict(type='L1Loss', reduction='mean', loss_weight=R.LOSS_WEIGHT), norm_bbox=True,
               train_cfg=dict(train_cfg or R.TRAIN_CFG), test_cfg=None)
    return build_head(cfg).to(DEV)


def frames_of(gold):
    off = gold['frame_offsets']
    boxes = [LiDARInstance3DBoxes(torch.from_numpy(gold['boxes'][a:b])) for a, b in zip(off[:-1], off[1:])]
    labels = [torch.from_numpy(gold['labels'][a:b]) for a, b in zip(off[:-1], off[1:])]
    return boxes, labels


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


# ----------------------------------------------------------------------------- targets
@pytest.mark.parametrize('layout', ['A', 'B'])
def test_targets_against_the_reference(layout, gold):
    head = make_head(layout)
    boxes, labels = frames_of(gold)
    heat, anno, ind, mask = head.get_targets(boxes, labels)
    T = len(R.LAYOUTS[layout])
    assert len(heat) == len(anno) == len(ind) == len(mask) == T
    worst = 0.0
    for t in range(T):
        g = {k: gold[f'{layout}.{k}.{t}'] for k in ('heatmap', 'anno_box', 'ind', 'mask')}
        assert ind[t].dtype == torch.int64 and mask[t].dtype == torch.uint8 and anno[t].dtype == heat[t].dtype == torch.float32
        assert ind[t].is_cuda and tuple(heat[t].shape) == g['heatmap'].shape == (R.B, len(R.LAYOUTS[layout][t]), R.H, R.W)
        assert np.array_equal(ind[t].cpu().numpy(), g['ind']) and np.array_equal(mask[t].cpu().numpy(), g['mask'])
        assert heat[t].cpu().numpy().tobytes() == g['heatmap'].tobytes()
        a = anno[t].cpu().numpy()
        assert a[..., :3].tobytes() == g['anno_box'][..., :3].tobytes()
        # log / sin / cos: within 4 eps max(1, |v|) of the float64 value of the float32 inputs (ROCm documents logf, sinf, cosf
        # at <= 2 ulp, the float64 value rounds within 1/2 ulp: the bound is twice that sum)
        slots, off = gold[f'{layout}.slot_obj'][t], gold['frame_offsets']
        live = g['mask'].astype(bool)
        assert (a[~live] == 0).all()
        for b, k in zip(*np.nonzero(live)):
            want = R.anno_ref64(gold['boxes'][off[b] + slots[b, k]][None])[0]
            got = a[b, k, 3:].astype(np.float64)
            assert (np.isnan(want) == np.isnan(got)).all()
            ok = ~np.isnan(want)
            ratio = np.abs(got[ok] - want[ok]) / (EPS * np.maximum(1.0, np.abs(want[ok])))
            worst = max(worst, float(ratio.max()))
    print(f'center_targets[{layout}]: largest |anno_box[3:8] - float64| = {worst:.3f} eps max(1, |v|)')
    assert worst <= 4.0


def test_targets_hold_the_cases(gold):
    """What the golden file is for (the generator asserts the same of the reference's outputs)."""
    head = make_head('A')
    heat, anno, ind, mask = head.get_targets(*frames_of(gold))
    m = [x.cpu().numpy() for x in mask]
    assert all(x[0].sum() == 0 for x in m) and all(float(h[0].abs().sum()) == 0 for h in heat)       # the empty frame
    assert m[2][1].tolist() == [1, 1, 1, 1] and int((gold['labels'][gold['frame_offsets'][1]:gold['frame_offsets'][2]] == 2).sum()) == 6
    assert int((heat[2][1] == 1).sum()) == 4                                                       # the two cars past K are not splatted
    assert m[0][1].tolist() == [0, 1, 0, 0] and m[1][1].tolist() == [0, 0, 1, 0]                   # off the map on each side
    assert m[0][2].tolist() == [0, 1, 0, 0] and m[1][2].tolist() == [0, 1, 0, 0]                   # width 0, negative length
    assert bool(torch.isnan(anno[1][2, 1, 5])) and int(torch.isnan(anno[1]).sum()) == 1            # dz < 0
    assert int(ind[2][2, 0]) == int(ind[2][2, 1]) and m[2][2, :2].tolist() == [1, 1]               # two objects, one cell
    assert int((heat[2][2] == 1).sum()) == 3                                                       # ... and one peak for both
    hb = make_head('B').get_targets(*frames_of(gold))[0]                                          # a two-channel heat map
    assert tuple(hb[0].shape) == (R.B, 2, R.H, R.W) and float(hb[0][:, 0].sum()) > 0 and float(hb[0][:, 1].sum()) > 0


def _slots_numpy(labels, num_classes, K):
    """(task, slot) of every object of one frame: class-major, then index order; slot -1 past K or without a task."""
    base = np.concatenate([[0], np.cumsum(num_classes)])
    task = np.full(len(labels), -1)
    slot = np.full(len(labels), -1)
    for t in range(len(num_classes)):
        order = [i for c in range(base[t], base[t + 1]) for i in np.flatnonzero(labels == c)]
        for k, i in enumerate(order[:K]):
            task[i], slot[i] = t, k
    return task, slot


@pytest.mark.parametrize('n_obj', [1, 255, 256, 257, 700])
def test_targets_rank_more_objects_than_a_workgroup_has_threads(n_obj):
    """Frames with up to several tiles of 256 objects (the ranks are counted tile by tile), K = 64, a two-class and a
    one-class task: ``ind`` / ``mask`` against a numpy restatement of the slot order; every centre is well inside its cell."""
    tc = dict(R.TRAIN_CFG, max_objs=64)
    rng = np.random.RandomState(n_obj)
    counts = [n_obj, 0, max(n_obj // 3, 1)]
    boxes, labels = [], []
    for n in counts:
        cx, cy = rng.randint(0, R.W, n), rng.randint(0, R.H, n)
        b = np.zeros((n, 7), np.float32)
        b[:, 0], b[:, 1] = (cx + 0.5) * 0.4, -9.6 + (cy + 0.5) * 0.4
        b[:, 2], b[:, 3], b[:, 4], b[:, 5] = -1.0, 0.8, 0.6, 1.5
        boxes.append(b)
        labels.append(rng.randint(-1, 4, n).astype(np.int64))                   # -1 and 3: no task
    prm = F.center_params(tc, [2, 1])
    up = F.upload_many(dict(boxes=np.concatenate(boxes), labels=np.concatenate(labels),
                            off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)), DEV)
    heat, anno, ind, mask = F.center_targets(up['boxes'], up['labels'], up['off'], prm, max_radius=16)
    ind, mask = ind.cpu().numpy(), mask.cpu().numpy()
    want_ind, want_mask = np.zeros_like(ind), np.zeros_like(mask)
    for f, (b, l) in enumerate(zip(boxes, labels)):
        task, slot = _slots_numpy(l, [2, 1], 64)
        for i in np.flatnonzero(slot >= 0):
            cx, cy = int(b[i, 0] / 0.4), int((b[i, 1] + 9.6) / 0.4)
            want_ind[task[i], f, slot[i]], want_mask[task[i], f, slot[i]] = cy * R.W + cx, 1
    assert np.array_equal(mask, want_mask) and np.array_equal(ind, want_ind)
    live = anno[torch.from_numpy(mask.astype(bool)).to(DEV)]
    assert len(live) == int(want_mask.sum()) and (len(live) == 0 or float(live[:, :2].sub(0.5).abs().max()) < 1e-3)
    assert float(heat.max()) <= 1.0 and (int((heat == 1).sum()) >= 1) == bool(want_mask.any())


# ----------------------------------------------------------------------------- loss
def golden_targets(gold, layout):
    T = len(R.LAYOUTS[layout])
    return [[torch.from_numpy(gold[f'{layout}.{k}.{t}']).to(DEV) for t in range(T)] for k in ('heatmap', 'anno_box', 'ind', 'mask')]


def device_loss(head, preds, targets):
    leaves = [[{k: v.to(DEV).requires_grad_(True) for k, v in pd[0].items()}] for pd in preds]
    losses = head.loss_from_targets(leaves, *targets)
    torch.stack(list(losses.values())).sum().backward()
    return losses, leaves


@pytest.mark.parametrize('layout', ['A', 'B'])
def test_loss_and_gradients_against_float64(layout, gold):
    head = make_head(layout)
    targets = golden_targets(gold, layout)
    preds = R.synth_preds(layout)
    losses, leaves = device_loss(head, preds, targets)
    T = len(preds)
    assert list(losses) == [f'task{t}.{k}' for t in range(T) for k in ('loss_heatmap', 'loss_bbox')]
    p64 = [[{k: v.double().requires_grad_(True) for k, v in pd[0].items()}] for pd in preds]
    cpu = [[x.cpu() for x in xs] for xs in targets]
    ref = R.loss_ref(p64, *cpu, R.TRAIN_CFG['code_weights'], R.LOSS_WEIGHT, **R.LOSS_CLS[layout])
    torch.stack(list(ref.values())).sum().backward()
    for k in ref:
        got, want, golden = float(losses[k]), float(ref[k]), float(gold[f'{layout}.{k}'])
        print(f'{layout} {k}: device {got:.9g} float64 {want:.9g} reference {golden:.9g}')
        assert np.isfinite(got)
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)
        if np.isfinite(golden):
            np.testing.assert_allclose(got, golden, rtol=1e-5, atol=1e-7)
        else:      # 0 * |pred - NaN| in the reference's product: the task with the dz < 0 object, and only that one
            assert k.endswith('loss_bbox') and bool(torch.isnan(cpu[1][int(k[4])]).any())
    for t in range(T):
        for key in ('heatmap', 'reg', 'height', 'dim', 'rot'):
            g, w = leaves[t][0][key].grad.cpu().numpy(), p64[t][0][key].grad.numpy()
            assert np.isfinite(g).all() and float(np.abs(w).max()) > 0
            np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-7 * float(np.abs(w).max()), err_msg=f'task {t} {key}')


def test_two_objects_in_one_cell_and_the_nan_target(gold):
    head = make_head('A')
    targets = golden_targets(gold, 'A')
    preds = R.synth_preds('A')
    _, leaves = device_loss(head, preds, targets)
    p64 = [[{k: v.double().requires_grad_(True) for k, v in pd[0].items()}] for pd in preds]
    cpu = [[x.cpu() for x in xs] for xs in targets]
    ref = R.loss_ref(p64, *cpu, R.TRAIN_CFG['code_weights'], R.LOSS_WEIGHT, **R.LOSS_CLS['A'])
    torch.stack(list(ref.values())).sum().backward()
    # task 2, frame 2, slots 0 and 1 share a cell: its gradient is the sum of both slots' terms
    cell = int(cpu[2][2][2, 0])
    assert cell == int(cpu[2][2][2, 1])
    y, x = divmod(cell, R.W)
    for key in ('reg', 'height', 'dim', 'rot'):
        g, w = leaves[2][0][key].grad[2, :, y, x].cpu().numpy(), p64[2][0][key].grad[2, :, y, x].numpy()
        np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-7 * float(p64[2][0][key].grad.abs().max()))
    # task 1, frame 2, slot 1: log dz is NaN - no gradient on that channel, the other seven as in float64
    assert bool(torch.isnan(cpu[1][1][2, 1, 5]))
    y, x = divmod(int(cpu[2][1][2, 1]), R.W)
    assert float(leaves[1][0]['dim'].grad[2, 2, y, x]) == 0.0 and float(p64[1][0]['dim'].grad[2, 2, y, x]) == 0.0
    assert float(leaves[1][0]['dim'].grad[2, 0, y, x]) != 0.0 and float(leaves[1][0]['rot'].grad[2, 1, y, x]) != 0.0
    assert all(torch.isfinite(leaves[1][0][k].grad).all() for k in leaves[1][0])


@pytest.mark.parametrize('layout', ['A', 'B'])
def test_tasks_share_a_launch_bit_for_bit_and_runs_repeat(layout, gold):
    heat, anno, ind, mask = golden_targets(gold, layout)
    T = len(anno)
    w = F.center_loss_weights(R.TRAIN_CFG['code_weights'], R.LOSS_WEIGHT)
    preds = [R.synth_map((R.B, R.K, 8), 7 + t).to(DEV) for t in range(T)]

    def run(tasks):
        p = [preds[t].clone().requires_grad_(True) for t in tasks]
        out = F.center_reg_loss_tasks(p, [anno[t] for t in tasks], [mask[t] for t in tasks], w)
        torch.stack(list(out)).sum().backward()
        return [bits(o) for o in out], [bits(x.grad) for x in p]

    together = run(range(T))
    assert run(range(T)) == together                                              # two runs: the same bits
    for t in range(T):
        alone = run([t])
        assert alone[0][0] == together[0][t] and alone[1][0] == together[1][t]      # a task does not see its neighbours
    rev = run(list(range(T))[::-1])
    assert rev[0][::-1] == together[0] and rev[1][::-1] == together[1]
    # an upstream gradient other than one, and a task nobody differentiates
    p = [preds[t].clone().requires_grad_(True) for t in range(T)]
    out = F.center_reg_loss_tasks(p, anno, mask, w)
    (out[0] * 3.0).backward()
    assert p[1].grad is None
    q = preds[0].clone().requires_grad_(True)
    F.center_reg_loss_tasks([q], anno[:1], mask[:1], w)[0].backward()
    np.testing.assert_allclose(p[0].grad.cpu().numpy(), 3.0 * q.grad.cpu().numpy(), rtol=1e-6)
    # a whole head: the grouped path against task-by-task calls of loss_from_targets
    head = make_head(layout)
    full, _ = device_loss(head, R.synth_preds(layout), (heat, anno, ind, mask))
    for t in range(T):
        pd = [[{k: v.to(DEV) for k, v in R.synth_preds(layout)[t][0].items()}]]
        one = head.loss_from_targets(pd, [heat[t]], [anno[t]], [ind[t]], [mask[t]])
        assert bits(one['task0.loss_bbox']) == bits(full[f'task{t}.loss_bbox'])
        assert bits(one['task0.loss_heatmap']) == bits(full[f'task{t}.loss_heatmap'])


# ----------------------------------------------------------------------------- train step
def test_two_iterations_of_train_detector_and_evaluate(tmp_path):
    from gga_amd import build_model
    from gga_amd.apis import single_gpu_test
    from gga_amd.cnn import to_channels_last
    from gga_amd.train import train_detector
    from test_center_head import pseudo_infos
    from test_loader import CLASSES, kitti_tree, matching_cfg
    pp = os.path.join(REPO, 'configs', 'gga', 'gga_kitti_pointpillars_config.py')
    infos = kitti_tree(str(tmp_path))
    cfg = Config.fromfile(pp)
    retrain = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_retrain_centerpoint.py'))
    m = cfg.model
    m['type'] = 'CenterPoint'
    m.pts_middle_encoder['channels_last'] = True
    head = dict(m['pts_bbox_head'], type='CenterHead')
    head.pop('loss_center', None)
    m['pts_bbox_head'] = head
    m.train_cfg['pts']['code_weights'] = [1.0] * 8
    rng = list(m.pts_voxel_layer['point_cloud_range'])
    pipe = copy.deepcopy(list(retrain.data['train']['dataset']['pipeline']))
    for t in pipe:
        if 'point_cloud_range' in t:
            t['point_cloud_range'] = rng
    train = dict(type='RepeatDataset', times=2,
                 dataset=dict(type='KittiDataset', data_root=str(tmp_path), ann_file=pseudo_infos(), split='training', pts_prefix='velodyne',
                              pipeline=pipe, modality=dict(use_lidar=True, use_camera=False), classes=CLASSES, test_mode=False))
    cfg.data = dict(samples_per_gpu=3, workers_per_gpu=0, train=train)
    cfg.runner = dict(type='EpochBasedRunner', max_epochs=1)
    cfg.work_dir, cfg.seed = str(tmp_path / 'work'), 0
    cfg.checkpoint_config = dict(interval=1)
    import random
    random.seed(0), np.random.seed(0), torch.manual_seed(0), torch.cuda.manual_seed_all(0)
    model = build_model(cfg.model)
    assert type(model).__name__ == 'CenterPoint' and type(model.pts_bbox_head).__name__ == 'CenterHead'
    with torch.no_grad():          # a random-init detector with finite box sizes that reports boxes (tests/test_validate_gpu.py)
        for th in model.pts_bbox_head.task_heads:
            for name in ('reg', 'height', 'dim', 'rot'):
                getattr(th, name)[-1].weight.mul_(0.05)
            th.heatmap[-1].bias.fill_(0.5)
    model.CLASSES = tuple(CLASSES)
    model = to_channels_last(model.to(DEV)).train()
    seen = []
    model.register_forward_hook(lambda mod, args, out: seen.append(out) if mod.training else None)
    ds = LD.build_dataset(copy.deepcopy(cfg.data['train']))
    runner = train_detector(model, ds, cfg, distributed=False, validate=False, device=torch.device(DEV))
    torch.cuda.synchronize()
    assert runner.iter == 2 and len(seen) == 2
    want = {f'task{t}.{k}' for t in range(3) for k in ('loss_heatmap', 'loss_bbox')}
    for losses in seen:
        assert set(losses) == want and all(bool(torch.isfinite(v).all()) for v in losses.values())
    assert any(float(v) > 0 for k, v in seen[-1].items() if k.endswith('loss_bbox'))
    for name, p in model.pts_bbox_head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    # the test run of tools/test.py --eval mAP on the same frames
    val_cfg = dict(matching_cfg(str(tmp_path), infos, pp).data['test'], type='KittiDataset', test_mode=True)
    val = LD.build_dataset(val_cfg)
    assert type(val).__name__ == 'KittiDataset'
    loader = LD.build_dataloader(val, samples_per_gpu=2, workers_per_gpu=0, dist=False, shuffle=False)
    outs = single_gpu_test(runner.raw_model.eval(), loader, torch.device(DEV), planes=runner.planes)
    assert len(outs) == 3 and set(outs[0]) == {'pts_bbox'}
    ap = val.evaluate(outs, device=DEV)
    assert all(k.startswith('pts_bbox/KITTI/') for k in ap) and 'pts_bbox/KITTI/Overall_3D_AP11_moderate' in ap
    assert all(np.isfinite(v) for v in ap.values())
