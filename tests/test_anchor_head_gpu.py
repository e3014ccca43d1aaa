"""Anchor3DHead on the GPU: the target, loss and decode kernels (csrc/anchor_head.hip) against the float32 restatement of the
reference's loop and float64 autograd (tests/_anchor_head_ref.py), the batched ``get_bboxes`` against the loop over frames, and two
iterations of ``train_detector`` with ``VoxelNet``."""
import copy
import os

import numpy as np
import pytest
import torch

import _anchor_head_ref as R
from conftest import REPO
from gga_amd import Config
from gga_amd import anchor_head as AH
from gga_amd import functional as F
from gga_amd import loader as LD
from gga_amd.registry import build_head

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = float(np.finfo(np.float32).eps)
EXACT = ('labels', 'label_weights', 'pos', 'dir_targets', 'dir_weights', 'pos_count')
_REF = {}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype).numpy().tobytes()


def ref_targets(aligned, assign_per_class):
    """The restatement's targets of the fixture, computed once per case and shared."""
    key = (aligned, assign_per_class)
    if key not in _REF:
        _REF[key] = R.ref_targets_batch(R.fixture_anchors(aligned), R.GT_BOXES, R.GT_LABELS, R.THRESHOLDS, assign_per_class, R.NUM_CLASSES)
    return _REF[key]


def check_targets(got, want, what):
    """Exact: labels, weights, the positive flag, direction targets, counts and the columns of ``bbox_targets`` made of
    subtractions, divisions and a square root. Columns 3-5 are logarithms of a float32 quotient: against the float64 value t,
    |err| <= EPS * (1 + 4 |t|) - the quotient carries half an ulp, i.e. EPS / 2 absolute in the logarithm, and logf is within 2
    ulp of its result, doubled for margin (measured on the MI355X: at most 0.42 of the bound). -> the largest error in units of
    that bound."""
    for key in EXACT:
        g = got[key].cpu()
        assert g.dtype == want[key].dtype and tuple(g.shape) == tuple(want[key].shape), (what, key)
        assert torch.equal(g, want[key]), (what, key, int((g != want[key]).sum()))
    g, w, w64 = got['bbox_targets'].cpu(), want['bbox_targets'], want['bbox_targets64']
    assert torch.equal(g[..., [0, 1, 2, 6]], w[..., [0, 1, 2, 6]]), what
    err = (g[..., 3:6].double() - w64[..., 3:6]).abs()
    bound = EPS * (1 + 4 * w64[..., 3:6].abs())
    worst = float((err / bound).max())
    print(f'{what}: log columns, max |err| {float(err.max()):.3e}, max err / bound {worst:.3f}')
    assert bool((err <= bound).all()), (what, worst)
    return worst


# ----------------------------------------------------------------------------- targets
@pytest.mark.parametrize('aligned', [True, False])
@pytest.mark.parametrize('assign_per_class', [True, False])
def test_targets_against_the_restatement(aligned, assign_per_class):
    head = build_head(R.head_cfg(aligned, assign_per_class))
    anchors = head.anchor_generator.grid_anchors([R.FEAT], device=DEV)[0]
    assert torch.equal(anchors.cpu(), R.fixture_anchors(aligned))
    got = head.get_targets(anchors, R.GT_BOXES, R.GT_LABELS, device=DEV, bbox_weights=True)
    assert got['labels'].is_cuda
    want = ref_targets(aligned, assign_per_class)
    check_targets(got, want, f'fixture aligned={aligned} per_class={assign_per_class}')
    assert torch.equal(got['bbox_weights'].cpu(), want['pos'].float()[..., None].expand(-1, -1, 7))
    again = head.get_targets(anchors, R.GT_BOXES, R.GT_LABELS, device=DEV)
    assert all(bits(again[k]) == bits(got[k]) for k in EXACT + ('bbox_targets', ))


@pytest.mark.parametrize('G', [1, 63, 64, 65, 200])
def test_targets_at_chunk_and_tail_boundaries(G):
    # a 7 x 5 map: 210 anchors, not a multiple of a wave; the ground truths are staged in chunks of 64
    feat = (7, 5)
    boxes, labels = R.random_boxes(G, 100 + G)
    ref_anchors = R.ref_anchors(feat, R.RANGES, R.SIZES, R.ROTATIONS, True)
    assert ref_anchors.numel() == 210 * 7
    for per_class in (True, False):
        head = build_head(R.head_cfg(True, per_class))
        anchors = head.anchor_generator.grid_anchors([feat], device=DEV)[0]
        gts, lbs = [boxes, torch.zeros(0, 7)], [labels, torch.zeros(0, dtype=torch.long)]
        want = R.ref_targets_batch(ref_anchors, gts, lbs, R.THRESHOLDS, per_class, R.NUM_CLASSES)
        got = head.get_targets(anchors, gts, lbs, device=DEV)
        check_targets(got, want, f'G={G} per_class={per_class}')
        assert int(got['pos_count'][1]) == 0 and (G == 1 or int(want['pos_count'][0]) > 0)      # (one box on this coarse map may match nothing)


def test_labels_out_of_range_take_no_part():
    head = build_head(R.head_cfg(True, False))
    anchors = head.anchor_generator.grid_anchors([R.FEAT], device=DEV)[0]
    extra = torch.tensor([[3.5, 0.3, -1.7, 3.9, 1.6, 1.5, 0.0], [1.6, -1.6, -0.6, 0.8, 0.6, 1.7, 1.57]])
    gts = [torch.cat([extra[:1], R.GT_BOXES[0][:2], extra[1:], R.GT_BOXES[0][2:]]), extra, R.GT_BOXES[2]]
    lbs = [torch.cat([torch.tensor([-1]), R.GT_LABELS[0][:2], torch.tensor([R.NUM_CLASSES]), R.GT_LABELS[0][2:]]),
           torch.tensor([R.NUM_CLASSES, -1]), R.GT_LABELS[2]]
    got = head.get_targets(anchors, gts, lbs, device=DEV)
    clean = head.get_targets(anchors, R.GT_BOXES, R.GT_LABELS, device=DEV)
    for key in EXACT + ('bbox_targets', ):
        assert bits(got[key]) == bits(clean[key]), key


# ----------------------------------------------------------------------------- losses
def loss_maps(seed=0, batch=3):
    H, W = R.FEAT
    return [R.synth_map((batch, 6 * c, H, W), seed + c, s) for c, s in ((3, 1.5), (7, 0.7), (2, 1.0))]


def device_losses(head, maps, targets, channels_last, upstream=(1.0, 1.0, 1.0)):
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    leaves = [m.to(DEV).contiguous(memory_format=fmt).requires_grad_(True) for m in maps]
    lc, lb, ld = head.loss_cls, head.loss_bbox, head.loss_dir
    out = F.anchor_losses(*leaves, targets, head.num_anchors, head.num_classes, lc.gamma, lc.alpha, lb.beta,
                          AH._get(head.train_cfg, 'code_weight', None), (lc.loss_weight, lb.loss_weight, ld.loss_weight),
                          head.diff_rad_by_sin)
    sum(o * u for o, u in zip(out, upstream)).backward()
    return out, leaves


@pytest.mark.parametrize('variant', ['plain', 'code_weight', 'no_sin', 'pos_weight'])
def test_losses_and_gradients_against_float64(variant):
    code_weight = [1.0, 1.0, 0.5, 2.0, 1.0, 1.0, 0.25] if variant == 'code_weight' else None
    extra = dict(code_weight=code_weight) if code_weight else {}
    if variant == 'pos_weight':
        extra['pos_weight'] = 2
    head = build_head(R.head_cfg(True, True, train_cfg_extra=extra, diff_rad_by_sin=variant != 'no_sin'))
    anchors = head.anchor_generator.grid_anchors([R.FEAT], device=DEV)[0]
    targets = head.get_targets(anchors, R.GT_BOXES, R.GT_LABELS, device=DEV)
    want_t = R.ref_targets_batch(R.fixture_anchors(True), R.GT_BOXES, R.GT_LABELS, R.THRESHOLDS, True, R.NUM_CLASSES,
                                 pos_weight=extra.get('pos_weight', -1))
    assert torch.equal(targets['label_weights'].cpu(), want_t['label_weights'])
    maps = loss_maps()
    m64 = [m.double().requires_grad_(True) for m in maps]
    ref = R.ref_losses(*m64, want_t, R.NUM_CLASSES, code_weight=code_weight, diff_rad_by_sin=variant != 'no_sin')
    sum(ref).backward()
    runs = {}
    for channels_last in (False, True):
        out, leaves = device_losses(head, maps, targets, channels_last)
        for name, got, want in zip(('loss_cls', 'loss_bbox', 'loss_dir'), out, ref):
            print(f'{variant} channels_last={channels_last} {name}: device {float(got.detach()):.9g} float64 {float(want.detach()):.9g}')
            assert np.isfinite(float(got))
            np.testing.assert_allclose(float(got), float(want), rtol=1e-5, atol=1e-7)
        for name, leaf, m in zip(('cls_score', 'bbox_pred', 'dir_cls_pred'), leaves, m64):
            assert leaf.grad.stride() == leaf.stride()
            g, w = leaf.grad.cpu().numpy(), m.grad.numpy()
            assert np.isfinite(g).all() and float(np.abs(w).max()) > 0
            np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-7 * float(np.abs(w).max()), err_msg=f'{variant} {name}')
        runs[channels_last] = [bits(o) for o in out] + [bits(l.grad) for l in leaves]      # (.contiguous(): logical order)
    assert runs[False] == runs[True]                                    # the two layouts: the same bits
    out, leaves = device_losses(head, maps, targets, True)
    assert [bits(o) for o in out] + [bits(l.grad) for l in leaves] == runs[True]           # two runs: the same bits
    # an upstream gradient other than one, and a loss nobody differentiates
    out3, leaves3 = device_losses(head, maps, targets, False, upstream=(3.0, 0.0, 1.0))
    np.testing.assert_allclose(leaves3[0].grad.cpu().numpy(), 3.0 * m64[0].grad.numpy(), rtol=1e-5,
                               atol=3e-7 * float(m64[0].grad.abs().max()))
    assert float(leaves3[1].grad.abs().max()) == 0.0


def test_a_batch_without_positives():
    # tests/test_models/test_heads.py:214-221 of the reference: loss_cls > 0, loss_bbox == 0, loss_dir == 0
    head = build_head(R.head_cfg(True, True))
    anchors = head.anchor_generator.grid_anchors([R.FEAT], device=DEV)[0]
    targets = head.get_targets(anchors, [torch.zeros(0, 7)] * 3, [torch.zeros(0, dtype=torch.long)] * 3, device=DEV)
    assert targets['pos_count'].tolist() == [0, 0, 0] and int(targets['pos'].sum()) == 0
    assert bool((targets['labels'] == R.NUM_CLASSES).all()) and bool((targets['label_weights'] == 1).all())
    assert float(targets['bbox_targets'].abs().max()) == 0.0
    out, leaves = device_losses(head, loss_maps(), targets, True)
    assert float(out[0]) > 0 and float(out[1]) == 0.0 and float(out[2]) == 0.0
    want = R.ref_losses(*[m.double() for m in loss_maps()], {k: v.cpu() for k, v in targets.items()}, R.NUM_CLASSES)
    np.testing.assert_allclose(float(out[0]), float(want[0]), rtol=1e-5)
    for leaf in leaves[1:]:
        assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) == 0.0
    assert bool(torch.isfinite(leaves[0].grad).all()) and float(leaves[0].grad.abs().max()) > 0


def test_device_path_equals_the_eager_path(monkeypatch):
    head = build_head(R.head_cfg(True, True, train_cfg_extra=dict(code_weight=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5]))).to(DEV)
    maps = [m.to(DEV).contiguous(memory_format=torch.channels_last) for m in loss_maps()]
    metas = [dict() for _ in range(3)]
    got = {}
    for on in (True, False):
        monkeypatch.setattr(AH, 'DEVICE_TARGETS', on)
        assert head._device_path([maps[0]]) is on
        losses = head.loss([maps[0]], [maps[1]], [maps[2]], R.GT_BOXES, R.GT_LABELS, metas)
        assert list(losses) == ['loss_cls', 'loss_bbox', 'loss_dir'] and all(len(v) == 1 for v in losses.values())
        got[on] = {k: float(v[0]) for k, v in losses.items()}
    for key in got[True]:
        print(f'{key}: device {got[True][key]:.9g} eager {got[False][key]:.9g}')
        np.testing.assert_allclose(got[True][key], got[False][key], rtol=1e-5, atol=1e-7)
    assert head._device_path([maps[0].cpu()]) is False and head._device_path([maps[0], maps[0]]) is False


# ----------------------------------------------------------------------------- get_bboxes
def test_get_bboxes_batched_equals_the_loop(monkeypatch):
    from gga_amd.box3d import CameraInstance3DBoxes, LiDARInstance3DBoxes
    head = build_head(R.head_cfg(True, True)).to(DEV)
    H, W = R.FEAT
    cls = R.synth_map((3, 18, H, W), 5, 1.0) - 1.5
    cls[2] -= 8.0                                           # frame 2: every score far below score_thr
    outs = [[cls.to(DEV).contiguous(memory_format=torch.channels_last)],
            [R.synth_map((3, 42, H, W), 6, 0.3).to(DEV).contiguous(memory_format=torch.channels_last)],
            [R.synth_map((3, 12, H, W), 7, 1.0).to(DEV)]]
    metas = [dict(box_type_3d=LiDARInstance3DBoxes) for _ in range(3)]
    assert head._get_bboxes_batched(*outs, metas) is not None
    fast = head.get_bboxes(*outs, metas)
    monkeypatch.setattr(AH, 'DETECT_BATCHED', False)
    assert head._get_bboxes_batched(*outs, metas) is None
    loop = head.get_bboxes(*outs, metas)
    counts = [len(s) for _, s, _ in loop]
    print('detections per frame:', counts)
    assert counts[2] == 0 and counts[0] > 0 and counts[1] > 0 and max(counts) == 5        # the max_num cut is reached
    for (fb, fs, fl), (lb, ls, ll) in zip(fast, loop):
        assert isinstance(fb, LiDARInstance3DBoxes) and fl.dtype == ll.dtype == torch.int64
        assert bits(fb.tensor) == bits(lb.tensor) and bits(fs) == bits(ls) and torch.equal(fl.cpu(), ll.cpu())
        assert bool((fs > head.test_cfg['score_thr']).all())
    monkeypatch.setattr(AH, 'DETECT_BATCHED', True)
    cam = [dict(box_type_3d=CameraInstance3DBoxes) for _ in range(3)]
    assert head._get_bboxes_batched(*outs, cam) is None         # camera boxes take the loop
    mixed = [metas[0], cam[1], metas[2]]
    assert head._get_bboxes_batched(*outs, mixed) is None
    res = head.get_bboxes(*outs, cam)
    assert len(res) == 3 and all(isinstance(b, CameraInstance3DBoxes) for b, _, _ in res)


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
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_retrain_pointpillars.py'))
    cfg.model['middle_encoder']['channels_last'] = True
    train = dict(type='RepeatDataset', times=2,
                 dataset=dict(type='KittiDataset', data_root=str(tmp_path), ann_file=pseudo_infos(), split='training', pts_prefix='velodyne',
                              pipeline=copy.deepcopy(list(cfg.data['train']['dataset']['pipeline'])),
                              modality=dict(use_lidar=True, use_camera=False), classes=CLASSES, test_mode=False))
    cfg.data = dict(samples_per_gpu=3, workers_per_gpu=0, train=train)
    cfg.runner = dict(type='EpochBasedRunner', max_epochs=1)
    cfg.work_dir, cfg.seed = str(tmp_path / 'work'), 0
    cfg.checkpoint_config = dict(interval=1)
    # two AdamW steps at the schedule's rate move every weight by about the rate, all against the negatives' focal gradient: the
    # random-init detector then reports nothing. A small rate keeps the evaluation below a run with detections in it.
    cfg.optimizer = dict(cfg.optimizer, lr=1e-6)
    import random
    random.seed(0), np.random.seed(0), torch.manual_seed(0), torch.cuda.manual_seed_all(0)
    model = build_model(cfg.model)
    assert type(model).__name__ == 'VoxelNet' and type(model.bbox_head).__name__ == 'Anchor3DHead'
    with torch.no_grad():
        model.bbox_head.conv_cls.bias.fill_(-1.5)           # a random-init detector that reports boxes (prior 0.18 > score_thr)
    model.CLASSES = tuple(CLASSES)
    model = to_channels_last(model.to(DEV)).train()
    seen = []
    model.register_forward_hook(lambda mod, args, out: seen.append(out) if mod.training else None)
    ds = LD.build_dataset(copy.deepcopy(cfg.data['train']))
    runner = train_detector(model, ds, cfg, distributed=False, validate=False, device=torch.device(DEV))
    torch.cuda.synchronize()
    assert runner.iter == 2 and len(seen) == 2
    for losses in seen:
        assert set(losses) == {'loss_cls', 'loss_bbox', 'loss_dir'}
        assert all(len(v) == 1 and bool(torch.isfinite(v[0]).all()) for v in losses.values())
    assert float(seen[-1]['loss_cls'][0].detach()) > 0 and float(seen[-1]['loss_bbox'][0].detach()) > 0
    for name, p in model.bbox_head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    # the test run of tools/test.py --eval mAP on the same frames
    val_cfg = dict(matching_cfg(str(tmp_path), infos, pp).data['test'], type='KittiDataset', test_mode=True)
    val = LD.build_dataset(val_cfg)
    loader = LD.build_dataloader(val, samples_per_gpu=2, workers_per_gpu=0, dist=False, shuffle=False)
    outs = single_gpu_test(runner.raw_model.eval(), loader, torch.device(DEV), planes=runner.planes)
    assert len(outs) == 3 and set(outs[0]) == {'boxes_3d', 'scores_3d', 'labels_3d'}
    assert sum(len(o['scores_3d']) for o in outs) > 0
    ap = val.evaluate(outs, device=DEV)
    assert any(k.endswith('KITTI/Overall_3D_AP11_moderate') for k in ap) and all(np.isfinite(v) for v in ap.values())
