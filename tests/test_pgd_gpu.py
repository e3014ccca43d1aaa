"""PGDHead (configs/gga/gga_pdg.py) against a run of the reference's own
PGDHead / FCOSMono3DHead / coders / camera boxes (tests/golden/pgd_head.npz from
tools_dev/make_golden.py::golden_pgd): forward with shared weights, per-level targets (labels exact),
the loss dict and the gradients w.r.t. every prediction tensor."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from gga_amd.box3d import CameraInstance3DBoxes
from gga_amd.registry import build_head

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IMG_HW = (128, 384)     # tools_dev/make_golden.py PGD_IMG

HEAD_CFG = dict(
    type='PGDHead', num_classes=3, in_channels=32, stacked_convs=2, feat_channels=32, use_direction_classifier=True,
    diff_rad_by_sin=True, pred_attrs=False, pred_velo=False, pred_bbox2d=True, pred_keypoints=True, dir_offset=0.7854,
    strides=(4, 8, 16, 32), regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 1e8)), group_reg_dims=(2, 1, 3, 1, 16, 4),
    cls_branch=(32, ), reg_branch=((32, ), (32, ), (32, ), (32, ), (32, ), (32, )), dir_branch=(32, ),
    attr_branch=(32, ), centerness_branch=(32, ), weight_branch=((32, ), ), bbox_code_size=7, use_onlyreg_proj=True, norm_on_bbox=True,
    centerness_on_reg=True, center_sampling=True, conv_bias=True, dcn_on_last_conv=False, norm_cfg=None,
    loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
    loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0),
    loss_dir=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
    loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0), use_depth_classifier=True,
    depth_branch=(32, ), depth_range=(0, 70), depth_unit=10, division='uniform', depth_bins=8, weight_dim=1,
    loss_depth=dict(type='UncertainSmoothL1Loss', alpha=1.0, beta=3.0, loss_weight=1.0),
    bbox_coder=dict(type='PGDBBoxCoder', base_depths=((28.01, 16.32), ),
                    base_dims=((0.8, 1.73, 0.6), (1.76, 1.73, 0.6), (3.9, 1.56, 1.6)), code_size=7),
    train_cfg=dict(code_weight=[1.0] * 7 + [0.2] * 16 + [1.0] * 4),
    test_cfg=dict(nms_pre=100, nms_thr=0.05, score_thr=0.001, max_per_img=20))


@pytest.fixture(scope='module')
def head_and_golden(golden):
    g = golden('pgd_head')
    head = build_head(dict(HEAD_CFG))
    sd = {k[len('state.'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('state.')}
    missing, unexpected = head.load_state_dict(sd, strict=True), None      # same parameter names as the reference head
    head.to(DEV).train()
    return head, g


def test_state_dict_names_and_forward(head_and_golden):
    head, g = head_and_golden
    feats = [torch.from_numpy(g[f'fwd.feat.{i}']).to(DEV) for i in range(4)]
    out = head(feats)
    assert len(out) == 7
    for name, lst in zip(('cls', 'bbox', 'dir', 'depth', 'weight', 'attr', 'cen'), out):
        for i, t in enumerate(lst):
            if name == 'attr':
                assert t is None
                continue
            want = torch.from_numpy(g[f'fwd.{name}.{i}'])
            got = t.detach().cpu()
            if name == 'bbox':       # the size priors follow argmax(cls): compare sizes only where that argmax has a margin
                top2 = torch.from_numpy(g[f'fwd.cls.{i}']).topk(2, dim=1)[0]
                clear = ((top2[:, 0] - top2[:, 1]) > 1e-3).unsqueeze(1)
                assert float(clear.float().mean()) > 0.5
                keep = torch.ones_like(want, dtype=torch.bool)
                keep[:, 3:6] = clear
                got, want = got[keep], want[keep]
            torch.testing.assert_close(got, want, rtol=2e-4, atol=2e-4, msg=f'{name}.{i}')


@pytest.mark.parametrize('seed', [81, 82, 83])
def test_targets_losses_and_gradients(head_and_golden, seed):
    head, g = head_and_golden
    B = 2
    gts = [{k: torch.from_numpy(g[f'{seed}.gt.{b}.{k}']).to(DEV) for k in ('gt_bboxes', 'gt_labels', 'gt_bboxes_3d', 'gt_labels_3d',
                                                                          'centers2d', 'depths')} for b in range(B)]
    preds = {k: [torch.from_numpy(g[f'{seed}.pred.{k}.{i}']).to(DEV).requires_grad_(True) for i in range(4)]
             for k in ('cls', 'bbox', 'dir', 'depth', 'weight', 'cen')}
    img_metas = [dict(cam2img=g[f'{seed}.cam2img'].tolist(), box_type_3d=CameraInstance3DBoxes) for _ in range(B)]
    lists = lambda k: [gt[k] for gt in gts]
    points = head.get_points([t.shape[-2:] for t in preds['cls']], torch.float32, torch.device(DEV))
    tg = head.get_targets(points, lists('gt_bboxes'), lists('gt_labels'), lists('gt_bboxes_3d'), lists('gt_labels_3d'),
                          lists('centers2d'), lists('depths'), None)
    for name, lst in zip(('labels_3d', 'bbox_targets_3d', 'centerness', 'attr'), tg):
        for i, t in enumerate(lst):
            want = g[f'{seed}.tg.{name}.{i}']
            if t.dtype == torch.int64:
                assert np.array_equal(t.cpu().numpy(), want), (name, i)         # integer work: exact
            else:
                np.testing.assert_allclose(t.cpu().numpy(), want, rtol=2e-6, atol=1e-6, err_msg=f'{name}.{i}')
    # the caller's boxes are not edited (the reference turns their yaw local in place)
    assert torch.equal(gts[0]['gt_bboxes_3d'].cpu(), torch.from_numpy(g[f'{seed}.gt.0.gt_bboxes_3d']))
    losses = head.loss(preds['cls'], preds['bbox'], preds['dir'], preds['depth'], preds['weight'], [None] * 4, preds['cen'],
                       lists('gt_bboxes'), lists('gt_labels'), lists('gt_bboxes_3d'), lists('gt_labels_3d'), lists('centers2d'),
                       lists('depths'), None, img_metas)
    want_keys = sorted(k[len(f'{seed}.loss.'):] for k in g.files if k.startswith(f'{seed}.loss.'))
    assert sorted(losses) == want_keys
    for k in want_keys:
        assert float(losses[k]) == pytest.approx(float(g[f'{seed}.loss.{k}']), rel=1e-4, abs=1e-5), k
    head.fuse_lambda.grad = None
    sum(losses.values()).backward()
    for k, lst in preds.items():
        for i, t in enumerate(lst):
            want = torch.from_numpy(g[f'{seed}.grad.{k}.{i}'])
            got = t.grad.cpu() if t.grad is not None else torch.zeros_like(want)
            scale = float(want.abs().max()) + 1e-12
            assert float((got - want).abs().max()) <= 1e-4 * scale + 1e-7, (k, i)
    assert float(head.fuse_lambda.grad) == pytest.approx(float(g[f'{seed}.grad.fuse_lambda']), rel=1e-3, abs=1e-6)


def test_get_bboxes_matches_reference(head_and_golden):
    """Inference (pgd_head.py:878-1130 + box3d_nms.py:8-127) on the golden forward features: same detections
    in the same order as the reference head's ``get_bboxes``."""
    head, g = head_and_golden
    saved = head.conv_cls.bias.detach().clone()
    try:
        head.eval()
        with torch.no_grad():
            head.conv_cls.bias.copy_(torch.from_numpy(g['inf.conv_cls.bias']))
            out = head([torch.from_numpy(g[f'fwd.feat.{i}']).to(DEV) for i in range(4)])
            metas = [dict(cam2img=g['81.cam2img'].tolist(), box_type_3d=CameraInstance3DBoxes, scale_factor=1.0,
                          img_shape=(IMG_HW[0], IMG_HW[1], 3)) for _ in range(2)]
            dets = head.get_bboxes(*out, metas, cfg=dict(use_rotate_nms=True, nms_pre=100, nms_thr=0.05, score_thr=0.004,
                                                         max_per_img=20))
    finally:
        with torch.no_grad():
            head.conv_cls.bias.copy_(saved)
        head.train()
    for i, (bboxes, scores, labels, attrs, bboxes2d) in enumerate(dets):
        assert attrs is None
        want_scores = torch.from_numpy(g[f'inf.{i}.scores'])
        assert scores.shape == want_scores.shape and len(scores) > 0
        torch.testing.assert_close(scores.cpu(), want_scores, rtol=1e-4, atol=1e-6)         # the sorted score list
        # detections with (nearly) tied scores may come out in either order: pair each reference detection with
        # its produced one and compare pairwise
        want_boxes, got_boxes = torch.from_numpy(g[f'inf.{i}.bboxes']), bboxes.tensor.cpu()
        match = torch.cdist(want_boxes, got_boxes).argmin(dim=1)
        assert sorted(match.tolist()) == list(range(len(scores))), 'not a one-to-one pairing'
        moved = (match != torch.arange(len(match))).nonzero().flatten()
        assert all(abs(float(want_scores[j] - want_scores[match[j]])) < 1e-4 * float(want_scores[j]) for j in moved), \
            'order differs between detections whose scores are not tied'
        torch.testing.assert_close(got_boxes[match], want_boxes, rtol=2e-4, atol=2e-4)
        torch.testing.assert_close(scores.cpu()[match], want_scores, rtol=1e-4, atol=1e-6)
        assert torch.equal(labels.cpu()[match], torch.from_numpy(g[f'inf.{i}.labels']))
        torch.testing.assert_close(bboxes2d.cpu()[match], torch.from_numpy(g[f'inf.{i}.bboxes2d']), rtol=2e-4, atol=2e-3)


def test_pgd_config_head_builds_with_dcn():
    """bbox_head of configs/gga/gga_pdg.py (over configs/_base_/models/pgd.py: GN towers, DCNv2 on the last tower
    convs) builds through the registry and runs forward + backward on the HIP DCN path."""
    from gga_amd.dcn import ModulatedDeformConv2dPack
    wide = lambda v: (256, ) if v == (32, ) else tuple((256, ) for _ in v) if isinstance(v, tuple) and v and isinstance(v[0], tuple) else v
    cfg = {k: wide(v) if k.endswith('_branch') else v for k, v in HEAD_CFG.items()}
    cfg.update(in_channels=256, feat_channels=256, dcn_on_last_conv=True)
    cfg.pop('norm_cfg')                       # default GN(32)
    head = build_head(cfg).to(DEV).train()
    head.init_weights()
    assert isinstance(head.cls_convs[-1].conv, ModulatedDeformConv2dPack) and isinstance(head.reg_convs[-1].conv, ModulatedDeformConv2dPack)
    assert isinstance(head.cls_convs[0].gn, torch.nn.GroupNorm)
    feats = [torch.randn(2, 256, 128 // s, 384 // s, device=DEV, requires_grad=True) for s in (4, 8, 16, 32)]
    out = head(feats)
    assert out[1][0].shape == (2, 27, 32, 96) and out[3][0].shape == (2, 8, 32, 96)
    sum(t.sum() for lst in out for t in lst if t is not None).backward()
    assert all(f.grad is not None and torch.isfinite(f.grad).all() for f in feats)
    assert head.cls_convs[-1].conv.conv_offset.weight.grad is not None


def test_fcos_mono3d_train_step_learns():
    """configs/gga/gga_pdg.py end to end (ResNet-101 + FPN + PGDHead with DCNv2, SGD with the config's paramwise
    multipliers, warm-up, gradient clipping) on synthetic KITTI-mono3d batches: finite losses with every key of
    the reference's loss dict, and the total falls."""
    from gga_amd import Config, build_model, synthetic
    from gga_amd.cnn import to_channels_last
    from gga_amd.train import Runner
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_pdg.py'))
    torch.manual_seed(0)
    model = to_channels_last(build_model(cfg.model).to(DEV))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')        # the backbone's model-zoo checkpoint cannot be fetched here
        model.init_weights()
    synthetic.damp_random_backbone(model)
    model.train()
    runner = Runner(model, cfg, max_iters=100, iters_per_epoch=10)
    b = synthetic.make_mono_batch(2, device=DEV, img_hw=(192, 640))
    data = {k: b[k] for k in synthetic.MONO_BATCH_KEYS}
    data['img'] = data['img'].contiguous(memory_format=torch.channels_last)
    out = runner.step(data)
    assert set(out['log_vars']) == {'loss_cls', 'loss_offset', 'loss_size', 'loss_rotsin', 'loss_dir', 'loss_depth', 'loss_kpts',
                                    'loss_bbox2d', 'loss_consistency', 'loss_centerness', 'loss'}
    first = float(out['loss'])
    for _ in range(12):
        out = runner.step(data)
    last = float(out['loss'])
    assert np.isfinite(first) and np.isfinite(last) and last < first, (first, last)
    assert runner.optimizer.param_groups[0]['lr'] < 0.002 and runner.iter == 13


def test_level_streams_and_prepared_targets_change_nothing(monkeypatch):
    """The PGD step's scheduling measures are invisible in the numbers: the head layer by layer with one convolution
    launch over all FPN levels (mono3d_heads.LEVEL_BATCH) or one stream per level (LEVEL_STREAMS), and the target side of
    the loss computed before the forward pass
    (PGDHead.prepare_loss, with the FPN sizes predicted from the image shape). Losses and gradients of one step with
    both, against one stream and targets computed inside ``loss`` from the actual maps."""
    from gga_amd import Config, build_model, synthetic, mono3d_heads
    from gga_amd.cnn import to_channels_last
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_pdg.py'))
    torch.manual_seed(0)
    model = to_channels_last(build_model(cfg.model).to(DEV))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')        # the backbone's model-zoo checkpoint cannot be fetched here
        model.init_weights()
    synthetic.damp_random_backbone(model)
    model.train()
    b = synthetic.make_mono_batch(2, device=DEV, img_hw=(192, 640))
    data = {k: b[k] for k in synthetic.MONO_BATCH_KEYS}
    data['img'] = data['img'].contiguous(memory_format=torch.channels_last)
    # the predicted level sizes are the sizes of the maps the neck delivers
    with torch.no_grad():
        feats = model.extract_feat(data['img'])
    assert model.bbox_head.featmap_sizes_of(data['img'].shape) == [tuple(f.shape[-2:]) for f in feats]

    def one_step(mode, prepared):
        monkeypatch.setattr(mono3d_heads, 'LEVEL_BATCH', mode == 'batch')
        monkeypatch.setattr(mono3d_heads, 'LEVEL_STREAMS', mode == 'streams')
        if not prepared:       # the detector only prepares when the head offers it
            monkeypatch.setattr(type(model.bbox_head), 'prepare_loss_before_forward', False, raising=False)
        else:
            monkeypatch.setattr(type(model.bbox_head), 'prepare_loss_before_forward', True, raising=False)
        model.zero_grad(set_to_none=True)
        out = model.train_step(data)
        out['loss'].backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        return {k: float(v) for k, v in out['log_vars'].items()}, grads

    bn_state = {k: v.clone() for k, v in model.state_dict().items()}
    l0, g0 = one_step('plain', False)
    for mode in ('batch', 'streams'):      # the shipped form (one launch over the levels), and one stream per level
        model.load_state_dict(bn_state)
        l1, g1 = one_step(mode, True)
        assert l1.keys() == l0.keys()
        for k in l1:
            assert abs(l1[k] - l0[k]) <= 1e-5 * abs(l0[k]) + 1e-7, (mode, k, l1[k], l0[k])
        assert g1.keys() == g0.keys()
        # Two steps of the same inputs are not bit-identical (global float atomics in DCN col2im and the target scatter order
        # their additions differently from run to run; the one-launch form runs other tile shapes), and below the head sit 101
        # random, un-normalised layers: the run-to-run floor is 2e-3 of a parameter's largest gradient element
        # (tools_dev/dbg_pgd_modes.py, the same mode twice) - until ONE ReLU decision at an element near zero falls the other
        # way, which it does in about half the runs whatever the mode: the same alternate gradient then appears (up to 0.1 of
        # the largest element in ~50 backbone parameters, 2.3e-2 of a parameter's norm, 6.7e-4 of the whole gradient's norm).
        # The test therefore bounds norms, which a flipped decision moves little and a scheduling bug (a level read before
        # its stream finished, targets of the wrong level sizes) would not respect.
        num = sum(float((g1[n] - g0[n]).double().pow(2).sum()) for n in g1) ** 0.5
        den = sum(float(g0[n].double().pow(2).sum()) for n in g0) ** 0.5
        assert num <= 2e-3 * den, (mode, num / den)
        for n in g1:
            assert float((g1[n] - g0[n]).norm()) <= 5e-2 * float(g0[n].norm()) + 1e-7, (mode, n)


@pytest.mark.parametrize('planes', [2, 3])
def test_wide_head_with_groupnorm_and_dcn_runs_the_hip_kernels_and_matches_the_reference(planes, monkeypatch):
    """The head at its real width - 256 channels, GroupNorm(32) after every tower convolution, DCNv2 as the
    last convolution of both towers (configs/_base_/models/pgd.py towers) - against a run of the reference's PGDHead with the
    same (name-derived) weights and features (tests/golden/pgd_head_wide.npz; DCNv2 there = oracle/dcn_ref, parity unpinned):
    forward, and the gradients of a fixed linear functional of the outputs w.r.t. the features and the parameters. The
    forward and backward must go through gga_dense_conv3x3_* (tower and branch convolutions), gga_gn_relu_* and the DCN
    sampling kernels - counted."""
    import sys
    sys.path.insert(0, os.path.join(REPO, 'tools_dev'))
    from make_golden import WIDE_C, WIDE_GRAD_KEYS, synth_state, synth_tensor, wide_sample
    from gga_amd import _lib, dense_conv
    from gga_amd.cnn import to_channels_last
    from gga_amd.dcn import ModulatedDeformConv2dPack
    monkeypatch.setattr(dense_conv, 'PLANES', planes)
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'pgd_head_wide.npz'))
    wide = lambda v: (WIDE_C, ) if v == (32, ) else tuple((WIDE_C, ) for _ in v) if isinstance(v, tuple) and v and isinstance(v[0], tuple) else v
    cfg = {k: wide(v) if k.endswith('_branch') else v for k, v in HEAD_CFG.items()}
    cfg.update(in_channels=WIDE_C, feat_channels=WIDE_C, dcn_on_last_conv=True, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True))
    head = build_head(cfg)
    synth_state(head)
    head = to_channels_last(head.to(DEV)).train()
    assert isinstance(head.cls_convs[-1].conv, ModulatedDeformConv2dPack) and isinstance(head.cls_convs[0].gn, torch.nn.GroupNorm)
    L = _lib.lib()
    calls = {}
    for name in ('gga_dense_conv3x3_bn_bwd', 'gga_dense_conv3x3_levels', 'gga_dense_wgrad3x3_block_amax', 'gga_gn_relu_fwd', 'gga_gn_relu_bwd',
                 'gga_dcn_im2col_amax', 'gga_dcn_col2im'):
        if hasattr(L, name):
            def counted(*a, _real=getattr(L, name), _n=name):
                calls[_n] = calls.get(_n, 0) + 1
                return _real(*a)
            monkeypatch.setattr(L, name, counted)
    hw = (64, 192)
    feats = [(synth_tensor(f'feat.{i}', (1, WIDE_C, hw[0] // s, hw[1] // s)) * 0.5).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
             for i, s in enumerate((4, 8, 16, 32))]
    out = head(feats)
    total = 0
    for name, lst in zip(('cls', 'bbox', 'dir', 'depth', 'weight', 'attr', 'cen'), out):
        for i, t in enumerate(lst):
            if t is None:
                continue
            want = torch.from_numpy(g[f'fwd.{name}.{i}'])
            if name == 'bbox':          # sizes carry the prior of argmax(cls): compared where both sides chose the same class
                same = (out[0][i].argmax(1).cpu() == torch.from_numpy(g[f'fwd.cls.{i}']).argmax(1))[:, None].expand_as(want)
                assert same.float().mean() > 0.99
                torch.testing.assert_close(t.detach().cpu()[same], want[same], rtol=2e-3, atol=2e-3)
                continue
            torch.testing.assert_close(t.detach().cpu(), want, rtol=1e-3, atol=1e-3, msg=lambda m: f'{name}.{i}: {m}')
            total = total + (t * synth_tensor(f'coef.{name}.{i}', t.shape).to(DEV)).sum()
    total.backward()
    for i, f in enumerate(feats):
        want = torch.from_numpy(g[f'grad.feat.{i}'])
        err = float((f.grad.cpu() - want).norm() / want.norm())
        assert err < 2e-3, (i, err)
    checked = 0
    for k, p in head.named_parameters():
        if p.grad is not None and any(t in k for t in WIDE_GRAD_KEYS):
            want = torch.from_numpy(g['grad.' + k])
            err = float((wide_sample(k, p.grad.cpu()) - want).norm() / (want.norm() + 1e-12))
            assert err < 3e-3, (k, err)
            checked += 1
    assert checked >= 25
    # the HIP paths ran: dense 3x3 convolutions forward (per level or over the levels) and their weight gradients,
    # fused GroupNorm + ReLU both ways, DCN sampling both ways
    assert calls.get('gga_dense_conv3x3_bn_bwd', 0) + calls.get('gga_dense_conv3x3_levels', 0) >= 8, calls
    assert calls.get('gga_dense_wgrad3x3_block_amax', 0) >= 4 and calls.get('gga_gn_relu_fwd', 0) >= 4 and calls.get('gga_gn_relu_bwd', 0) >= 4, calls
    assert calls.get('gga_dcn_im2col_amax', 0) >= 2, calls


def test_two_ranks_keep_identical_parameters():
    """Two ranks (gloo, sharing the one GPU) step the camera-only detector under DistributedDataParallel with one stream
    per FPN level: after three optimizer steps on different batches every rank holds bit-identical parameters (the
    all-reduced gradients reached every parameter on every rank), different losses (different data), and autograd never
    had to accumulate a gradient on a level stream."""
    import socket
    import subprocess
    import sys
    env = dict(os.environ, GGA_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    for attempt in range(2):       # a launcher that could not start its ranks (rendezvous port taken in between, a rank killed by
        with socket.socket() as s:  # the box) is tried once more; what the ranks REPORT is never retried
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
               '--master-port', str(port), os.path.join(REPO, 'tests', '_ddp_pgd_worker.py')]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        lines = [l for l in out.stdout.splitlines() if l.startswith('RANK ')]
        if out.returncode == 0 and len(lines) == 2:
            break
        print('attempt', attempt, 'rc', out.returncode, out.stdout[-1500:], out.stderr[-3000:])
    assert out.returncode == 0 and len(lines) == 2, (out.stdout[-2000:], out.stderr[-3000:])
    assert all('identical_across_ranks True' in l and 'accumulate_grad_warnings 0' in l for l in lines), lines
    losses = [float(l.split(' loss ')[1].split()[0]) for l in lines]
    assert losses[0] != losses[1]
