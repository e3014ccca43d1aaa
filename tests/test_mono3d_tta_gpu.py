"""The mono3d test run on the device: flip test-time augmentation (``gga_mono3d_tta_merge`` / ``functional.mono3d_tta_merge``,
``SingleStageMono3DDetector.aug_test``) and the whole-batch ``PGDHead.get_bboxes`` (``gga_multiclass_nms3d`` +
``gga_mono3d_collect``).

* the merge kernel against the reference's sequence (mmdet3d/models/detectors/single_stage_mono3d.py:141-181) restated here with
  torch on the host, frame by frame, and against maps recorded from the reference's own ``aug_test``
  (tests/golden/mono3d_tta.npz, ``tools_dev/make_golden.py mono3d_tta``): bit for bit - with two views the mean is one rounded
  addition and an exact halving, ``1 - x`` one operation;
* the batched detect against the loop over images (``GGA_MONO3D_DETECT_BATCHED=0``): every output field equal;
* end to end from a written KITTI tree with ``configs/gga/gga_pdg_tta.py``'s test pipeline."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu
GROUPS = ('cls_scores', 'bbox_preds', 'dir_cls_preds', 'depth_cls_preds', 'weights', 'attr_preds', 'centernesses')
LEVEL_SETS = ([(1, 4), (3, 5)], [(6, 10), (5, 7), (2, 3), (1, 1)], [(24, 78), (12, 39)])      # W % 4 = 0, 1, 2, 3; a single pixel
DEV = 'cuda:0'


# ------------------------------------------------------------------------------------------------------------ the merge
def head_maps(levels, n_frames, code, optional, seed):
    """Random head output for the view-major [2 F] batch: the seven groups, per level [2 F, C, H, W] (host, float32)."""
    g = torch.Generator().manual_seed(seed)
    channels = (3, code + 4, 2, 8 if optional else None, 1 if optional else None, 9 if optional else None, 1)
    return tuple([None] * len(levels) if c is None else [torch.randn(2 * n_frames, c, h, w, generator=g) for h, w in levels]
                 for c in channels)


def reference_merge(outs, n_frames, pred_velo):
    """single_stage_mono3d.py:141-181 on the host, operation by operation, for each frame on its own (the reference takes one
    frame per call) -> the merged groups with batch ``n_frames``."""
    frames = []
    for f in range(n_frames):
        outs_list = [[None if g[0] is None else [x[v * n_frames + f:v * n_frames + f + 1].clone() for x in g] for g in outs]
                     for v in range(2)]
        for i, flipped in enumerate((False, True)):
            if flipped:
                for j in range(len(outs_list[i])):
                    if outs_list[i][j] is None:
                        continue
                    for k in range(len(outs_list[i][j])):
                        outs_list[i][j][k] = torch.flip(outs_list[i][j][k], dims=[3])
                for reg_feat in outs_list[i][1]:
                    reg_feat[:, 0, :, :] = 1 - reg_feat[:, 0, :, :]
                    if pred_velo:
                        reg_feat[:, 7, :, :] = -reg_feat[:, 7, :, :]
                    reg_feat[:, 6, :, :] = -reg_feat[:, 6, :, :] + np.pi
        merged = []
        for i in range(len(outs_list[0])):
            if outs_list[0][i] is None:
                merged.append(None)
                continue
            feats = []
            for j in range(len(outs_list[0][i])):
                avg = torch.mean(torch.cat([x[i][j] for x in outs_list]), dim=0, keepdim=True)
                if i == 1:
                    avg[:, 6:, :, :] = outs_list[0][i][j][:, 6:, :, :]
                if i == 2:
                    avg = outs_list[0][i][j]
                feats.append(avg)
            merged.append(feats)
        frames.append(merged)
    return tuple(None if g[0] is None else [torch.cat([m[i][j] for m in frames]) for j in range(len(g))] for i, g in enumerate(outs))


def to_dev(outs):
    return tuple([None if x is None else x.to(DEV) for x in g] for g in outs)


def assert_same_maps(got, want, what):
    assert len(got) == len(want) == len(GROUPS)
    for name, g, w in zip(GROUPS, got, want):
        if w is None:
            assert all(x is None for x in g), (what, name)
            continue
        assert len(g) == len(w), (what, name)
        for lvl, (a, b) in enumerate(zip(g, w)):
            assert a.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape), (what, name, lvl, a.shape, b.shape)
            assert torch.equal(a.cpu().contiguous().view(torch.int32), b.contiguous().view(torch.int32)), (what, name, lvl)


@pytest.mark.parametrize('n_frames', [1, 3])
@pytest.mark.parametrize('levels', LEVEL_SETS, ids=['w4w5', 'w10w7w3w1', 'w78w39'])
def test_merge_kernel_equals_the_eager_reference_sequence_bitwise(levels, n_frames):
    from gga_amd import functional as F
    for code in (7, 9):
        for optional in (True, False):
            outs = head_maps(levels, n_frames, code, optional, seed=100 * code + 10 * n_frames + int(optional))
            got = F.mono3d_tta_merge(to_dev(outs), n_frames)
            assert_same_maps(got, reference_merge(outs, n_frames, pred_velo=code == 9), (levels, n_frames, code, optional))


def test_merge_kernel_on_unaligned_sources():
    from gga_amd import functional as F
    levels, n_frames = [(5, 8), (2, 4)], 2            # widths that would take the 16-byte path ...
    outs = head_maps(levels, n_frames, 7, True, seed=7)
    dev = []
    for g in outs:                                    # ... but every source begins one float behind a 16-byte boundary
        group = []
        for x in g:
            flat = torch.empty(x.numel() + 1, device=DEV)
            flat[1:] = x.reshape(-1).to(DEV)
            group.append(flat[1:].view(x.shape))
            assert group[-1].data_ptr() % 16 == 4 and group[-1].is_contiguous()
        dev.append(group)
    assert_same_maps(F.mono3d_tta_merge(tuple(dev), n_frames), reference_merge(outs, n_frames, False), 'unaligned')


def test_merge_kernel_reproduces_the_maps_recorded_from_the_reference():
    from gga_amd import functional as F
    z = np.load(os.path.join(REPO, 'tests', 'golden', 'mono3d_tta.npz'))
    cases = sorted({int(k.split('.')[1]) for k in z.files if k.startswith('levels.')})
    assert len(cases) == 2
    for c in cases:
        n_levels = len(z[f'levels.{c}'])
        have = [f'in.{c}.{g}.0' in z.files for g in GROUPS]
        assert have[:3] == [True] * 3 and have[6]
        outs = tuple([torch.from_numpy(z[f'in.{c}.{g}.{l}']) for l in range(n_levels)] if h else [None] * n_levels for g, h in zip(GROUPS, have))
        want = tuple([torch.from_numpy(z[f'out.{c}.{g}.{l}']) for l in range(n_levels)] if h else None for g, h in zip(GROUPS, have))
        assert_same_maps(F.mono3d_tta_merge(to_dev(outs), 1), want, f'golden case {c}')
    assert any(f'in.{c}.depth_cls_preds.0' not in z.files for c in cases) and any(z[f'in.{c}.bbox_preds.0'].shape[1] == 9 for c in cases)


def test_a_scene_merged_with_its_own_mirror_gives_the_scene_back():
    """View 1 = the mirrored maps with regression channel 0 set to 1 - x: every MEAN map and the regression channels >= 1 come
    back exactly ((a + a) * 0.5 = a). Channel 0 goes through y = fl(1 - a), fl(1 - y), fl(a + .) and the halving: with |a| < 2
    (so |1 - a| < 4, |sum| < 8) the three roundings are at most 2^-23, 2^-23 and 2^-22, halved at the end: 2^-22 in all."""
    from gga_amd import functional as F
    g = torch.Generator().manual_seed(5)
    levels, n_frames = [(6, 10), (3, 5), (2, 4)], 2
    view0 = tuple([torch.rand(n_frames, c, h, w, generator=g) * 4 - 2 for h, w in levels] for c in (3, 11, 2, 8, 1, 9, 1))
    outs = []
    for i, group in enumerate(view0):
        both = []
        for x in group:
            m = x.flip(3).clone()
            if i == 1:
                m[:, 0] = 1 - m[:, 0]
            both.append(torch.cat([x, m]))
        outs.append(both)
    got = F.mono3d_tta_merge(to_dev(tuple(outs)), n_frames)
    for i, (group, want) in enumerate(zip(got, view0)):
        for a, b in zip(group, want):
            a = a.cpu()
            if i == 1:
                worst = float((a[:, 0] - b[:, 0]).abs().max())
                print(f'regression channel 0: worst distance {worst:.3e} (bound {2.0 ** -22:.3e})')
                assert worst <= 2.0 ** -22
                a, b = a[:, 1:], b[:, 1:]
            assert torch.equal(a, b), GROUPS[i]


# ----------------------------------------------------------------------------------------------------- the batched detect
FEATS = ((8, 24), (4, 12), (2, 6), (1, 3))
SETTINGS = dict(cap=dict(score_thr=0.001, max_per_img=5), nocap=dict(score_thr=0.001, max_per_img=200),
                class_empty=dict(score_thr=0.02, max_per_img=200), all_empty=dict(score_thr=0.999, max_per_img=200))


@pytest.fixture(scope='module')
def head():
    from gga_amd import Config
    from gga_amd.registry import build_head
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_pdg.py'))
    h = dict(cfg.model['bbox_head'])
    h.update(train_cfg=None, test_cfg=dict(cfg.model['test_cfg']))
    torch.manual_seed(0)
    return build_head(h).to(DEV).eval()


def detect_inputs(B, seed):
    """Random head outputs (continuous logits: no score ties) on the four levels and metas with one cam2img per image.
    Depths of 10 .. 20 m and sizes of 2 .. 4 m so that BEV boxes overlap; image 1 has no class-1 score worth a candidate
    and image 2 none at all (for the settings with a high threshold)."""
    from gga_amd.box3d import CameraInstance3DBoxes
    g = torch.Generator().manual_seed(seed)
    r = lambda c, h, w: torch.randn(B, c, h, w, generator=g)
    outs = [[], [], [], [], [], [], []]
    for h, w in FEATS:
        cls = r(3, h, w) + 1.0
        if B > 1:
            cls[1, 1] -= 12.0
        if B > 2:
            cls[2] -= 12.0
        box = r(27, h, w)
        box[:, 2] = 10 + 10 * torch.rand(B, h, w, generator=g)
        box[:, 3:6] = 2 + 2 * torch.rand(B, 3, h, w, generator=g)
        box[:, -4:] = 6 * torch.rand(B, 4, h, w, generator=g)
        for group, x in zip(outs, (cls, box, r(2, h, w), 2 * r(8, h, w), 0.3 * r(1, h, w), None, r(1, h, w) + 1.0)):
            group.append(None if x is None else x.to(DEV))
    metas = []
    for b in range(B):
        cam = [[700.0 + 9 * b, 0.0, 47.5 + b, 40.0 + b], [0.0, 700.0 + 9 * b, 16.25 - b, 2.0], [0.0, 0.0, 1.0, 0.003], [0.0, 0.0, 0.0, 1.0]]
        metas.append(dict(cam2img=cam, scale_factor=1.0, img_shape=(32 - b, 96 - 2 * b, 3), box_type_3d=CameraInstance3DBoxes))
    return outs, metas


def fields_of(out):
    boxes, scores, labels, attrs = out[:4]
    return dict(boxes=boxes.tensor.cpu(), scores=scores.cpu(), labels=labels.cpu(), attrs=None if attrs is None else attrs.cpu(),
                boxes2d=out[4].cpu() if len(out) > 4 else None)


def assert_same_detections(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = fields_of(a), fields_of(b)
        for k in a:
            if b[k] is None:
                assert a[k] is None, (what, i, k)
                continue
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, i, k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
            assert torch.equal(a[k], b[k]), (what, i, k)


@pytest.mark.parametrize('setting', list(SETTINGS))
@pytest.mark.parametrize('rotate', [True, False], ids=['rotated', 'axis_aligned'])
@pytest.mark.parametrize('B', [1, 3])
def test_batched_detect_equals_the_loop(head, monkeypatch, B, rotate, setting):
    outs, metas = detect_inputs(B, seed=31 + B)
    cfg = dict(head.test_cfg, nms_pre=20, use_rotate_nms=rotate, **SETTINGS[setting])
    assert FEATS[0][0] * FEATS[0][1] > cfg['nms_pre'] > FEATS[2][0] * FEATS[2][1]
    monkeypatch.setenv('GGA_MONO3D_DETECT_BATCHED', '0')
    loop = head.get_bboxes(*outs, metas, cfg=cfg, rescale=True)
    monkeypatch.setenv('GGA_MONO3D_DETECT_BATCHED', '1')
    batched = head.get_bboxes(*outs, metas, cfg=cfg, rescale=True)
    assert all(o[0].tensor.is_cuda for o in loop) and not any(o[0].tensor.is_cuda for o in batched)     # (which path ran)
    counts = [len(o[1]) for o in loop]
    classes = [sorted(set(o[2].tolist())) for o in loop]
    print(f'B={B} rotate={rotate} {setting}: detections per image {counts}, classes {classes}')
    if setting == 'cap':
        assert max(counts) == cfg['max_per_img'], 'the cap must bind in at least one image'
        assert all((o[1][:-1] >= o[1][1:]).all() for o in loop if len(o[1]) == cfg['max_per_img'])
    elif setting == 'nocap':
        assert max(counts) < cfg['max_per_img'] and any(len(c) >= 2 for c in classes)
    elif setting == 'class_empty':
        assert any(counts)
        if B > 1:
            assert counts[1] > 0 and 1 not in classes[1] and len(classes[0]) == 3
        if B > 2:
            assert counts[2] == 0
    else:
        assert counts == [0] * B
    assert_same_detections(batched, loop, (B, rotate, setting))


# --------------------------------------------------------------------------------------------------------- end to end
def _tta_cfg(root):
    from gga_amd import Config
    from test_kitti_mono_gpu import mono_cfg
    cfg = mono_cfg(root)
    tta = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_pdg_tta.py'))
    for split in ('val', 'test'):
        cfg.data[split]['pipeline'] = copy.deepcopy(tta.data[split]['pipeline'])
    return cfg


def _same_results(got, want):
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b) == {'img_bbox', 'img_bbox2d'}, f
        assert set(a['img_bbox']) == set(b['img_bbox']) == {'boxes_3d', 'scores_3d', 'labels_3d'}
        for k in ('scores_3d', 'labels_3d'):
            x, y = a['img_bbox'][k], b['img_bbox'][k]
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (f, k)
        x, y = a['img_bbox']['boxes_3d'], b['img_bbox']['boxes_3d']
        assert type(x) is type(y) and x.tensor.shape == y.tensor.shape and torch.equal(x.tensor, y.tensor), f
        assert len(a['img_bbox2d']) == len(b['img_bbox2d']) == 3
        for x, y in zip(a['img_bbox2d'], b['img_bbox2d']):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f


def test_tta_test_run_from_a_kitti_root(tmp_path, monkeypatch):
    from gga_amd import functional as F
    from gga_amd import loader as LD
    from gga_amd.apis import generate_pseudo_labels, single_gpu_test
    from test_kitti_mono_gpu import fresh_mono_model
    monkeypatch.setenv('GGA_MONO_IMAGE_DEVICE', '1')
    cfg = _tta_cfg(str(tmp_path))
    model = fresh_mono_model(cfg).eval()
    val = LD.build_dataset(copy.deepcopy(cfg.data['val']))
    loader = LD.build_dataloader(val, samples_per_gpu=2, workers_per_gpu=0, dist=False, shuffle=False)
    # the head's output of every [2 B] batch, once
    batches = []
    with torch.no_grad():
        for batch in loader:
            data = LD.to_step_inputs(batch, torch.device(DEV))
            assert len(data['img']) == 2 and data['img'][0].shape == data['img'][1].shape and data['img'][0].shape[0] == 2
            assert data['img'][0]._base is data['img'][1]._base                    # one tensor, built in one launch
            batches.append((model.tta_head_outputs(data['img'], data['img_metas']), data['img_metas'][0]))
    assert len(batches) == 3

    def run(merge, batched):
        monkeypatch.setenv('GGA_MONO3D_DETECT_BATCHED', batched)
        results = []
        for outs, metas in batches:
            results += model._results(model.bbox_head.get_bboxes(*merge(outs, len(metas)), metas, rescale=True))
        return results

    # a threshold at which the random-weight model detects something in at least half of the frames
    for thr in (1e-3, 1e-5, 1e-8, 0.0):
        model.bbox_head.test_cfg['score_thr'] = thr
        reference = run(model.tta_merge_eager, '0')
        with_dets = sum(len(r['img_bbox']['scores_3d']) > 0 for r in reference)
        print(f'score_thr {thr}: {with_dets} of {len(reference)} frames with detections')
        if 2 * with_dets >= len(reference):
            break
    assert 2 * with_dets >= len(reference) == 6
    _same_results(run(F.mono3d_tta_merge, '1'), reference)
    # the test run itself, both switches in both positions through the environment
    runs = {}
    for merge, batched in (('1', '1'), ('0', '0')):
        monkeypatch.setenv('GGA_MONO3D_TTA_MERGE', merge)
        monkeypatch.setenv('GGA_MONO3D_DETECT_BATCHED', batched)
        calls = []
        real = F.mono3d_tta_merge
        monkeypatch.setattr(F, 'mono3d_tta_merge', lambda *a, **k: calls.append(1) or real(*a, **k))
        runs[merge] = single_gpu_test(model, loader, torch.device(DEV))
        monkeypatch.setattr(F, 'mono3d_tta_merge', real)
        assert len(calls) == (3 if merge == '1' else 0)
        assert len(runs[merge]) == 6 and all(set(r) == {'img_bbox', 'img_bbox2d'} for r in runs[merge])
    # --format-only on data.test with the TTA pipeline: six files per result name
    monkeypatch.setenv('GGA_MONO3D_TTA_MERGE', '1')
    monkeypatch.setenv('GGA_MONO3D_DETECT_BATCHED', '1')
    sub = str(tmp_path / 'submission_')
    outs_t, result = generate_pseudo_labels(copy.deepcopy(cfg), None, eval_metrics=None, eval_options=dict(submission_prefix=sub),
                                            device=DEV, model=model, format_only=True)
    assert result is None and len(outs_t) == 6
    for name in ('img_bbox', 'img_bbox2d'):
        assert sorted(os.listdir(sub + name)) == [f'{i:06d}.txt' for i in range(6)]
