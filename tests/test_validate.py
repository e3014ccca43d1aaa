"""The host-side pieces of in-training validation (``gga_amd.train.EvalHook``: schedule, rule, best-file bookkeeping, the keys
that reach ``evaluate``), ``tools/train.py --validate`` on a config without ``data.val``, and the float64 restatement the
device formatter is tested against (tests/test_kitti_format_gpu.py) on a box computed by hand."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from gga_amd.train import EVAL_HOOK_KEYS, EvalHook, evaluate_kwargs, infer_rule, should_evaluate
from test_kitti_format_gpu import format_ref64, left_out_shares, make_run, reference_run


def test_schedule_predicate():
    assert [e for e in range(1, 9) if should_evaluate(e)] == list(range(1, 9))
    assert [e for e in range(1, 9) if should_evaluate(e, interval=5)] == [5]
    assert [e for e in range(1, 11) if should_evaluate(e, interval=3)] == [3, 6, 9]
    assert [e for e in range(1, 9) if should_evaluate(e, interval=2, start=2)] == [2, 4, 6, 8]
    assert [e for e in range(1, 9) if should_evaluate(e, interval=2, start=3)] == [3, 5, 7]
    assert [e for e in range(1, 9) if should_evaluate(e, interval=3, start=0)] == [3, 6]
    assert [e for e in range(1, 5) if should_evaluate(e, interval=1, start=4)] == [4]


def test_rule_inference():
    assert infer_rule('KITTI/Overall_3D_AP11_moderate') == 'greater'
    assert infer_rule('pts_bbox/KITTI/Car_3D_AP40_easy_strict') == 'greater'
    assert infer_rule('mAP') == 'greater' and infer_rule('AR@100') == 'greater' and infer_rule('top1_acc') == 'greater'
    assert infer_rule('val_loss') == 'less'
    assert infer_rule('pseudo_labels/objects', 'less') == 'less' and infer_rule('val_loss', 'greater') == 'greater'
    with pytest.raises(ValueError):
        infer_rule('pseudo_labels/objects')
    with pytest.raises(ValueError):
        infer_rule('mAP', 'largest')
    with pytest.raises(ValueError):                    # at construction, not at the first evaluation
        EvalHook(None, save_best='pseudo_labels/objects')
    assert EvalHook(None, save_best='pseudo_labels/objects', rule='less').rule == 'less'
    assert EvalHook(None, save_best='auto').rule is None           # decided by the first key that comes back
    with pytest.raises(ValueError):
        EvalHook(None, interval=0)
    with pytest.raises(NotImplementedError):
        EvalHook(None, by_epoch=False)


class _Runner:
    def __init__(self):
        self.epoch, self.hook_msgs, self.saves = 0, {}, []

    def save_checkpoint(self, out_dir, filename_tmpl='epoch_{}.pth', create_symlink=True, **kw):
        self.saves.append((out_dir, filename_tmpl.format(self.epoch), create_symlink, dict(self.hook_msgs)))


def test_best_file_bookkeeping():
    removed = []
    hook = EvalHook(None, save_best='auto', out_dir='/w')
    hook._remove = removed.append
    r = _Runner()
    key = 'KITTI/Overall_3D_AP11_moderate'
    scores = [10.0, 30.0, 20.0, 30.0, 31.5]
    for e, s in enumerate(scores, 1):
        r.epoch = e
        assert hook.update_best(r, {key: s, 'KITTI/Overall_BEV_AP11_moderate': 99.0 - e}) == (e in (1, 2, 5))
    assert hook.save_best == key and hook.rule == 'greater'
    names = [f'best_KITTI_Overall_3D_AP11_moderate_epoch_{e}.pth' for e in (1, 2, 5)]
    assert [(d, n, link) for d, n, link, _ in r.saves] == [('/w', n, False) for n in names]
    # the file is written with the new best already in its meta
    assert [m for *_, m in r.saves] == [dict(best_score=s, best_ckpt=os.path.join('/w', n)) for s, n in zip((10.0, 30.0, 31.5), names)]
    assert removed == [os.path.join('/w', names[0]), os.path.join('/w', names[1])]
    assert r.hook_msgs == dict(best_score=31.5, best_ckpt=os.path.join('/w', names[2]))
    # 'less', continuing from a resumed best
    hook = EvalHook(None, save_best='val_loss', out_dir='/w')
    hook._remove = removed.append
    r = _Runner()
    r.hook_msgs = dict(best_score=0.5, best_ckpt='/old/best_val_loss_epoch_3.pth')
    r.epoch = 4
    assert not hook.update_best(r, dict(val_loss=0.7)) and not r.saves
    r.epoch = 5
    assert hook.update_best(r, dict(val_loss=0.4)) and removed[-1] == '/old/best_val_loss_epoch_3.pth'
    with pytest.raises(KeyError):
        hook.update_best(r, dict(other=1.0))
    with pytest.raises(ValueError):
        EvalHook(None, save_best='mAP').update_best(_Runner(), dict(mAP=1.0))          # nowhere to write to


def test_hook_keys_do_not_reach_evaluate():
    cfg = dict(interval=5, start=2, by_epoch=True, save_best='auto', rule='greater', tmpdir='/t', gpu_collect=True,
               pipeline=[dict(type='LoadPointsFromFile')], metric='mAP', pklfile_prefix='/p/x', device='cuda:1')
    assert evaluate_kwargs(cfg) == dict(metric='mAP', pklfile_prefix='/p/x', device='cuda:1')
    assert set(EVAL_HOOK_KEYS) == {'interval', 'start', 'by_epoch', 'save_best', 'rule', 'tmpdir', 'gpu_collect'}
    hook = EvalHook(None, **cfg)
    assert hook.eval_kwargs == dict(metric='mAP', pklfile_prefix='/p/x', device='cuda:1')
    assert (hook.interval, hook.start, hook.tmpdir, hook.gpu_collect) == (5, 2, '/t', True)
    assert evaluate_kwargs(None) == {}


def test_train_tool_refuses_validate_without_a_val_section(tmp_path):
    cfg = tmp_path / 'no_val.py'
    cfg.write_text("model = dict(type='X')\ndata = dict(samples_per_gpu=1, workers_per_gpu=0, train=dict(type='Y'))\n")
    run = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'train.py'), str(cfg), '--validate', '--work-dir', str(tmp_path / 'w')],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 2 and 'data.val' in run.stderr, (run.returncode, run.stderr[-800:])
    assert not os.path.exists(tmp_path / 'w')
    run = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'train.py'), str(cfg), '--validate', '--no-validate'],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 2 and 'exclude' in run.stderr


def test_float64_restatement_on_a_box_computed_by_hand():
    """Box (10, 0, -1), sizes (4, 2, 1.5), yaw 0; the camera looks along the LiDAR's x. Camera box: location (0, 1, 10), sizes
    (4, 1.5, 2), rotation_y -pi/2 - its corners are x = +-1, y in {-0.5, 1}, z in {8, 12}; with f = 700, c = (600, 180):
    u in 600 -+ 700/8, v from 180 - 350/8 to 180 + 700/8."""
    rt = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1.0]])
    p2 = np.array([[700, 0, 600, 0], [0, 700, 180, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    boxes = np.array([[10, 0, -1, 4, 2, 1.5, 0], [10, 0, -1, 4, 2, 1.5, 2 * np.pi], [10, 0, 0.5, 4, 2, 1.5, 0], [-10, 0, -1, 4, 2, 1.5, 0],
                      [10, 30, -1, 4, 2, 1.5, 0], [4, 0, -1, 4, 2, 1.5, np.pi / 2]])
    r = format_ref64(boxes, rt, p2, (375, 1242))
    assert r['valid'].tolist() == [True, True, False, False, False, True]
    np.testing.assert_allclose(r['location'][0], [0, 1, 10], atol=1e-12)
    np.testing.assert_allclose(r['dimensions'][0], [4, 1.5, 2])
    np.testing.assert_allclose(r['rotation_y'][:2], [-np.pi / 2] * 2, atol=1e-12)
    np.testing.assert_allclose(r['alpha'][0], -np.pi / 2, atol=1e-12)
    np.testing.assert_allclose(r['bbox'][0], [512.5, 136.25, 687.5, 267.5], atol=1e-9)
    np.testing.assert_allclose(r['bbox'][1], r['bbox'][0], atol=1e-9)
    np.testing.assert_allclose(r['yaw'][:2], [0, 0], atol=1e-12)
    assert r['min_depth'][0] == pytest.approx(8.0)
    # yaw pi/2: the long side across the view (x = +-2, z = 4 +- 1), rotation_y -pi -> +pi after limiting; the 2D box is clipped
    np.testing.assert_allclose(abs(r['rotation_y'][5]), np.pi, atol=1e-12)
    np.testing.assert_allclose(r['bbox_raw'][5], [600 - 1400 / 3, 180 - 350 / 3, 600 + 1400 / 3, 180 + 700 / 3], atol=1e-9)
    np.testing.assert_allclose(r['bbox'][5], [600 - 1400 / 3, 180 - 350 / 3, 600 + 1400 / 3, 375], atol=1e-9)
    assert r['near'].tolist() == [False] * 6


def test_generator_stays_within_the_cap_on_what_is_left_out():
    infos, outs = make_run()
    refs = reference_run(infos, outs)
    counts = [len(r['valid']) for r in refs]
    assert len(refs) == 200 and counts[0] == 0 and counts[2] > 64 and not refs[1]['valid'].any() and len(refs[1]['valid']) > 0
    near, shallow = left_out_shares(refs)
    assert near <= 0.05 and shallow <= 0.05, (near, shallow)
    n, valid = sum(counts), sum(int(r['valid'].sum()) for r in refs)
    assert 0.3 < valid / n < 0.8                        # both outcomes of the validity test are well represented
    assert sum(len(i['annos']['name']) for i in infos) > 1000
    for o in outs:                                      # scores identify a detection within its frame
        s = o['scores_3d'].numpy()
        assert len(set(s.tolist())) == len(s)
