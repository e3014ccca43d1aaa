"""KITTI AP evaluation, the checks that need no device: argument validation of the new entry points, the host side of
gga_amd/kitti_eval.py (clean_data flags, thresholds, text / dictionary assembly) against tests/golden/kitti_eval.npz - written by
the reference's own eval.py (tools_dev/make_golden.py::golden_kitti_eval) - and the opt-in switch of ``evaluate``."""
import inspect
import os

import numpy as np
import pytest

from conftest import GOLDEN
from gga_amd import _lib

import _kitti_eval_ref as K


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'kitti_eval.npz'))


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    L = _lib.lib()
    assert L.gga_kitti_eval_overlaps(None, None, 4, None, None, 4, 2, 1, 1, 0, None, None, 16, None) == -1
    assert b'null pointer' in L.gga_last_error()
    assert L.gga_kitti_eval_overlaps(None, None, 4, None, None, 4, 0, 1, 1, 0, None, None, 16, None) == -1
    assert b'bad sizes' in L.gga_last_error()
    assert L.gga_kitti_eval_overlaps(None, None, 4, None, None, 4, 2, 0, 1, 0, None, None, 16, None) == -1
    assert b'metric' in L.gga_last_error()
    stats = lambda n_frames, n_combos, metric: L.gga_kitti_eval_stats(
        None, 0, None, 8, None, None, None, None, 4, None, 2, None, 0, None, None, 1, None, None, n_combos, n_frames, 4, metric, 1, 1, 0,
        None, None, None, None, None, None, 0, None)
    assert stats(2, 3, 0) == -1 and b'null pointer' in L.gga_last_error()
    assert stats(0, 3, 0) == -1 and b'bad sizes' in L.gga_last_error()
    assert stats(2, 0, 0) == -1 and b'bad sizes' in L.gga_last_error()
    assert stats(2, 3, 5) == -1 and b'metric' in L.gga_last_error()
    assert L.gga_kitti_eval_stats_workspace_bytes(0, 1, 1) == 0
    assert L.gga_kitti_eval_stats_workspace_bytes(3769, 18, 40) > L.gga_kitti_eval_stats_workspace_bytes(40, 18, 40) > 0


def test_clean_data_flags_equal_the_goldens(golden):
    from gga_amd import kitti_eval as KE
    gts, dts = K.unpack_annos('B.gt', golden), K.unpack_annos('B.dt', golden)
    names = np.concatenate([g['name'] for g in gts])
    assert {'Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'DontCare'} <= set(names.tolist())
    for c in range(3):
        for l in range(3):
            got = KE._prepare_data(gts, dts, c, l)
            assert np.array_equal(got['ignored_gt'], golden[f'B.clean.{c}.{l}.ignored_gt'])
            assert np.array_equal(got['ignored_dt'], golden[f'B.clean.{c}.{l}.ignored_dt'])
            assert got['total_num_valid_gt'] == int(golden[f'B.clean.{c}.{l}.num_valid_gt'])
            assert np.array_equal(got['total_dc_num'], golden[f'B.clean.{c}.{l}.dc_num'])
    # the per-frame form of the reference's signature
    n, ig, idt, dc = KE.clean_data(gts[0], dts[0], 0, 1)
    n0 = len(gts[0]['name'])
    assert ig == golden['B.clean.0.1.ignored_gt'][:n0].tolist() and n == ig.count(0)
    assert idt == golden['B.clean.0.1.ignored_dt'][:len(dts[0]['name'])].tolist() and len(dc) == golden['B.clean.0.1.dc_num'][0]


def test_text_and_dictionary_assembly_reproduces_the_golden(golden):
    from gga_amd import kitti_eval as KE
    mAPs = tuple(golden[f'B.mAP{k}'] for k in ('11_bbox', '11_bev', '11_3d', '11_aos', '40_bbox', '40_bev', '40_3d', '40_aos'))
    text, ret = KE.format_kitti_results(mAPs, [0, 1, 2], KE.kitti_min_overlaps([0, 1, 2]), True)
    assert text == str(golden['B.result'])
    assert list(ret.keys()) == golden['B.ret_keys'].tolist()
    assert np.array_equal(np.array([ret[k] for k in ret]), golden['B.ret_values'])
    # mAP arithmetic on the golden precision arrays
    for metric, name in enumerate(('bbox', 'bev', '3d')):
        prec = golden[f'B.eval_class.{metric}.precision']
        assert np.array_equal(KE.get_mAP11(prec), golden[f'B.mAP11_{name}']) and np.array_equal(KE.get_mAP40(prec), golden[f'B.mAP40_{name}'])
    # without AOS and for one class: no aos lines, no Overall block
    text1, ret1 = KE.format_kitti_results(tuple(m[:1] if i % 4 != 3 else None for i, m in enumerate(mAPs)), [0], KE.kitti_min_overlaps([0]), False)
    assert 'aos' not in text1 and 'Overall' not in text1 and len(ret1) == 2 * 3 * 3 * 2


def get_thresholds_plain(scores, num_gt, num_sample_pts=41):
    """The scalar walk get_thresholds vectorises (KITTI's recall sampling rule), written out for the comparison."""
    scores = np.sort(scores)[::-1]
    current_recall, out = 0, []
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < len(scores) - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(scores) - 1:
            continue
        out.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return out


def test_get_thresholds_equals_the_scalar_walk():
    from gga_amd.kitti_eval import get_thresholds
    rng = np.random.default_rng(5)
    for n, num_gt in ((0, 5), (1, 1), (7, 9), (40, 41), (300, 310), (5000, 5200), (90, 400)):
        scores = np.round(rng.uniform(0, 1, n), 2).astype(np.float32)
        got, want = get_thresholds(scores.copy(), num_gt), get_thresholds_plain(scores.copy(), num_gt)
        assert len(got) == len(want) <= 41 and all(a == b for a, b in zip(got, want))


def test_case_a_fixture_and_the_references_own_error(golden):
    """Case A covers what it must, the degenerate pairs (identical boxes, a shared edge) stay within the 2 % that may be
    exempted from the float64 comparison, and the emulated reference's distance from float64 recorded by the generator is
    what the restatement here gives."""
    dc, gc = golden['A.dt_count'], golden['A.gt_count']
    assert ((dc == 0) & (gc == 0)).any() and ((dc == 0) & (gc > 0)).any() and ((dc > 0) & (gc == 0)).any()
    deg = golden['A.degenerate']
    assert 350 <= deg.size <= 450 and 0 < deg.mean() <= 0.02
    assert (np.abs(golden['A.dt'][:, 6]) > np.pi).any() or (np.abs(golden['A.gt'][:, 6]) > np.pi).any()
    do, go = np.concatenate([[0], np.cumsum(dc)]), np.concatenate([[0], np.cumsum(gc)])
    for metric, name in ((1, 'bev'), (2, '3d')):
        o64 = np.concatenate([K.rotated_overlaps64(golden['A.dt'][do[f]:do[f + 1]], golden['A.gt'][go[f]:go[f + 1]], metric).reshape(-1)
                              for f in range(len(dc))])
        ref = golden[f'A.{name}'].astype(np.float64)
        assert np.abs(ref - o64)[~deg].max() <= float(golden['A.ref_err'])
        assert (o64 == 0).sum() > 20 and ((o64 > 0.05) & (o64 < 0.95)).sum() > 40
    assert (golden['A.bev'] > 0).sum() > (golden['A.3d'] > 0).sum()          # height-disjoint pairs
    assert float(golden['A.ref_err']) < 5e-6


def test_evaluate_has_the_opt_in_switch():
    from gga_amd.datasets import KittiDataset_GGA_match
    assert inspect.signature(KittiDataset_GGA_match.evaluate).parameters['kitti_ap'].default is False
