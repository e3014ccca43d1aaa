"""The float64 references of tests/_geometry_ref.py, proven on the CPU before any kernel is compared with them: closed forms,
the C oracle (a different algorithm: half-plane clipping) and the reference's known answers."""
import numpy as np
import pytest

import _geometry_ref as G
from oracle import oracle as O
from test_oracle import KA_ALL, KA_BOXES, KA_DEPTH_BOXES, KA_DEPTH_PART, KA_DEPTH_PTS, KA_PART, KA_PTS

R2 = np.sqrt(2.0)


def _iou(b1, b2, mode='iou'):
    return float(G.rect_iou64(np.array([b1]), np.array([b2]), mode, aligned=True)[0])


def test_rect_iou64_axis_aligned_closed_forms():
    g = np.random.default_rng(0)
    n = 200
    c1, c2 = g.integers(-20, 20, (n, 2)) / 8.0, g.integers(-20, 20, (n, 2)) / 8.0
    s1, s2 = g.integers(1, 48, (n, 2)) / 8.0, g.integers(1, 48, (n, 2)) / 8.0
    b1 = np.concatenate([c1, s1, np.zeros((n, 1))], 1)
    b2 = np.concatenate([c2, s2, np.zeros((n, 1))], 1)
    ov = np.clip(np.minimum(c1 + s1 / 2, c2 + s2 / 2) - np.maximum(c1 - s1 / 2, c2 - s2 / 2), 0, None).prod(1)
    a1, a2 = s1.prod(1), s2.prod(1)
    assert (ov > 0).sum() > 50 and (ov == 0).sum() > 20
    np.testing.assert_allclose(G.rect_iou64(b1, b2, aligned=True), ov / (a1 + a2 - ov), rtol=0, atol=1e-12)
    np.testing.assert_allclose(G.rect_iou64(b1, b2, 'iof', aligned=True), ov / a1, rtol=0, atol=1e-12)
    # the same rectangles given as (h, w, angle + pi/2) and as angle + pi: the float32 angle is 4e-8 off, hence 1e-6
    b1r = np.concatenate([c1, s1[:, ::-1], np.full((n, 1), np.pi / 2)], 1)
    b2r = np.concatenate([c2, s2, np.full((n, 1), np.pi)], 1)
    np.testing.assert_allclose(G.rect_iou64(b1r, b2r, aligned=True), ov / (a1 + a2 - ov), rtol=0, atol=1e-6)
    # pairwise form = aligned form of every pair
    pw = G.rect_iou64(b1[:7], b2[:9])
    assert pw.shape == (7, 9)
    for i in range(7):
        np.testing.assert_array_equal(pw[i], G.rect_iou64(np.repeat(b1[i:i + 1], 9, 0), b2[:9], aligned=True))


@pytest.mark.parametrize('a', [0.5, 1.0, 3.0, 0.001, 64.0])
def test_rect_iou64_equal_squares_at_45_degrees(a):
    inter = 2 * (R2 - 1) * a * a                                  # a regular octagon
    for base in (0.0, 0.3, -2.0):
        got = _iou([1.0, -2.0, a, a, base], [1.0, -2.0, a, a, base + np.pi / 4])
        assert abs(got - inter / (2 * a * a - inter)) < 1e-6      # float32 angles: pi/4 is 2e-8 off
        got = _iou([1.0, -2.0, a, a, base], [1.0, -2.0, a, a, base + np.pi / 4], 'iof')
        assert abs(got - 2 * (R2 - 1)) < 1e-6


def test_rect_iou64_nested_touching_and_degenerate():
    for ang_out, ang_in in ((0.0, 0.0), (0.0, 0.7), (1.1, -0.4), (20.3, 3.0)):
        outer, inner = [3.0, 4.0, 8.0, 8.0, ang_out], [3.25, 3.5, 2.0, 1.0, ang_in]
        assert abs(_iou(inner, outer) - 2.0 / 64.0) < 1e-12 and abs(_iou(outer, inner) - 2.0 / 64.0) < 1e-12
        assert abs(_iou(inner, outer, 'iof') - 1.0) < 1e-12 and abs(_iou(outer, inner, 'iof') - 2.0 / 64.0) < 1e-12
    sq = [0.0, 0.0, 2.0, 2.0, 0.0]
    assert _iou(sq, [2.0, 0.0, 2.0, 2.0, 0.0]) == 0.0             # shared edge
    assert _iou(sq, [2.0, 0.5, 2.0, 1.0, 0.0]) == 0.0             # shared part of an edge
    assert _iou(sq, [2.0, 2.0, 2.0, 2.0, 0.0]) == 0.0             # touching corner
    assert _iou(sq, [1.0 + R2, 0.0, 2.0, 2.0, np.pi / 4]) < 1e-7  # a corner touching an edge
    assert _iou(sq, [np.nextafter(np.float32(2), np.float32(3)), 0.0, 2.0, 2.0, 0.0]) == 0.0      # a gap of one ulp
    assert _iou(sq, [5.0, 0.0, 2.0, 2.0, 0.3]) == 0.0
    assert _iou(sq, sq) == 1.0 and abs(_iou([5, 5, 3, 1, 0.7], [5, 5, 3, 1, 0.7]) - 1.0) < 1e-12
    for dead in ([0.0, 0.0, 0.0, 2.0, 0.0], [0.0, 0.0, 1e-8, 1e-8, 0.3], [0.0, 0.0, 2.0, 0.0, 0.0]):
        for mode in ('iou', 'iof'):
            assert _iou(sq, dead, mode) == 0.0 and _iou(dead, sq, mode) == 0.0 and _iou(dead, dead, mode) == 0.0
    assert G.rect_iou64(np.zeros((0, 5)), np.zeros((3, 5))).shape == (0, 3)


def _random_pairs(n, seed):
    g = np.random.default_rng(seed)
    mk = lambda: np.stack([g.uniform(-4, 4, n), g.uniform(-4, 4, n), g.uniform(0.5, 6, n), g.uniform(0.5, 6, n),
                           g.uniform(-4, 4, n)], 1).astype(np.float32)
    return mk(), mk()


def test_rect_iou64_equals_the_oracle_on_random_pairs():
    b1, b2 = _random_pairs(25, 11)
    for mode in ('iou', 'iof'):
        ref = G.rect_iou64(b1, b2, mode)                         # 625 pairs
        want = O.box_iou_rotated(b1, b2, mode)                   # float64 clip, rounded to float32
        assert (want > 0.05).sum() > 100
        np.testing.assert_allclose(ref, want, rtol=2e-7, atol=1e-7)
    # far from the origin (float32 centres) and thin boxes
    b1[:, :2] += 600
    b2[:, :2] += 600
    b2[:, 2] = 1e-3
    np.testing.assert_allclose(G.rect_iou64(b1, b2), O.box_iou_rotated(b1, b2), rtol=2e-7, atol=1e-7)


def test_clip32_restatement_is_the_clip():
    """The float32 restatement of the kernel's algorithm agrees with float64 on ordinary pairs to float32 accuracy."""
    b1, b2 = _random_pairs(300, 5)
    for mode in ('iou', 'iof'):
        np.testing.assert_allclose(G.rect_iou_clip32(b1, b2, mode), G.rect_iou64(b1, b2, mode, aligned=True), rtol=1e-4, atol=2e-5)


def test_pts_in_boxes64_known_answers():
    assert G.pts_in_boxes64(KA_PTS, KA_BOXES, all_boxes=True).tolist() == KA_ALL
    assert G.pts_in_boxes64(KA_PTS, KA_BOXES).tolist() == KA_PART
    assert G.pts_in_boxes64(KA_DEPTH_PTS, KA_DEPTH_BOXES).tolist() == KA_DEPTH_PART
    # batched form, empty sides
    assert G.pts_in_boxes64(KA_PTS[None], KA_BOXES[None]).tolist() == [KA_PART]
    assert G.pts_in_boxes64(KA_PTS, np.zeros((0, 7))).tolist() == [-1] * len(KA_PTS)
    assert G.pts_in_boxes64(KA_PTS, np.zeros((0, 7)), True).shape == (len(KA_PTS), 0)
    assert G.pts_in_boxes64(np.zeros((0, 3)), KA_BOXES, True).shape == (0, 4)


def test_pts_in_boxes64_faces_and_nan():
    box = np.array([[2.0, -4.0, 1.0, 4.0, 2.0, 0.5, 0.0]])
    inside = [[2, -4, 1.5], [2, -4, 1.0], [0.125, -4, 1.25], [3.875, -3.125, 1.0]]
    outside = [[0, -4, 1.25], [4, -4, 1.25], [2, -5, 1.25], [2, -3, 1.25], [2, -4, 1.625], [2, -4, 0.875]]
    assert G.pts_in_boxes64(np.array(inside + outside), box).tolist() == [0] * 4 + [-1] * 6
    nan = np.nan
    assert G.pts_in_boxes64(np.array([[nan, -4, 1.25], [2, nan, 1.25], [2, -4, nan]]), box).tolist() == [-1] * 3
    for k in range(7):
        b = box.copy()
        b[0, k] = nan
        assert G.pts_in_boxes64(np.array([[2.0, -4.0, 1.25]]), b, True).tolist() == [[0]]
    d = G.pts_face_distance64(np.array([[2.0, -4.0, 1.25], [0.25, -4, 1.25]]), box)
    np.testing.assert_allclose(d[:, 0], [0.25, 0.25])


@pytest.mark.parametrize('n,seed', [(1, 0), (7, 1), (300, 2), (600, 3)])
def test_nms_groups_equal_the_oracle(n, seed):
    thr = 0.5
    boxes, scores, keep, margin, group = G.nms_groups(n, thr, seed=seed)
    assert boxes.shape == (n, 5) and boxes.dtype == np.float32 and len(np.unique(scores)) == n
    assert margin >= 0.1
    assert np.array_equal(keep, O.nms_rotated(boxes, scores, thr))
    assert np.all(np.diff(scores[keep]) < 0)
    if n >= 300:
        # closed form of the generator: copies shifted by d * w along the box's own axis have IoU (1 - d) / (1 + d) ...
        k = 1 + len(G.FRACTIONS)
        fr = np.concatenate([[0.0], G.FRACTIONS])
        iou = G.rect_iou64(boxes[:k], boxes[:k])
        d = np.abs(fr[:, None] - fr[None])
        np.testing.assert_allclose(iou, (1 - d) / (1 + d), atol=1e-5)
        # ... boxes of different groups are disjoint, and the greedy pass depends on the order inside a group
        full = G.rect_iou64(boxes, boxes)
        assert np.all(full[group[:, None] != group[None]] == 0.0)
        per_group = np.bincount(group[keep])
        assert per_group.min() >= 1 and len(np.unique(per_group[:n // k])) >= 2


@pytest.mark.parametrize('n', [1, 9, 500])
def test_circle_groups_equal_the_oracle(n):
    dets, keep, margin = G.circle_groups(n, 6.25, seed=n)
    assert margin >= 2.0
    assert O.circle_nms(dets, 6.25, None) == keep.tolist()
    assert O.circle_nms(dets, 6.25, 7) == keep[:7].tolist()
