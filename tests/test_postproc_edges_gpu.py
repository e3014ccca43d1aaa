"""Edge and scale tests of the post-processing geometry kernels (csrc/rotated_iou.h, csrc/postproc.hip) through
``gga_amd.ops``, against the float64 references of tests/_geometry_ref.py (proven on the CPU by tests/test_geometry_ref.py):
the pair classes a float32 half-plane clip gets wrong, the NMS scan beyond its first register word, tied scores, the label
offset, the points-in-boxes kernel beyond one tile of boxes and on the faces themselves."""
import numpy as np
import pytest
import torch

import _geometry_ref as G
from gga_amd import ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)          # (a copy: cached inputs stay untouched)
PI = np.pi

# ----------------------------------------------------------------------------------------------- rotated IoU
RTOL, ATOL = 1e-4, 2e-5                 # the bar of test_postproc_gpu.test_box_iou_rotated_vs_oracle
LOWEST_NMS_THR = 0.05                   # configs/gga/gga_pdg.py; the others use 0.2 and 0.5
SHIFTS = [(0.0, 0.0), (70.0, -40.0), (600.0, 600.0)]
ANGLES = [0.0, PI / 2, -PI / 2, PI, 1e-3, 0.7, 20.3]
SIZES = [(2.0, 2.0), (4.0, 1.5), (0.5, 6.0), (3.875, 1.625)]


def _f32(rows, shift):
    b = np.asarray(rows, np.float64).reshape(-1, 5).copy()
    b[:, 0] += shift[0]
    b[:, 1] += shift[1]
    return b.astype(np.float32)


def _identical(shift):
    rows = [(cx, cy, w, h, a) for a in ANGLES for (w, h) in SIZES for (cx, cy) in ((0.0, 0.0), (1.3, -2.7))]
    b = _f32(rows, shift)
    return b, b.copy(), np.ones(len(b))


def _reparametrised(shift):
    r1, r2 = [], []
    for a in ANGLES:
        for (w, h) in SIZES:
            r1 += [(1.25, -0.5, w, h, a)] * 3
            r2 += [(1.25, -0.5, w, h, a + PI), (1.25, -0.5, h, w, a + PI / 2), (1.25, -0.5, h, w, a - PI / 2)]
    return _f32(r1, shift), _f32(r2, shift), None              # 1 up to the float32 rounding of the angle: rect_iou64


def _near_parallel(shift):
    r1, r2 = [], []
    for a in (0.0, 0.7, -2.1):
        for (w, h) in SIZES[:3]:
            for da in (1e-6, 1e-4, 1e-2):
                for (sx, sy) in ((0.0, 0.0), (0.01, -0.02), (0.3, 0.1)):
                    r1.append((0.5, 0.25, w, h, a))
                    r2.append((0.5 + sx, 0.25 + sy, w, h, a + da))
    return _f32(r1, shift), _f32(r2, shift), None


def _axis_and_nested(shift):
    """Dyadic coordinates (multiples of 1/8): every translation used here is exact in float32, so the closed forms hold."""
    r1, r2, want = [], [], []
    g = np.random.default_rng(12)
    for _ in range(24):                                         # axis-aligned overlaps, angle 0 / pi/2 with w and h swapped
        c1, c2 = g.integers(-12, 12, 2) / 8.0, g.integers(-12, 12, 2) / 8.0
        s1, s2 = g.integers(8, 40, 2) / 8.0, g.integers(8, 40, 2) / 8.0
        ov = np.clip(np.minimum(c1 + s1 / 2, c2 + s2 / 2) - np.maximum(c1 - s1 / 2, c2 - s2 / 2), 0, None).prod()
        r1.append((c1[0], c1[1], s1[0], s1[1], 0.0))
        r2.append((c2[0], c2[1], s2[0], s2[1], 0.0))
        want.append(ov / (s1.prod() + s2.prod() - ov))
    for a_out, a_in in ((0.0, 0.0), (0.0, 0.7), (1.1, -0.4), (20.3, 3.0), (PI / 2, PI)):     # nested: the ratio of the areas
        r1.append((3.0, 4.0, 8.0, 8.0, a_out))
        r2.append((3.25, 3.5, 2.0, 1.0, a_in))
        want.append(2.0 / 64.0)
        r1.append((3.25, 3.5, 2.0, 1.0, a_in))
        r2.append((3.0, 4.0, 8.0, 8.0, a_out))
        want.append(2.0 / 64.0)
    for a in (0.5, 1.0, 3.0, 64.0):                             # equal squares at 45 degrees: a regular octagon
        for base in (0.0, 0.3):
            r1.append((1.0, -2.0, a, a, base))
            r2.append((1.0, -2.0, a, a, base + PI / 4))
            want.append(2 * (np.sqrt(2) - 1) / (2 - 2 * (np.sqrt(2) - 1)))
    return _f32(r1, shift), _f32(r2, shift), np.asarray(want)


def _touching(shift):
    """Angles 0 / +-pi/2 / pi with dyadic sizes and centres touch exactly in float32 at every translation used here
    (expected 0); at other angles the rounded centres leave a sliver or a gap, which rect_iou64 measures."""
    r1, r2, want = [], [], []
    for (w, h) in SIZES:
        for a in (0.0, PI / 2, PI, -PI / 2, 0.7, -2.1):
            ux, uy, vx, vy = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
            r1 += [(0.5, 0.25, w, h, a)] * 3
            r2 += [(0.5 + w * ux, 0.25 + w * uy, w, h, a),                                 # shared edge
                   (0.5 + w * ux + 0.25 * h * vx, 0.25 + w * uy + 0.25 * h * vy, w, h / 2, a),   # part of an edge
                   (0.5 + w * ux + h * vx, 0.25 + w * uy + h * vy, w, h, a)]               # touching corner
            want += [0.0 if a not in (0.7, -2.1) else np.nan] * 3
    b1, b2 = _f32(r1, shift), _f32(r2, shift)
    gap1, gap2 = [], []
    for (w, h) in SIZES:                                        # a gap of one float32 ulp between axis-aligned boxes
        a = _f32([(0.5, 0.25, w, h, 0.0)], shift)[0]
        b = a.copy()
        b[0] = np.nextafter(np.float32(a[0] + np.float32(w)), np.float32(np.inf))
        assert float(b[0]) - float(a[0]) > w
        gap1.append(a)
        gap2.append(b)
        want.append(0.0)
    return np.concatenate([b1, np.stack(gap1)]), np.concatenate([b2, np.stack(gap2)]), np.asarray(want)


def _thin(shift):
    """The one family where float32 itself misses the bar: the clip works in the world frame, where the side tests and the
    shoelace sum of a 1 mm x 10 m box at an oblique angle cancel to about 1e-3 of the overlap. Measured on an MI355X: worst
    |err| 7.2e-4 (iou) / 6.5e-4 (iof), the float32 restatement on the CPU 7.2e-4 / 5.9e-4, so the bound is 4 x that (_check).
    Every other family stays under 1.3e-6."""
    r1, r2 = [], []
    for (w, h) in ((1e-3, 10.0), (10.0, 1e-3), (5e-4, 5.0)):    # aspect 1 : 1e4
        for a in (0.0, 0.7, PI / 2, -2.1):
            base = (0.5, 0.25, w, h, a)
            r1 += [base] * 6
            r2 += [base,                                        # itself
                   (0.5 + 0.25 * w * np.cos(a), 0.25 + 0.25 * w * np.sin(a), w, h, a),     # a quarter of its width aside
                   (0.5 - 0.25 * h * np.sin(a), 0.25 + 0.25 * h * np.cos(a), w, h, a),     # a quarter of its length along
                   (0.5, 0.25, w, h, a + 0.4),                  # crossing itself
                   (0.5, 0.25, h, w, a + 0.4),
                   (0.6, 0.2, 3.0, 2.0, a + 0.2)]               # crossing an ordinary box
    return _f32(r1, shift), _f32(r2, shift), None


def _degenerate(shift):
    live = [(0.5, 0.25, 2.0, 2.0, 0.0), (0.5, 0.25, 4.0, 1.5, 0.7)]
    dead = [(0.5, 0.25, 0.0, 2.0, 0.0), (0.5, 0.25, 2.0, 0.0, 0.3), (0.5, 0.25, 0.0, 0.0, 0.0), (0.5, 0.25, 1e-8, 1e-8, 0.3),
            (0.6, 0.25, 1e-10, 1e-5, 1.0), (0.5, 0.25, 1e-20, 1e3, 0.0)]
    r1 = [d for d in dead for _ in range(len(live) + len(dead))] + [x for x in live for _ in dead]
    r2 = (live + dead) * len(dead) + dead * len(live)
    return _f32(r1, shift), _f32(r2, shift), np.zeros(len(r1))


def _large_yaw(shift):
    g = np.random.default_rng(13)
    n, top = 48, 6 * PI + 1
    mk = lambda: np.stack([g.uniform(-1.5, 1.5, n), g.uniform(-1.5, 1.5, n), g.uniform(0.5, 6, n), g.uniform(0.5, 6, n),
                           g.uniform(-top, top, n)], 1)
    r1, r2 = mk(), mk()
    r1[:4, 4] = [top, -top, top, 6 * PI]
    r2[:4, 4] = [-top, top, top - 2 * PI, -6 * PI]
    return _f32(r1, shift), _f32(r2, shift), None


FAMILIES = dict(identical=_identical, reparametrised=_reparametrised, near_parallel=_near_parallel,
                axis_and_nested=_axis_and_nested, touching=_touching, thin=_thin, degenerate=_degenerate, large_yaw=_large_yaw)


def _check(what, got, ref, b1, b2, mode):
    """The bar of this op, |err| <= ATOL + RTOL * |ref| against float64. It is raised for a family only where float32
    arithmetic alone already misses it: when the kernel's algorithm evaluated step for step in numpy float32 on the CPU
    (G.rect_iou_clip32) is outside the bar on some pair of the family, the bound becomes four times that restatement's own
    worst error (the factor covers cosf / sinf and FMA contraction differing between host and device). Nothing here is
    taken from the kernel's output. -> (worst error, worst error of the float32 restatement or 0 where the bar stands)"""
    bound = ATOL + RTOL * np.abs(ref)
    err, e32 = np.abs(got - ref), 0.0
    if not (err <= bound).all():
        off = np.abs(G.rect_iou_clip32(b1, b2, mode) - ref)
        if not (off <= bound).all():
            e32 = float(off.max())
            bound = np.maximum(bound, 4.0 * e32)
    k = int(np.argmax(err - bound))
    assert (err <= bound).all(), (what, mode, b1[k].tolist(), b2[k].tolist(), got[k], ref[k], e32)
    return float(err.max()), e32


@pytest.mark.parametrize('shift', SHIFTS, ids=lambda s: f'at{int(s[0])}_{int(s[1])}')
@pytest.mark.parametrize('family', list(FAMILIES))
def test_box_iou_rotated_family(family, shift):
    b1, b2, closed = FAMILIES[family](shift)
    n = len(b1)
    assert n == len(b2) >= 20
    ii, jj = np.divmod(np.arange(n * n), n)
    known = ~np.isnan(closed) if closed is not None else np.zeros(n, bool)         # pairs with a closed-form answer
    for mode in ('iou', 'iof'):
        ref = G.rect_iou64(b1, b2, mode, aligned=True)
        pw_ref = G.rect_iou64(b1, b2, mode)
        got = ops.box_iou_rotated(_dev(b1), _dev(b2), mode=mode, aligned=True).cpu().numpy().astype(np.float64)
        pw = ops.box_iou_rotated(_dev(b1), _dev(b2), mode=mode).cpu().numpy().astype(np.float64)
        assert got.shape == (n,) and pw.shape == (n, n) and np.isfinite(got).all() and np.isfinite(pw).all()
        assert np.abs(np.diagonal(pw) - got).max() <= 1e-6       # the pairwise form computes what the aligned form does
        if closed is not None and mode == 'iou':                # the reference itself against the closed form
            np.testing.assert_allclose(ref[known], closed[known], rtol=0, atol=1e-6)
        err, e32 = _check((family, shift, 'aligned'), got, ref, b1, b2, mode)
        pw_err, pw_e32 = _check((family, shift, 'pairwise'), pw.reshape(-1), pw_ref.reshape(-1), b1[ii], b2[jj], mode)
        raised = max(e32, pw_e32)
        print(f'box_iou_rotated {family:>16} at {shift}: {mode} worst |err| aligned {err:.2e} pairwise {pw_err:.2e} '
              f'(bar {ATOL:g} + {RTOL:g}|ref|' + (f'; float32 restatement off by {raised:.2e}, bound 4x that' if raised else '') + ')')
        if family == 'identical':
            assert np.all(np.abs(got - 1.0) <= ATOL + RTOL)
        if family == 'reparametrised':
            assert np.all(np.abs(ref - 1.0) < 5e-5)
        if family == 'touching':
            # boxes that only touch must not suppress each other under any threshold the configs use
            assert np.all(got[known] <= ATOL) and np.all(got < LOWEST_NMS_THR / 100)
        if family == 'degenerate':
            a1 = (b1[:, 2] * b1[:, 3])[:, None]
            a2 = (b2[:, 2] * b2[:, 3])[None]
            dead = (a1 < 5e-15) | (a2 < 5e-15)                  # under the kernel's 1e-14 cut
            assert np.all(got == 0.0) and np.all(pw[dead] == 0.0) and dead.sum() > pw.size // 2


# ----------------------------------------------------------------------------------------------- NMS at scale
THR = 0.5
SCALE_N = [4097, 4160, 8191, 12289]     # the scan's register word ("slot") of the last box: 1, 1, 1, 3


def _groups(n):
    for seed in range(n, n + 64):       # a case whose lowest-scored box survives, so a cut can fall on the last position
        boxes, scores, keep, margin, _ = G.nms_groups(n, THR, seed=seed)
        if np.argmin(scores) == keep[-1]:
            return boxes, scores, keep, margin
    raise AssertionError('no such case')


def _sorted_position(scores):
    pos = np.empty(len(scores), np.int64)
    pos[np.argsort(-scores, kind='stable')] = np.arange(len(scores))
    return pos


def _cuts(want, scores):
    """max_keep values whose last kept box lies in slot 0 and in a slot >= 1 of the scan (4096 sorted positions per slot)."""
    kpos = _sorted_position(scores)[want]
    k0 = int((kpos < 4096).sum())
    deep = k0 + max(1, (len(want) - k0) // 2)
    assert 100 < k0 and deep <= len(want) and kpos[99] < 4096 <= kpos[deep - 1]
    return 100, deep


@pytest.mark.parametrize('n', SCALE_N)
def test_nms_rotated_beyond_one_slot(n):
    boxes, scores, want, margin = _groups(n)
    assert margin >= 0.1 and (n - 1) >> 12 == {4097: 1, 4160: 1, 8191: 1, 12289: 3}[n]
    dets, keep = ops.nms_rotated(_dev(boxes), _dev(scores), THR)
    assert keep.cpu().tolist() == want.tolist()
    assert torch.equal(dets[:, 5].cpu(), torch.from_numpy(scores[want])) and torch.equal(dets[:, :5].cpu(), torch.from_numpy(boxes[want]))
    for cut in _cuts(want, scores):
        dets, keep = ops.nms_rotated(_dev(boxes), _dev(scores), THR, max_keep=cut)
        assert keep.cpu().tolist() == want[:cut].tolist(), cut
        assert torch.equal(dets[:, 5].cpu(), torch.from_numpy(scores[want[:cut]]))


def _circles(n):
    for seed in range(n, n + 64):
        dets, keep, margin = G.circle_groups(n, 6.25, seed=seed)
        if np.argmin(dets[:, 2]) == keep[-1]:
            return dets, keep, margin
    raise AssertionError('no such case')


@pytest.mark.parametrize('n', SCALE_N)
def test_circle_nms_beyond_one_slot(n):
    dets, want, margin = _circles(n)
    assert margin >= 2.0                                        # squared distances are integers, the threshold is 6.25
    assert ops.circle_nms(_dev(dets), 6.25, post_max_size=None).cpu().tolist() == want.tolist()
    for cut in _cuts(want, dets[:, 2]) + (83,):
        assert ops.circle_nms(_dev(dets), 6.25, post_max_size=cut).cpu().tolist() == want[:cut].tolist(), cut


def test_nms_over_the_size_limit_raises_and_launches_nothing():
    n = 32769
    boxes = torch.zeros(n, 5, device=DEV)
    boxes[:, 2:4] = 1.0
    scores = torch.arange(n, device=DEV, dtype=torch.float32)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='32768'):
        ops.nms_rotated(boxes, scores, THR)
    with pytest.raises(RuntimeError, match='32768'):
        ops.circle_nms(torch.cat([boxes[:, :2], scores[:, None]], 1), 1.0)
    torch.cuda.synchronize()                                    # no kernel was queued, none can have faulted
    small, sc, want, _, _ = G.nms_groups(7, THR, seed=1)
    assert ops.nms_rotated(_dev(small), _dev(sc), THR)[1].cpu().tolist() == want.tolist()


# ----------------------------------------------------------------------------------------------- ties and labels
def _tied_case():
    boxes, _, _, margin, _ = G.nms_groups(600, THR, seed=21)
    assert margin >= 0.1
    g = np.random.default_rng(22)
    boxes = np.concatenate([boxes, boxes[:120]])                 # duplicated detections
    scores = (g.integers(1, 9, len(boxes)) / 8.0).astype(np.float32)        # 8 blocks of equal scores
    scores[600:] = scores[:120]
    return boxes, scores


def test_nms_rotated_tied_scores_keep_input_order():
    boxes, scores = _tied_case()
    assert len(np.unique(scores)) == 8
    want = O.nms_rotated(boxes, scores, THR)                     # stable order: ties in input order
    assert not set(want.tolist()) & set(range(600, 720))         # of two equal detections the first one stays
    first = ops.nms_rotated(_dev(boxes), _dev(scores), THR)
    again = ops.nms_rotated(_dev(boxes), _dev(scores), THR)
    assert first[1].cpu().tolist() == want.tolist()
    assert torch.equal(first[1], again[1]) and torch.equal(first[0], again[0])
    cut = ops.nms_rotated(_dev(boxes), _dev(scores), THR, max_keep=50)[1]
    assert cut.cpu().tolist() == want[:50].tolist()


@pytest.mark.parametrize('pre,post', [(None, None), (400, 50), (333, None)])
def test_nms_bev_tied_scores_keep_input_order(pre, post):
    boxes, scores = _tied_case()
    xyxyr = ops.xywhr2xyxyr(torch.from_numpy(boxes)).numpy()
    want = O.nms_bev(xyxyr, scores, THR, pre, post)
    first = ops.nms_bev(_dev(xyxyr), _dev(scores), THR, pre_max_size=pre, post_max_size=post)
    again = ops.nms_bev(_dev(xyxyr), _dev(scores), THR, pre_max_size=pre, post_max_size=post)
    assert first.cpu().tolist() == want.tolist() and torch.equal(first, again)
    if pre is not None:                                          # the cut falls inside a block of equal scores
        order = np.argsort(-scores, kind='stable')
        assert scores[order[pre - 1]] == scores[order[pre]]


def _small_tied_case(n, blocks):
    """n <= 32 boxes in ``blocks`` blocks of equal scores, interleaved (box i has score block i % blocks), so a sort that
    is not stable has something to permute. A quarter of the boxes are exact duplicates of earlier ones, the rest are
    chains in which neighbours suppress each other and next-but-one members do not: the order of equal scores decides
    the kept set. This is the size per-class NMS after a score threshold works at (box3d_multiclass_nms -> nms_bev), and
    the size at which torch's plain device sort takes an in-register bitonic network, which is not stable."""
    base = G.nms_groups(n - n // 4, THR, seed=100 + n)
    assert base[3] >= 0.1
    boxes = np.concatenate([base[0], base[0][:n // 4]])
    scores = (1.0 - (np.arange(n) % blocks) / 8.0).astype(np.float32)
    return boxes, scores


SMALL_TIES = [(n, blocks) for n in (8, 16, 24, 31, 32) for blocks in (1, 2, 3)]


@pytest.mark.parametrize('n,blocks', SMALL_TIES)
def test_nms_rotated_small_tied_inputs_keep_input_order(n, blocks):
    boxes, scores = _small_tied_case(n, blocks)
    want = O.nms_rotated(boxes, scores, THR)
    assert 2 <= len(want) < n - n // 4                           # something is suppressed, not by duplication alone
    for _ in range(2):
        dets, keep = ops.nms_rotated(_dev(boxes), _dev(scores), THR)
        assert keep.cpu().tolist() == want.tolist()
        assert torch.equal(dets[:, :5].cpu(), torch.from_numpy(boxes[want]))


@pytest.mark.parametrize('n,blocks', SMALL_TIES)
def test_nms_bev_small_tied_inputs_keep_input_order(n, blocks):
    boxes, scores = _small_tied_case(n, blocks)
    xyxyr = ops.xywhr2xyxyr(torch.from_numpy(boxes)).numpy()
    for pre, post in ((None, None), (n - 3, 4)):
        want = O.nms_bev(xyxyr, scores, THR, pre, post)
        for _ in range(2):
            got = ops.nms_bev(_dev(xyxyr), _dev(scores), THR, pre_max_size=pre, post_max_size=post)
            assert got.cpu().tolist() == want.tolist(), (pre, post)


def test_nms_rotated_labels_equal_per_label_calls():
    """Three labels whose boxes sit at identical places, centres out to 70 m: the label offset must separate the labels
    completely and must not disturb a single decision within one (the generator's margin is 0.1)."""
    boxes, _, _, margin, _ = G.nms_groups(720, THR, seed=31)
    assert margin >= 0.1 and 60 < np.abs(boxes[:, :2]).max() < 71
    n = len(boxes)
    g = np.random.default_rng(32)
    dets = np.tile(boxes, (3, 1))
    labels = np.repeat(np.arange(3), n)
    scores = ((g.permutation(3 * n) + 1) / (3.0 * n)).astype(np.float32)
    got = ops.nms_rotated(_dev(dets), _dev(scores), THR, labels=_dev(labels))[1].cpu().numpy()
    parts = []
    for l in range(3):
        idx = np.flatnonzero(labels == l)
        k = ops.nms_rotated(_dev(dets[idx]), _dev(scores[idx]), THR)[1].cpu().numpy()
        assert np.array_equal(k, O.nms_rotated(dets[idx], scores[idx], THR))
        parts.append(idx[k])
    union = np.concatenate(parts)
    union = union[np.argsort(-scores[union], kind='stable')]
    assert np.array_equal(got, union)
    assert len({tuple(np.sort(p % n)) for p in parts}) == 3      # the labels' survivors differ: no label decided for another


# ----------------------------------------------------------------------------------------------- points in boxes
FACE_MARGIN = 1e-4


def _scene(B, M, Tn):
    """Random boxes and points; no point within FACE_MARGIN of a face plane of any box of its frame (float64), so float32
    rounding (1e-6 at these coordinates) cannot decide anything. Points too close are drawn again, none is dropped. Half the
    points are drawn around box centres, and the first point of each frame sits in the frame's LAST box."""
    g = np.random.default_rng(B * 1000003 + M * 1009 + Tn)
    boxes = np.concatenate([g.uniform(-10, 10, (B, Tn, 2)), g.uniform(-3, 1, (B, Tn, 1)), g.uniform(0.5, 6, (B, Tn, 3)),
                            g.uniform(-4, 4, (B, Tn, 1))], 2).astype(np.float32)
    centre = boxes[..., :3].astype(np.float64) + np.stack([0 * boxes[..., 5], 0 * boxes[..., 5], boxes[..., 5] * 0.5], -1)

    def draw(b, idx):
        p = np.stack([g.uniform(-12, 12, len(idx)), g.uniform(-12, 12, len(idx)), g.uniform(-4, 8, len(idx))], 1)
        near = idx % 2 == 1
        p[near] = centre[b, g.integers(0, Tn, near.sum())] + g.normal(0, 1.5, (near.sum(), 3))
        p[idx == 0] = centre[b, -1] + g.uniform(-0.1, 0.1, ((idx == 0).sum(), 3))
        return p.astype(np.float32)

    pts = np.stack([draw(b, np.arange(M)) for b in range(B)])
    for _ in range(200):
        bad = np.stack([G.pts_face_distance64(pts[b], boxes[b]).min(1) <= 2 * FACE_MARGIN for b in range(B)])
        if not bad.any():
            break
        for b in range(B):
            pts[b, bad[b]] = draw(b, np.flatnonzero(bad[b]))
    part = G.pts_in_boxes64(pts, boxes)
    allb = G.pts_in_boxes64(pts, boxes, all_boxes=True)
    return pts, boxes, part, allb


@pytest.mark.parametrize('B,M,Tn', [(1, 1, 257), (2, 65, 256), (2, 1000, 600), (3, 63, 1)])
def test_points_in_boxes_beyond_one_tile(B, M, Tn):
    pts, boxes, want_part, want_all = _scene(B, M, Tn)
    assert pts.shape == (B, M, 3) and boxes.shape == (B, Tn, 7)
    assert min(G.pts_face_distance64(pts[b], boxes[b]).min() for b in range(B)) > FACE_MARGIN
    assert np.all(want_all[:, 0, Tn - 1] == 1)                  # the last box (of a partial last tile) holds a point
    if M >= 1000:
        assert (want_part >= 0).sum() > 300 and (want_all[:, :, 256:].sum() > 100) and (want_all.sum(2) > 1).sum() > 100
    part = ops.points_in_boxes_part(_dev(pts), _dev(boxes)).cpu().numpy()
    allb = ops.points_in_boxes_all(_dev(pts), _dev(boxes)).cpu().numpy()
    assert part.shape == (B, M) and allb.shape == (B, M, Tn) and part.dtype == allb.dtype == np.int32
    assert np.array_equal(allb, want_all)
    assert np.array_equal(part, want_part)
    first = np.where(allb.any(2), allb.argmax(2), -1)           # every row of `all` agrees with `part`
    assert np.array_equal(first, part)


def _face_case():
    """Yaw 0 and dyadic coordinates: float32 is exact, a point ON a face is on it in the kernel too. 260 boxes, so the boxes
    under test lie in the first tile of the `all` kernel (index 3, 4) and in its second, partial one (258, 259)."""
    far = np.array([100.0, 100.0, 50.0, 1.0, 1.0, 1.0, 0.0])
    boxes = np.tile(far, (260, 1))
    box = np.array([2.0, -4.0, 1.0, 4.0, 2.0, 0.5, 0.0])        # x in (0, 4), y in (-5, -3), z in [1, 1.5]
    wide = np.array([2.0, -4.0, 0.5, 8.0, 4.0, 2.0, 0.0])       # x in (-2, 6), y in (-6, -2), z in [0.5, 2.5]: holds `box`
    boxes[3], boxes[4], boxes[258], boxes[259] = box, wide, box + [16, 0, 0, 0, 0, 0, 0], wide + [16, 0, 0, 0, 0, 0, 0]
    inside = [[2, -4, 1.5], [2, -4, 1.0], [0.125, -4.875, 1.5], [3.875, -3.125, 1.0]]      # top / bottom face, near the sides
    on_side = [[0, -4, 1.25], [4, -4, 1.25], [2, -5, 1.25], [2, -3, 1.25], [0, -5, 1.0], [4, -3, 1.5]]   # side faces, edges
    beyond = [[2, -4, 1.625], [2, -4, 0.875]]
    wide_side = [[-2, -4, 1.25], [6, -4, 1.25], [2, -6, 1.25], [2, -2, 1.25], [2, -4, 2.5], [2, -4, 0.5]]
    p = np.array(inside + on_side + beyond + wide_side, np.float64)
    pts = np.concatenate([p, p + [16, 0, 0]])
    # [first box, number of boxes] per point of the first copy; the second copy meets boxes 258 / 259 the same way
    want = [(3, 2)] * 4 + [(4, 1)] * 6 + [(4, 1)] * 2 + [(-1, 0)] * 4 + [(4, 1)] * 2
    return pts.astype(np.float32)[None], boxes.astype(np.float32)[None], want


def test_points_in_boxes_exact_faces_and_first_box_wins():
    pts, boxes, want = _face_case()
    assert np.array_equal(pts.astype(np.float64) * 8, np.round(pts.astype(np.float64) * 8))
    part = ops.points_in_boxes_part(_dev(pts), _dev(boxes)).cpu().numpy()[0]
    allb = ops.points_in_boxes_all(_dev(pts), _dev(boxes)).cpu().numpy()[0]
    n = len(want)
    assert part[:n].tolist() == [w[0] for w in want]
    assert part[n:].tolist() == [w[0] + 255 if w[0] >= 0 else -1 for w in want]
    assert allb.sum(1).tolist() == [w[1] for w in want] * 2
    assert np.array_equal(part, G.pts_in_boxes64(pts, boxes)[0]) and np.array_equal(allb, G.pts_in_boxes64(pts, boxes, True)[0])
    # top and bottom faces are inside, the four side faces are not, and of two boxes holding a point `part` names the first
    assert part[0] == part[1] == 3 and allb[0, 3] == allb[0, 4] == 1 and allb[4:8, 3].tolist() == [0] * 4


def test_points_in_boxes_nan_is_inside_nothing():
    nan = np.float32(np.nan)
    box = np.array([2.0, -4.0, 1.0, 4.0, 2.0, 0.5, 0.3], np.float32)
    boxes = np.tile(box, (270, 1))
    for base in (0, 256):                                       # both tiles of the `all` kernel
        for k in range(7):
            boxes[base + k, k] = nan
        boxes[base + 7] = nan
    probe = [2.0, -4.0, 1.25]
    pts = np.array([probe, [nan, -4, 1.25], [2, nan, 1.25], [2, -4, nan], [nan, nan, nan], probe], np.float32)
    part = ops.points_in_boxes_part(_dev(pts[None]), _dev(boxes[None])).cpu().numpy()[0]
    allb = ops.points_in_boxes_all(_dev(pts[None]), _dev(boxes[None])).cpu().numpy()[0]
    assert part.tolist() == [8, -1, -1, -1, -1, 8]
    valid = np.ones(270, np.int32)
    valid[0:8] = valid[256:264] = 0
    assert np.array_equal(allb[0], valid) and np.array_equal(allb[5], valid) and not allb[1:5].any()
    assert np.array_equal(allb, G.pts_in_boxes64(pts, boxes, True)) and np.array_equal(part, G.pts_in_boxes64(pts, boxes))


def test_points_in_boxes_empty_sides():
    pts, boxes = torch.zeros(2, 5, 3, device=DEV), torch.zeros(2, 0, 7, device=DEV)
    part, allb = ops.points_in_boxes_part(pts, boxes), ops.points_in_boxes_all(pts, boxes)
    assert part.shape == (2, 5) and part.dtype == torch.int32 and bool((part == -1).all()) and allb.shape == (2, 5, 0)
    pts, boxes = torch.zeros(2, 0, 3, device=DEV), torch.ones(2, 4, 7, device=DEV)
    assert ops.points_in_boxes_part(pts, boxes).shape == (2, 0) and ops.points_in_boxes_all(pts, boxes).shape == (2, 0, 4)
