"""Float64 references of the post-processing geometry ops (rotated IoU, points in boxes) and generators of NMS inputs
whose answer is known in closed form. Plain numpy, TEST INFRASTRUCTURE ONLY: nothing here touches ``gga_amd`` or the C
oracle, and ``rect_iou64`` is deliberately NOT the half-plane clip that the kernel (csrc/rotated_iou.h) and the oracle
(oracle/gga_oracle.c) both use, so an error the two clips share cannot hide.

tests/test_geometry_ref.py pins everything in this file to closed forms and to the oracle before a kernel is involved.
"""
import numpy as np

AREA_CUT = 1e-14        # mmcv's single_box_iou_rotated: a box with area below this has IoU 0 with everything


def _f64_of_f32(a, cols):
    return np.asarray(a, np.float32).reshape(-1, cols).astype(np.float64)


# --------------------------------------------------------------------------------------------------- rotated IoU
def _corners(b):
    """[P,5] (x, y, w, h, angle) -> [P,4,2] corners, counter-clockwise."""
    c, s = np.cos(b[:, 4])[:, None], np.sin(b[:, 4])[:, None]
    dx = b[:, 2, None] * 0.5 * np.array([-1.0, 1.0, 1.0, -1.0])
    dy = b[:, 3, None] * 0.5 * np.array([-1.0, -1.0, 1.0, 1.0])
    return np.stack([b[:, 0, None] + dx * c - dy * s, b[:, 1, None] + dx * s + dy * c], -1)


def _inside(pts, b, eps):
    """pts [P,K,2] inside-or-on rectangle b [P,5]: the rectangle's own frame, |local| <= half extent."""
    c, s = np.cos(b[:, 4])[:, None], np.sin(b[:, 4])[:, None]
    rx, ry = pts[..., 0] - b[:, 0, None], pts[..., 1] - b[:, 1, None]
    lx, ly = rx * c + ry * s, -rx * s + ry * c
    return (np.abs(lx) <= b[:, 2, None] * 0.5 + eps) & (np.abs(ly) <= b[:, 3, None] * 0.5 + eps)


def rect_inter64(b1, b2):
    """Overlap area of the aligned pairs b1[i], b2[i] ([P,5] float64): the vertices of the overlap polygon are the corners
    of either rectangle that lie in the other one plus the crossings of their edges; ordered by angle about their
    centroid, the shoelace formula gives the area."""
    b1, b2 = b1.copy(), b2.copy()
    b2[:, :2] -= b1[:, :2]                            # exact for float32-valued inputs; keeps far-away pairs precise
    b1[:, :2] = 0.0
    P = len(b1)
    scale = np.maximum(np.abs(b1[:, 2:4]).max(1), np.abs(b2[:, 2:4]).max(1)) + np.abs(b2[:, :2]).max(1)
    eps = 1e-13 * scale[:, None]
    A, B = _corners(b1), _corners(b2)
    pts = [A, B]
    ok = [_inside(A, b2, eps), _inside(B, b1, eps)]
    ea, eb = np.roll(A, -1, 1) - A, np.roll(B, -1, 1) - B          # edge vectors
    for i in range(4):
        a0, r = A[:, i], ea[:, i]
        for j in range(4):
            b0, s = B[:, j], eb[:, j]
            den = r[:, 0] * s[:, 1] - r[:, 1] * s[:, 0]
            d = b0 - a0
            par = np.abs(den) <= 1e-12 * np.hypot(r[:, 0], r[:, 1]) * np.hypot(s[:, 0], s[:, 1])
            den = np.where(par, 1.0, den)
            t = (d[:, 0] * s[:, 1] - d[:, 1] * s[:, 0]) / den
            u = (d[:, 0] * r[:, 1] - d[:, 1] * r[:, 0]) / den
            hit = ~par & (t >= -1e-13) & (t <= 1 + 1e-13) & (u >= -1e-13) & (u <= 1 + 1e-13)
            pts.append((a0 + t[:, None] * r)[:, None])
            ok.append(hit[:, None])
    pts, ok = np.concatenate(pts, 1), np.concatenate(ok, 1)        # [P,24,2], [P,24]
    cnt = ok.sum(1)
    first = pts[np.arange(P), ok.argmax(1)]
    pts = np.where(ok[..., None], pts, first[:, None])            # an absent vertex repeats a present one: no area
    ctr = pts.mean(1, keepdims=True)
    rel = pts - ctr
    order = np.argsort(np.arctan2(rel[..., 1], rel[..., 0]), 1, kind='stable')
    rel = np.take_along_axis(rel, order[..., None], 1)
    nxt = np.roll(rel, -1, 1)
    area = 0.5 * np.abs((rel[..., 0] * nxt[..., 1] - rel[..., 1] * nxt[..., 0]).sum(1))
    return np.where(cnt >= 3, area, 0.0)


def rect_iou64(b1, b2, mode='iou', aligned=False):
    """IoU (``mode='iou'``) or intersection over the first box's area (``'iof'``) of rotated rectangles (x, y, w, h, angle),
    in float64 on the float32-rounded inputs. [N,5] x [M,5] -> [N,M], or [N] for ``aligned`` pairs. A box whose area is
    under mmcv's 1e-14 cut overlaps nothing (0, not NaN)."""
    assert mode in ('iou', 'iof')
    b1, b2 = _f64_of_f32(b1, 5), _f64_of_f32(b2, 5)
    n, m = len(b1), len(b2)
    if aligned:
        assert n == m
        p1, p2 = b1, b2
    else:
        p1, p2 = np.repeat(b1, m, 0), np.tile(b2, (n, 1))
    if len(p1) == 0:
        return np.zeros((n,) if aligned else (n, m))
    a1, a2 = p1[:, 2] * p1[:, 3], p2[:, 2] * p2[:, 3]
    live = (a1 >= AREA_CUT) & (a2 >= AREA_CUT)
    out = np.zeros(len(p1))
    if live.any():
        inter = rect_inter64(p1[live], p2[live])
        out[live] = inter / (a1[live] if mode == 'iof' else a1[live] + a2[live] - inter)
    return out if aligned else out.reshape(n, m)


def rect_iou_clip32(b1, b2, mode='iou'):
    """The kernel's algorithm (csrc/rotated_iou.h: mid-point shift, corners, Sutherland-Hodgman clip with ``>= 0`` side
    tests, shoelace) evaluated step for step in numpy float32 on aligned pairs. NOT a reference: it measures what float32
    arithmetic alone costs this algorithm on a given pair, which bounds what may be asked of the kernel there."""
    f = np.float32
    b1, b2 = np.asarray(b1, f).reshape(-1, 5), np.asarray(b2, f).reshape(-1, 5)
    out = np.zeros(len(b1), f)

    def corners(b, sx, sy):
        c, s = np.cos(b[4]), np.sin(b[4])
        hw, hh = b[2] * f(0.5), b[3] * f(0.5)
        cx, cy = b[0] - sx, b[1] - sy
        return [(cx + dx * c - dy * s, cy + dx * s + dy * c) for dx, dy in ((-hw, -hh), (hw, -hh), (hw, hh), (-hw, hh))]

    cross = lambda ax, ay, bx, by: ax * by - ay * bx
    for k, (p, q) in enumerate(zip(b1, b2)):
        a1, a2 = p[2] * p[3], q[2] * q[3]
        if a1 < f(1e-14) or a2 < f(1e-14):
            continue
        sx, sy = (p[0] + q[0]) * f(0.5), (p[1] + q[1]) * f(0.5)
        poly, clip = corners(p, sx, sy), corners(q, sx, sy)
        for e in range(4):
            if not poly:
                break
            (ax, ay), (bx, by) = clip[e], clip[(e + 1) & 3]
            ex, ey = bx - ax, by - ay
            new = []
            for i in range(len(poly)):
                (px, py), (rx, ry) = poly[i], poly[(i + 1) % len(poly)]
                dp, dr = cross(ex, ey, px - ax, py - ay), cross(ex, ey, rx - ax, ry - ay)
                if dp >= 0:
                    new.append((px, py))
                if (dp >= 0) != (dr >= 0):
                    t = dp / (dp - dr)
                    new.append((px + t * (rx - px), py + t * (ry - py)))
            poly = new
        inter = f(0)
        if len(poly) >= 3:
            area = f(0)
            for i in range(len(poly)):
                area = area + cross(*poly[i], *poly[(i + 1) % len(poly)])
            inter = np.abs(area) * f(0.5)
        out[k] = inter / (a1 if mode == 'iof' else a1 + a2 - inter)
    return out.astype(np.float64)


# --------------------------------------------------------------------------------------------------- points in boxes
def pts_face_distance64(points, boxes):
    """[M,3] x [T,7] -> [M,T]: distance of each point from the nearest face plane of each box (float64)."""
    p, b = _f64_of_f32(points, 3), _f64_of_f32(boxes, 7)
    lx, ly, lz = _local(p, b)
    return np.minimum(np.minimum(np.abs(np.abs(lx) - b[:, 3] * 0.5), np.abs(np.abs(ly) - b[:, 4] * 0.5)),
                      np.abs(np.abs(lz) - b[:, 5] * 0.5))


def _local(p, b):
    sx, sy = p[:, None, 0] - b[None, :, 0], p[:, None, 1] - b[None, :, 1]
    c, s = np.cos(b[:, 6])[None], np.sin(b[:, 6])[None]
    return sx * c + sy * s, -sx * s + sy * c, p[:, None, 2] - (b[None, :, 2] + b[None, :, 5] * 0.5)


def pts_in_boxes64(points, boxes, all_boxes=False):
    """mmcv's points_in_boxes rule in float64 on the float32-rounded inputs: a point is in a box (x, y, z_bottom, dx, dy, dz,
    yaw) when |z - z_centre| <= dz / 2 (the top and bottom faces belong to the box) and its offsets along the box's own
    axes are STRICTLY inside +-dx/2 and +-dy/2 (the side faces do not). NaN anywhere: not inside.
    points [M,3] / boxes [T,7] -> [M,T] flags (``all_boxes``) or [M] index of the FIRST box holding the point, -1 for none;
    with a leading batch dimension on both, frame by frame."""
    points, boxes = np.asarray(points, np.float32), np.asarray(boxes, np.float32)
    if points.ndim == 3:
        res = [pts_in_boxes64(p, b, all_boxes) for p, b in zip(points, boxes)]
        shape = (0, points.shape[1], boxes.shape[1]) if all_boxes else (0, points.shape[1])
        return np.stack(res) if res else np.zeros(shape, np.int32)
    p, b = _f64_of_f32(points, 3), _f64_of_f32(boxes, 7)
    with np.errstate(invalid='ignore'):
        lx, ly, lz = _local(p, b)
        flags = (np.abs(lz) <= b[:, 5] * 0.5) & (np.abs(lx) < b[:, 3] * 0.5) & (np.abs(ly) < b[:, 4] * 0.5)
    if all_boxes:
        return flags.astype(np.int32)
    return np.where(flags.any(1), flags.argmax(1), -1).astype(np.int32) if flags.shape[1] else np.full(len(p), -1, np.int32)


# --------------------------------------------------------------------------------------------------- NMS with a known answer
# Fractions of the box length by which the copies of a group's base box are shifted along the box's own axis. Two copies
# shifted by d * w against each other have IoU (1 - d) / (1 + d). With multiples of 0.22 every pair of a group has d in
# {0.22, 0.44, 0.66, 0.88}: IoU 0.639, 0.389, 0.205, 0.064, each at least 0.11 from the threshold 0.5, and neighbours
# suppress each other while next-but-one members do not, so which members survive depends on the order of the scores.
FRACTIONS = (0.22, 0.44, 0.66, 0.88)


def _greedy(iou_or_hit, order):
    """Greedy pass over one small group: members in ``order`` (descending score); hit[i, j] = i suppresses j."""
    keep = []
    for i in order:
        if not any(iou_or_hit[k, i] for k in keep):
            keep.append(i)
    return keep


def _lattice(n_groups, pitch, g):
    side = int(np.ceil(np.sqrt(n_groups)))
    cells = g.permutation(side * side)[:n_groups]
    return np.stack([(cells % side - (side - 1) / 2.0) * pitch, (cells // side - (side - 1) / 2.0) * pitch], 1)


def nms_groups(n, thr=0.5, fractions=FRACTIONS, seed=0, pitch=12.0):
    """n rotated boxes in groups of 1 + len(fractions) (the last group may be short): a base box (w in [2, 4], h in [1, 2],
    random yaw shared by the group) and its copies shifted along its own axis by fractions[k] * w. Groups sit on a square
    lattice of ``pitch``, wider than twice any member's reach from its lattice point, so boxes of different groups are
    disjoint (IoU exactly 0). Scores are a random permutation of (1 .. n) / n: distinct.
    -> boxes [n,5] float32, scores [n] float32, keep (int64, descending score: the greedy pass inside each group on the
    float64 IoU of the float32 boxes, merged by score), margin (the least |IoU - thr| over all pairs within a group),
    group [n] (the index of each box's group)."""
    g = np.random.default_rng(seed)
    fr = np.concatenate([[0.0], np.asarray(fractions, np.float64)])
    k = len(fr)
    n_groups = (n + k - 1) // k
    w, h = g.uniform(2.0, 4.0, n_groups), g.uniform(1.0, 2.0, n_groups)
    yaw = g.uniform(-np.pi, np.pi, n_groups)
    reach = fr.max() * 4.0 + 0.5 * np.hypot(4.0, 2.0)
    assert pitch > 2 * reach + 1e-3, (pitch, reach)
    ctr = _lattice(n_groups, pitch, g)
    shift = (fr[None, :] * w[:, None])[..., None] * np.stack([np.cos(yaw), np.sin(yaw)], 1)[:, None]     # [G,k,2]
    boxes = np.concatenate([ctr[:, None] + shift, np.broadcast_to(np.stack([w, h, yaw], 1)[:, None], (n_groups, k, 3))], 2)
    boxes = boxes.reshape(-1, 5)[:n].astype(np.float32)
    group = np.repeat(np.arange(n_groups), k)[:n]
    scores = (g.permutation(n) + 1).astype(np.float32) / np.float32(n)
    # float64 IoU of every pair within a group, on the float32 boxes
    ii, jj = np.triu_indices(k, 1)
    base = np.arange(n_groups)[:, None] * k
    pi, pj = (base + ii[None]).reshape(-1), (base + jj[None]).reshape(-1)
    live = (pi < n) & (pj < n)
    pi, pj = pi[live], pj[live]
    iou = rect_iou64(boxes[pi], boxes[pj], aligned=True)
    margin = float(np.abs(iou - thr).min()) if len(iou) else np.inf
    hit = np.zeros((n, k), bool)                       # hit[i, slot of j]: i and j of one group overlap beyond thr
    over = iou > thr
    hit[pi[over], pj[over] % k] = True
    hit[pj[over], pi[over] % k] = True
    keep = []
    for s in range(n_groups):
        members = np.arange(s * k, min((s + 1) * k, n))
        local = hit[members][:, :len(members)]
        order = np.argsort(-scores[members], kind='stable')
        keep.extend(members[_greedy(local, order)])
    keep = np.asarray(keep, np.int64)
    keep = keep[np.argsort(-scores[keep], kind='stable')]
    return boxes, scores, keep, margin, group


def circle_groups(n, thresh=6.25, seed=0, pitch=24.0):
    """The same construction for circle_nms (suppression within SQUARED distance ``thresh``): groups of 5 centres at integer
    offsets (0, 2, 4, 9, 13) along x from an integer lattice point, so every squared distance within a group is an integer
    (4, 16, 25, 49, 81, ...), exact in float32 and at least 2.25 from 6.25: neighbours of the chain 0 - 2 - 4 suppress each
    other, its ends do not, the last two members stand alone. Different groups are >= 11 apart.
    -> dets [n,3] float32 (x, y, score), keep (int64, descending score), margin."""
    g = np.random.default_rng(seed)
    off = np.array([0.0, 2.0, 4.0, 9.0, 13.0])
    k = len(off)
    n_groups = (n + k - 1) // k
    assert pitch % 2 == 0 and (pitch - off.max()) ** 2 > thresh + 1
    ctr = _lattice(n_groups, pitch, g)
    assert np.array_equal(ctr, np.round(ctr))
    xy = (ctr[:, None] + np.stack([off, np.zeros(k)], 1)[None]).reshape(-1, 2)[:n]
    scores = (g.permutation(n) + 1).astype(np.float32) / np.float32(n)
    d2 = (off[:, None] - off[None]) ** 2
    margin = float(np.abs(d2[np.triu_indices(k, 1)] - thresh).min())
    hit = d2 <= thresh
    keep = []
    for s in range(n_groups):
        members = np.arange(s * k, min((s + 1) * k, n))
        order = np.argsort(-scores[members], kind='stable')
        keep.extend(members[_greedy(hit, order)])
    keep = np.asarray(keep, np.int64)
    keep = keep[np.argsort(-scores[keep], kind='stable')]
    dets = np.concatenate([xy, scores[:, None]], 1).astype(np.float32)
    assert np.array_equal(dets[:, :2].astype(np.float64), xy)       # the centres are exact in float32
    return dets, keep, margin
