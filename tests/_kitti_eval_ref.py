"""Float64 restatements for the KITTI AP evaluation tests and their golden generator: an independent rotated-box overlap
(Sutherland-Hodgman clip + shoelace area, not the reference's corner / intersection-point collection) and the image-plane
IoU. Plain numpy, per pair."""
import numpy as np

ANNO_KEYS = ('name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score')


def bev_corners(cx, cy, xd, yd, angle):
    """Corners of the BEV rectangle, rotation clockwise for a positive angle (the KITTI camera convention)."""
    c, s = np.cos(angle), np.sin(angle)
    xs = np.array([-xd, -xd, xd, xd]) / 2
    ys = np.array([-yd, yd, yd, -yd]) / 2
    return np.stack([c * xs + s * ys + cx, -s * xs + c * ys + cy], 1)


def _signed_area(p):
    x, y = p[:, 0], p[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def convex_intersection_area(p, q):
    """Area of the intersection of two convex polygons [n,2] (float64)."""
    if _signed_area(p) < 0:
        p = p[::-1]
    if _signed_area(q) < 0:
        q = q[::-1]
    out = [tuple(v) for v in p]
    for k in range(len(q)):
        a, b = q[k], q[(k + 1) % len(q)]
        side = lambda v: (b[0] - a[0]) * (v[1] - a[1]) - (b[1] - a[1]) * (v[0] - a[0])
        nxt = []
        for i in range(len(out)):
            cur, prev = out[i], out[i - 1]
            sc, sp = side(cur), side(prev)
            if sc >= 0:
                if sp < 0:
                    t = sp / (sp - sc)
                    nxt.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
                nxt.append(cur)
            elif sp >= 0:
                t = sp / (sp - sc)
                nxt.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
        out = nxt
        if not out:
            return 0.0
    return abs(_signed_area(np.array(out))) if len(out) >= 3 else 0.0


def rotated_overlaps64(dt7, gt7, metric):
    """[n_dt, n_gt] float64: metric 1 = BEV IoU, metric 2 = 3D IoU of camera boxes (location, dimensions, rotation_y)."""
    dt7, gt7 = np.asarray(dt7, np.float64).reshape(-1, 7), np.asarray(gt7, np.float64).reshape(-1, 7)
    out = np.zeros((len(dt7), len(gt7)))
    cd = [bev_corners(b[0], b[2], b[3], b[5], b[6]) for b in dt7]
    cg = [bev_corners(b[0], b[2], b[3], b[5], b[6]) for b in gt7]
    for j, b in enumerate(dt7):
        for i, q in enumerate(gt7):
            inter = convex_intersection_area(cg[i], cd[j])
            if metric == 1:
                out[j, i] = inter / (b[3] * b[5] + q[3] * q[5] - inter)
            elif inter > 0:
                ih = min(b[1], q[1]) - max(b[1] - b[4], q[1] - q[4])
                if ih > 0:
                    inc = ih * inter
                    out[j, i] = inc / (b[3] * b[4] * b[5] + q[3] * q[4] * q[5] - inc)
    return out


def image_overlaps64(dt4, gt4):
    dt4, gt4 = np.asarray(dt4, np.float64).reshape(-1, 4), np.asarray(gt4, np.float64).reshape(-1, 4)
    iw = np.minimum(dt4[:, None, 2], gt4[None, :, 2]) - np.maximum(dt4[:, None, 0], gt4[None, :, 0])
    ih = np.minimum(dt4[:, None, 3], gt4[None, :, 3]) - np.maximum(dt4[:, None, 1], gt4[None, :, 1])
    inter = np.clip(iw, 0, None) * np.clip(ih, 0, None)
    area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (area(dt4)[:, None] + area(gt4)[None, :] - inter)


def box7(anno):
    return np.concatenate([np.asarray(anno['location']).reshape(-1, 3), np.asarray(anno['dimensions']).reshape(-1, 3),
                           np.asarray(anno['rotation_y']).reshape(-1, 1)], 1)


def pack_annos(prefix, annos, out):
    """Anno dicts of all frames -> flat arrays in ``out`` (npz-friendly): one concatenated array per key + the counts."""
    out[f'{prefix}.count'] = np.array([len(a['name']) for a in annos], np.int64)
    for k in ANNO_KEYS:
        if k in annos[0]:
            out[f'{prefix}.{k}'] = np.concatenate([np.asarray(a[k]) for a in annos], 0)


def unpack_annos(prefix, z):
    count = z[f'{prefix}.count']
    off = np.concatenate([[0], np.cumsum(count)])
    keys = [k for k in ANNO_KEYS if f'{prefix}.{k}' in z]
    return [{k: z[f'{prefix}.{k}'][off[f]:off[f + 1]] for k in keys} for f in range(len(count))]
