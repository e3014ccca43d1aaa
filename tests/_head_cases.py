"""Cases, float64 yardstick and comparison code of tests/test_head_loss_gpu.py (the loss kernels of gga_amd/csrc/head_loss.hip
and heatmap_focal.hip against float64 autograd). Plain functions, no fixtures; tests/test_head_cases.py runs all of it on the
CPU with the fp32 restatement in the kernel's place.

Every loss term is piecewise smooth. ``box_kinks`` / ``pal_kinks`` / ``focal_kinks`` give, in float64, how far each slot /
object / element is from its nearest kink relative to the magnitudes whose fp32 rounding could carry it across; gradients of
what lies closer than ``MARGIN`` are not compared (values are continuous and always are), and ``CAP`` bounds that share."""
import math
import os

import numpy as np
import torch

from conftest import FMAP, GOLDEN, TRAIN_CFG
from oracle import torch_ref as R

CODE_WEIGHTS = [0.5, 0.8, 0.3, 1.1, 0.7]
WEIGHTS = dict(l1_loss_weight=0.35, w_bpl=0.3, w_srl=0.17, w_pal=0.12)
UPSTREAM = [1.0, 0.7, 1.3, 0.45, 1.9]                 # d total / d (bpl, srl, pal_min, pal_x, pal_y)
PART_UP = [UPSTREAM[0]] * 4 + UPSTREAM[1:]            # the same per part of R.box_loss_terms
CFG = {c: dict(TRAIN_CFG[c], code_weights=CODE_WEIGHTS) for c in TRAIN_CFG}    # one object per geometry: F.loss_params caches by identity

MARGIN = 1e-5          # ~170 fp32 eps of the magnitudes that cancel in a slot / object
CAP = 0.05             # share of live slots / of PAL objects a gradient comparison may leave out
FOCAL_MARGIN = 4e-3    # in the logit: 1 - sigmoid(9.21) = 1e-4 carries 6e-8 / 1e-4 = 6e-4 of fp32 rounding
FOCAL_CAP = 1e-3
X_CLAMP = math.log(9999.0)
PAL_COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 1000, 5000]


def calibrations():
    d = np.load(os.path.join(GOLDEN, 'head.npz'))
    return [d[k].astype(np.float32) for k in ('second.meta_l2i.0', 'second.meta_l2i.1', 'second.meta_l2i.2', 'pp.meta_l2i.0',
                                              'pp.meta_l2i.1')]


# ----------------------------------------------------------------------------- float64 geometry for kinks and the generator
_OX = np.array([-.5, -.5, -.5, -.5, .5, .5, .5, .5])
_OY = np.array([-.5, -.5, .5, .5, -.5, -.5, .5, .5])
_OZ = np.array([0., 1., 1., 0., 0., 1., 1., 0.])


def geometry(pred, ind, l2i, tc):
    """numpy float64: pred [n,8], ind [n], l2i [n,4,4] -> dict of per-slot / per-corner quantities and of the magnitudes
    (sums of absolute terms) that the fp32 rounding of each is proportional to."""
    pred, M = pred.astype(np.float64), l2i.astype(np.float64)
    fw = int(tc['grid_size'][0]) // int(tc['out_size_factor'])
    vs = np.asarray(tc['voxel_size'], np.float32).astype(np.float64)
    pc = np.asarray(tc['point_cloud_range'], np.float32).astype(np.float64)
    osf = float(tc['out_size_factor'])
    rot = np.arctan2(pred[:, 6], pred[:, 7])
    X = ((ind % fw) + pred[:, 0]) * vs[0] * osf + pc[0]
    Y = ((ind // fw) + pred[:, 1]) * vs[1] * osf + pc[1]
    l, w, h = np.exp(pred[:, 3]), np.exp(pred[:, 4]), np.exp(pred[:, 5])
    c, s = np.cos(rot)[:, None], np.sin(rot)[:, None]
    lx, ly, lz = l[:, None] * _OX, w[:, None] * _OY, h[:, None] * _OZ
    x, y, z = lx * c - ly * s + X[:, None], lx * s + ly * c + Y[:, None], lz + (pred[:, 2] - h * 0.5)[:, None]
    q, sq = [], []
    for i in range(3):
        t = [M[:, i, 0:1] * x, M[:, i, 1:2] * y, M[:, i, 2:3] * z, M[:, i, 3:4] + 0 * x]
        q.append(sum(t))
        sq.append(sum(np.abs(v) for v in t))
    dep = np.maximum(q[2], 0.1)
    u, v = q[0] / dep, q[1] / dep
    free = q[2] > 0.1                                    # a clamped corner divides by the constant: the depth's rounding is out
    su = (sq[0] + np.abs(u) * sq[2] * free) / dep
    sv = (sq[1] + np.abs(v) * sq[2] * free) / dep
    return dict(rot=rot, X=X, Y=Y, l=l, w=w, h=h, u=u, v=v, q2=q[2], sq2=sq[2], su=su, sv=sv,
                clamped=(q[2] <= 0.1).sum(1))


def box_kinks(geo, anno, wb, w_srl):
    """-> kink [n] (relative distance of every slot to its nearest kink; inf where no term is active), box_scale [n,4]
    (magnitude behind each 2D box side)."""
    n = len(geo['X'])
    kink = np.full(n, np.inf)
    scale = np.zeros((n, 4))
    rows = np.arange(n)
    for j in range(4):
        val, sc = (geo['u'], geo['su']) if j % 2 == 0 else (geo['v'], geo['sv'])
        order = np.argsort(val if j < 2 else -val, axis=1, kind='stable')
        b, b2 = order[:, 0], order[:, 1]
        vb, v2 = val[rows, b], val[rows, b2]
        scale[:, j] = sc[rows, b]
        d = np.minimum(np.abs(vb - v2) / np.maximum(sc[rows, b], sc[rows, b2]), np.abs(vb - anno[:, j]) / sc[rows, b])
        d = np.minimum(d, np.abs(geo['q2'][rows, b] - 0.1) / geo['sq2'][rows, b])
        kink = np.where(wb[:, j] != 0, np.minimum(kink, d), kink)
    l, w = geo['l'], geo['w']
    rl, rw = np.maximum(l, w), np.minimum(l, w)
    d = np.minimum(np.abs(l - w) / rl, np.abs(rl - rw * anno[:, 4]) / (rl + rw * np.abs(anno[:, 4])))
    kink = np.where(w_srl != 0, np.minimum(kink, d), kink)
    return kink, scale


def pal_scale(geo, s):
    return abs(geo['X'][s]) + abs(geo['Y'][s]) + geo['l'][s] + geo['w'][s]


def _local_kink(a, b, hl, hw):
    d = np.sort(np.abs(np.stack([a + hl, a - hl, b + hw, b - hw], 1)), 1)
    return np.minimum(np.minimum(d[:, 0], d[:, 1] - d[:, 0]),
                      np.minimum(np.abs(np.abs(a) - 2 * hl), np.abs(np.abs(b) - 2 * hw)))


def pal_kinks(geo, xy, off, slot):
    """-> per entry: relative distance of its nearest point to a kink (inf without points / for skipped entries)."""
    out = np.full(len(slot), np.inf)
    n = len(geo['X'])
    for o, s in enumerate(slot):
        p = xy[off[o]:off[o + 1]].astype(np.float64)
        if s < 0 or s >= n or not len(p):
            continue
        c, sn = math.cos(geo['rot'][s]), math.sin(geo['rot'][s])
        dx, dy = p[:, 0] - geo['X'][s], p[:, 1] - geo['Y'][s]
        a, b = dx * c + dy * sn, -dx * sn + dy * c
        out[o] = _local_kink(a, b, geo['l'][s] / 2, geo['w'][s] / 2).min() / pal_scale(geo, s)
    return out


def _draw_points(rng, geo, s, n, kind):
    """n points of kind 'inside' / 'far' / 'mixed' around slot s's predicted box, none within 30 margins of a kink."""
    hl, hw = geo['l'][s] / 2, geo['w'][s] / 2
    m = 30 * MARGIN * pal_scale(geo, s)
    lo, hi = dict(inside=(0.0, 0.9), far=(1.6, 4.0), mixed=(0.0, 3.2))[kind]
    got = np.zeros((0, 2))
    while len(got) < n:
        k = 2 * (n - len(got)) + 32
        ab = rng.uniform(lo, hi, (k, 2)) * np.where(rng.uniform(size=(k, 2)) < 0.5, -1.0, 1.0) * [hl, hw]
        got = np.concatenate([got, ab[_local_kink(ab[:, 0], ab[:, 1], hl, hw) >= m]])
    a, b = got[:n, 0], got[:n, 1]
    c, sn = math.cos(geo['rot'][s]), math.sin(geo['rot'][s])
    return np.stack([geo['X'][s] + a * c - b * sn, geo['Y'][s] + a * sn + b * c], 1).astype(np.float32)


# ----------------------------------------------------------------------------- box cases
CLASSES = dict(
    generic=['gen'], rotation=['rot', 'pi'], behind=['behind', 'behind', 'behind_all'], borders=['border'],
    shared=['gen', 'shared', 'gen', 'shared', 'shared'], mixed=['gen', 'rot', 'pi', 'behind', 'border', 'shared', 'behind_all'])


def _draw_box(rng, cls, k):
    """-> X, Y, z, l, w, h, theta, norm of one predicted box (float64)."""
    X = rng.uniform(3, 60)
    Y = float(np.clip(rng.uniform(-0.35, 0.35) * X, -38, 38))
    lo = rng.uniform(1.5, 5.0)
    sh = lo * rng.uniform(0.25, 0.9)
    l, w = (lo, sh) if k % 2 == 0 else (sh, lo)
    theta, norm = rng.uniform(-math.pi, math.pi), rng.uniform(0.7, 1.3)
    if cls == 'rot':
        theta = (k // 2 % 4) * math.pi / 2 - math.pi + rng.uniform(0.05, math.pi / 2 - 0.05)
        norm = 0.1 * 50.0 ** rng.uniform(0, 1)
    elif cls == 'pi':
        theta = (1 if k % 2 else -1) * (math.pi - rng.uniform(1e-3, 2e-2))
    elif cls == 'behind':
        X, Y = rng.uniform(-3.0, 2.5), rng.uniform(-4, 4)
    elif cls == 'behind_all':
        X, Y = rng.uniform(-9, -5), rng.uniform(-4, 4)
    return X, Y, rng.uniform(-1.6, -0.4), l, w, rng.uniform(1.0, 2.0), theta, norm


def box_case(c, name, B, K, n_live, seed, classes='mixed', counts=None, pal_share=0.7, pal_extra=True):
    """One deterministic case as a dict of CPU tensors (maps, ind, mask, anno, l2i, bmask, xy, off, slot) plus ``cls``
    [B,K] (class name per live slot, '' for dead ones). ``counts``: point counts of the first in-box-point entries."""
    rng = np.random.default_rng(seed)
    tc = CFG[c]
    H, W = FMAP[c]
    cell = [float(np.float32(tc['voxel_size'][i])) * tc['out_size_factor'] for i in range(2)]
    pc = tc['point_cloud_range']
    cal = calibrations()
    maps = rng.uniform(-0.5, 0.5, (B, 8, H, W))
    maps[:, 3:6] *= 1.5
    maps[:, 7] += 1.0                                    # dead cells: finite boxes, rotation away from the origin
    ind = rng.integers(0, H * W, (B, K))
    mask = np.zeros((B, K), np.uint8)
    cls = np.full((B, K), '', dtype=object)
    border_cells = [(0, W // 3), (H - 1, W // 2), (H // 3, 0), (H // 2, W - 1), (0, 0), (H - 1, W - 1)]
    names = CLASSES[classes]
    for b in range(B):
        live = np.sort(rng.choice(K, min(n_live, K), replace=False))
        prev = None
        for k, s in enumerate(live):
            cl = names[(k + b) % len(names)]
            if cl == 'shared' and prev is None:
                cl = 'gen'
            X, Y, z, l, w, h, theta, norm = _draw_box(rng, cl, k)
            ix = int(np.clip(math.floor((X - pc[0]) / cell[0]), 0, W - 1))
            iy = int(np.clip(math.floor((Y - pc[1]) / cell[1]), 0, H - 1))
            if cl == 'border':
                iy, ix = border_cells[(k // len(names) + b) % len(border_cells)]
                if b == B - 1 and k < len(names):
                    iy, ix = H - 1, W - 1               # the last cell of the last frame
            if b > 0 and k == 0 and cl != 'border':
                iy, ix = first_cell                     # the cell frame 0 uses too: the frames must stay separate
            if cl == 'shared':
                iy, ix = prev                           # this slot names the cell of the live slot before it
            else:
                maps[b, :, iy, ix] = [(X - pc[0]) / cell[0] - ix, (Y - pc[1]) / cell[1] - iy, z, math.log(l),
                                      math.log(w), math.log(h), norm * math.sin(theta), norm * math.cos(theta)]
            if b == 0 and k == 0:
                first_cell = (iy, ix)
            prev = (iy, ix)
            ind[b, s], mask[b, s], cls[b, s] = iy * W + ix, 1, cl
        dead = np.flatnonzero(mask[b] == 0)
        if len(dead) and prev is not None:
            ind[b, dead[0]] = prev[0] * W + prev[1]       # a dead slot on a live slot's cell
    maps = maps.astype(np.float32)
    l2i = np.stack([cal[(b + seed) % len(cal)] for b in range(B)])[:, None].repeat(K, 1)
    bmask = (rng.uniform(size=(B, K, 4)) < 0.75).astype(np.uint8)
    # targets from the float64 geometry of what the maps hold: both sides of every box side, both signs of the SRL residual
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    pred = R.gather_pred(t(maps[:, 0:2]), t(maps[:, 2:3]), t(maps[:, 3:6]), t(maps[:, 6:8]), t(ind)).numpy().reshape(B * K, 8)
    geo = geometry(pred, ind.reshape(-1), l2i.reshape(-1, 4, 4), tc)
    box = np.stack([geo['u'].min(1), geo['v'].min(1), geo['u'].max(1), geo['v'].max(1)], 1)
    sc = np.stack([geo['su'].max(1), geo['sv'].max(1)] * 2, 1)
    sign = np.where(rng.uniform(size=box.shape) < 0.5, -1.0, 1.0)
    anno = np.zeros((B * K, 5))
    anno[:, :4] = box + sign * (rng.uniform(4, 40, box.shape) + 100 * MARGIN * sc)
    ratio = np.maximum(geo['l'], geo['w']) / np.minimum(geo['l'], geo['w'])
    anno[:, 4] = ratio * np.where(rng.uniform(size=B * K) < 0.5, rng.uniform(0.4, 0.8, B * K), rng.uniform(1.3, 2.0, B * K))
    # in-box points
    xy, off, slot = [], [0], []
    flat_live = np.flatnonzero(mask.reshape(-1))
    kinds = ['inside', 'far', 'mixed']
    taken = 0
    for i, s in enumerate(flat_live):
        if counts is None and rng.uniform() >= pal_share:
            continue                                     # a live slot without an entry
        npt = counts[taken] if counts is not None and taken < len(counts) else int(rng.integers(5, 150))
        if counts is not None and taken >= len(counts):
            break
        xy.append(_draw_points(rng, geo, s, npt, kinds[taken % 3]))
        off.append(off[-1] + npt)
        slot.append(int(s))
        taken += 1
    flat_dead = np.flatnonzero(mask.reshape(-1) == 0)
    if pal_extra and len(slot):
        if len(flat_dead):                               # an entry whose slot is masked out
            xy.append(_draw_points(rng, geo, flat_dead[-1], 70, 'mixed'))
            off.append(off[-1] + 70)
            slot.append(int(flat_dead[-1]))
        xy.append(rng.uniform(-5, 5, (9, 2)).astype(np.float32))        # an entry without a slot
        off.append(off[-1] + 9)
        slot.append(-1)
        order = rng.permutation(len(slot))               # entries in no particular order, -1 not last
        xy = [xy[o] for o in order]
        slot = [slot[o] for o in order]
        off = [0] + list(np.cumsum([len(p) for p in xy]))
    xy = np.concatenate(xy, 0) if xy else np.zeros((0, 2), np.float32)
    return dict(name=name, c=c, B=B, K=K, cls=cls.reshape(-1), reg=t(maps[:, 0:2]), height=t(maps[:, 2:3]), dim=t(maps[:, 3:6]),
                rot=t(maps[:, 6:8]), ind=t(ind), mask=t(mask), anno=t(anno.astype(np.float32).reshape(B, K, 5)),
                l2i=t(l2i.astype(np.float32)), bmask=t(bmask), xy=t(xy.astype(np.float32).reshape(-1, 2)),
                off=torch.tensor(off, dtype=torch.int32), slot=torch.tensor(slot, dtype=torch.int32))


BOX_CASES = {            # name: (B, K, live slots per frame, classes, in-box-point counts of the first entries)
    'generic': (4, 500, 40, 'generic', None), 'rotation': (4, 500, 40, 'rotation', None),
    'behind': (4, 500, 40, 'behind', None), 'borders': (4, 500, 24, 'borders', None), 'shared': (4, 500, 40, 'shared', None),
    'mixed': (4, 500, 42, 'mixed', None), 'one_live': (4, 500, 1, 'generic', None), 'all_live': (2, 500, 500, 'mixed', None),
    'K1': (4, 1, 1, 'generic', None), 'B1': (1, 500, 40, 'mixed', None), 'B16': (16, 500, 30, 'mixed', None),
    'pal_counts': (2, 500, 8, 'generic', PAL_COUNTS), 'pal_n1': (1, 7, 3, 'generic', [70]),
    'pal_n4': (2, 50, 5, 'generic', [3, 200, 64, 10]), 'pal_n5': (2, 50, 5, 'generic', [3, 200, 64, 10, 129])}


# compared (not left out) live slots that every case must keep per edge class; 'clamp_some' / 'clamp_all': 1..7 / all 8
# corners at or behind the depth clamp
MIN_COUNTS = {
    'generic': {'gen': 100, 'l<w': 40, 'l>w': 40, 'srl<0': 40, 'srl>0': 40},
    'rotation': {'rot': 60, 'pi': 60, 'quadrant0': 20, 'quadrant1': 20, 'quadrant2': 20, 'quadrant3': 20},
    'behind': {'clamp_some': 8, 'clamp_all': 8}, 'borders': {'border': 60}, 'shared': {'shared_cell': 60},
    'mixed': {'clamp_some': 8, 'clamp_all': 8, 'shared_cell': 20, 'pi': 8, 'rot': 8, 'border': 8},
    'all_live': {'clamp_some': 8, 'shared_cell': 100}, 'B16': {'clamp_some': 8, 'shared_cell': 60},
    'pal_counts': {'gen': 10}, 'one_live': {'gen': 4}, 'K1': {'gen': 4}}


def make_box_case(c, name):
    B, K, n_live, classes, counts = BOX_CASES[name]
    seed = 1000 * (1 + sorted(BOX_CASES).index(name)) + (7 if c == 'pp' else 0)
    return box_case(c, name, B, K, n_live, seed, classes, counts, pal_extra=not name.startswith('pal_n'))


def empty_case(c, B=2, K=500):
    """No live slot at all; in-box-point entries of masked-out slots only."""
    case = box_case(c, 'none', B, K, 3, 31, 'generic')
    case['mask'] = torch.zeros_like(case['mask'])
    case['cls'] = np.full(B * K, '', dtype=object)
    return case


# ----------------------------------------------------------------------------- reference runs and comparison
def reference(case, dtype, scales=False):
    """The torch restatement of gather + the five losses in ``dtype`` with autograd. -> dict(losses [5], box_out [B,K,12],
    g_pred [B,K,8], g_maps (4 tensors)); with ``scales`` also scale_pred / scale_maps: the sum over the eight parts of the
    absolute gradient of each, i.e. what cancels in g_pred / g_maps."""
    tc = CFG[case['c']]
    maps = [case[k].detach().clone().to(dtype).requires_grad_(True) for k in ('reg', 'height', 'dim', 'rot')]
    pred = R.gather_pred(*maps, case['ind'])
    losses, box_out, parts = R.box_loss_terms(pred, case['ind'], case['mask'], case['anno'], case['l2i'], case['bmask'],
                                              case['xy'], case['off'], case['slot'], tc, **WEIGHTS)
    out = dict(losses=losses.detach(), box_out=box_out.detach())
    if scales:
        sp = torch.zeros_like(pred)
        for p, up in zip(parts, PART_UP):
            if p.requires_grad:
                sp = sp + up * torch.autograd.grad(p, pred, retain_graph=True)[0].abs()
        out['scale_pred'] = sp
        out['scale_maps'] = torch.autograd.grad((pred * sp).sum(), maps, retain_graph=True)
    grads = torch.autograd.grad((losses * torch.tensor(UPSTREAM, dtype=dtype)).sum(), [pred] + maps)
    out['g_pred'], out['g_maps'] = grads[0], list(grads[1:])
    return out


def conditioning(case, r64):
    """-> dict: exclude [n] bool (live slots whose gradient is not compared), shares, per-class counts of compared slots."""
    tc = CFG[case['c']]
    B, K = case['B'], case['K']
    n = B * K
    pred = R.gather_pred(case['reg'], case['height'], case['dim'], case['rot'], case['ind']).double().numpy().reshape(n, 8)
    geo = geometry(pred, case['ind'].numpy().reshape(-1), case['l2i'].numpy().reshape(n, 4, 4), tc)
    mask = case['mask'].numpy().reshape(n).astype(bool)
    anno = case['anno'].double().numpy().reshape(n, 5)
    cw = np.asarray(CODE_WEIGHTS)
    wb = mask[:, None] * cw[:4] * case['bmask'].numpy().reshape(n, 4)
    kb, box_scale = box_kinks(geo, anno, wb, mask * cw[4])
    slot, off = case['slot'].numpy(), case['off'].numpy()
    kp = pal_kinks(geo, case['xy'].numpy(), off, slot)
    live_obj = np.array([0 <= s < n and mask[s] for s in slot], bool)
    kps = np.full(n, np.inf)
    for o, s in enumerate(slot):
        if live_obj[o]:
            kps[s] = min(kps[s], kp[o])
    exclude = mask & ((kb < MARGIN) | (kps < MARGIN))
    npts = np.zeros(n)
    for o, s in enumerate(slot):
        if 0 <= s < n:
            npts[s] += off[o + 1] - off[o]
    cls = case['cls'].copy()
    part = mask & (geo['clamped'] > 0) & (geo['clamped'] < 8)
    cls[part], cls[mask & (geo['clamped'] == 8)] = 'clamp_some', 'clamp_all'
    cells = case['ind'].numpy().reshape(B, K) + (np.arange(B) * 10 ** 7)[:, None]
    lc, cnt = np.unique(cells.reshape(-1)[mask], return_counts=True)
    on_shared = mask & np.isin(cells.reshape(-1), lc[cnt > 1])
    keep = mask & ~exclude
    counts = {k: int((keep & (cls == k)).sum()) for k in set(cls[mask])}
    counts['shared_cell'] = int((keep & on_shared).sum())
    counts['l<w'] = int((keep & (geo['l'] < geo['w'])).sum())
    counts['l>w'] = int((keep & (geo['l'] > geo['w'])).sum())
    res = np.maximum(geo['l'], geo['w']) - np.minimum(geo['l'], geo['w']) * anno[:, 4]
    counts['srl<0'], counts['srl>0'] = int((keep & (res < 0)).sum()), int((keep & (res > 0)).sum())
    for q, (lo, hi) in enumerate(((-math.pi, -math.pi / 2), (-math.pi / 2, 0), (0, math.pi / 2), (math.pi / 2, math.pi))):
        counts[f'quadrant{q}'] = int((keep & (geo['rot'] >= lo) & (geo['rot'] < hi)).sum())
    return dict(exclude=exclude, live=mask, n_live=int(mask.sum()), share=float(exclude.sum()) / max(1, int(mask.sum())),
                pal_share=float((live_obj & (kp < MARGIN)).sum()) / max(1, int(live_obj.sum())), n_pal=int(live_obj.sum()),
                counts=counts, box_scale=box_scale, geo=geo, npts=npts, clamped=geo['clamped'])


def _rel(d, scale):
    d, scale = np.abs(np.asarray(d, np.float64)), np.asarray(scale, np.float64)
    return float((d / scale).max()) if d.size else 0.0


def box_errors(got, r64, cond, case):
    """Errors of ``got`` (same dict as ``reference`` gives; any dtype / device already moved to the CPU) against the float64
    run, each relative to the per-slot magnitude of what is compared. Gradients: compared slots / their cells only."""
    n = case['B'] * case['K']
    f = lambda t: t.detach().double().cpu().numpy()
    b, b64 = f(got['box_out']).reshape(n, 12), f(r64['box_out']).reshape(n, 12)
    geo = cond['geo']
    drot = np.abs((b[:, 0] - b64[:, 0] + math.pi) % (2 * math.pi) - math.pi)        # the branch cut at +-pi is no kink
    e = {'box.rot': _rel(drot, 1.0), 'box.lw': _rel(b[:, 1:3] - b64[:, 1:3], np.abs(b64[:, 1:3])),
         'box.uv': _rel(b[:, 3:7] - b64[:, 3:7], cond['box_scale']),
         'box.xy': _rel(b[:, 7:9] - b64[:, 7:9], np.abs(b64[:, 7:9]) + 80.0),
         'box.pal': _rel(b[:, 9:12] - b64[:, 9:12], np.abs(b64[:, 9:12]) + ((cond['npts'] + 1) * (np.abs(geo['X']) + np.abs(
             geo['Y']) + geo['l'] + geo['w']))[:, None])}
    l, l64 = f(got['losses']), f(r64['losses'])
    for j, k in enumerate(('bpl', 'srl', 'pal_min', 'pal_x', 'pal_y')):
        e['loss.' + k] = abs(l[j] - l64[j]) / (abs(l64[j]) + 1e-300)
    keep = cond['live'] & ~cond['exclude']
    sp = f(r64['scale_pred']).reshape(n, 8)
    den = sp + 1e-6 * sp.max(1, keepdims=True) + 1e-300
    e['grad.pred'] = _rel((f(got['g_pred']).reshape(n, 8) - f(r64['g_pred']).reshape(n, 8))[keep], den[keep])
    # maps: cells named by compared slots and by no left-out one
    B, K = case['B'], case['K']
    ind = case['ind'].numpy()
    worst = 0.0
    for gm, gm64, sm in zip(got['g_maps'], r64['g_maps'], r64['scale_maps']):
        gm, gm64, sm = f(gm), f(gm64), f(sm)
        C = gm.shape[1]
        ok = np.zeros((B, gm.shape[2] * gm.shape[3]), bool)
        for bb in range(B):
            ok[bb, ind[bb][keep.reshape(B, K)[bb]]] = True
            ok[bb, ind[bb][cond['exclude'].reshape(B, K)[bb]]] = False
        okc = np.broadcast_to(ok[:, None], (B, C, ok.shape[1])).reshape(gm.shape)
        smx = sm.reshape(B, C, -1).max(1, keepdims=True)
        tot = np.broadcast_to(smx, (B, C, smx.shape[2])).reshape(gm.shape)
        worst = max(worst, _rel((gm - gm64)[okc], (sm + 1e-6 * tot + 1e-300)[okc]))
    e['grad.maps'] = worst
    return e


def off_cells_are_zero(g_maps, case):
    """Every cell that no live slot names holds an exact zero in all four map gradients."""
    B, K = case['B'], case['K']
    live = case['mask'].numpy().astype(bool)
    ind = case['ind'].numpy()
    for gm in g_maps:
        gm = gm.detach().cpu().numpy()
        named = np.zeros((B, gm.shape[2] * gm.shape[3]), bool)
        for b in range(B):
            named[b, ind[b][live[b]]] = True
        off = ~np.broadcast_to(named[:, None], (B, gm.shape[1], named.shape[1])).reshape(gm.shape)
        if np.any(gm[off] != 0):
            return False
    return True


# ----------------------------------------------------------------------------- focal loss
FOCAL_PAIRS = ((0.0, 4.0), (2.0, 4.0), (1.5, 3.0))
FOCAL_SIZES = {'n1': 1, 'n2': 2, 'n3': 3, 'n5': 5, 'n4k1': 4 * 257 + 1, 'n4k2': 4 * 300 + 2, 'n4k3': 4 * 4099 + 3,
               'head': 3 * 200 * 176, 'wrap': 4096 * 1024 + 4 * 5000 + 3}


def focal_case(name, positives=True):
    """logits over [-30, 30] with a dense band around the clamp at +-log(9999) and exact +-100; targets 0, 1, just below 1 and
    a Gaussian-like spread. Logits drawn within 2 margins of the clamp are moved out to 2 margins."""
    n = FOCAL_SIZES[name]
    rng = np.random.default_rng(500 + sorted(FOCAL_SIZES).index(name) + (0 if positives else 50))
    x = rng.uniform(-30, 30, n)
    band = rng.uniform(size=n) < 0.2
    x[band] = (np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0) * (X_CLAMP + rng.uniform(-1, 1, n)))[band]
    for k in (-X_CLAMP, X_CLAMP):
        near = np.abs(x - k) < 2 * FOCAL_MARGIN
        x[near] = k + np.where(x[near] >= k, 1.0, -1.0) * 2 * FOCAL_MARGIN
    x[::53] = 100.0
    x[7::53] = -100.0
    t = np.exp(-rng.uniform(0, 12, n) ** 2 / 8)
    r = rng.uniform(size=n)
    t[r < 0.3] = 0.0
    t[(r >= 0.3) & (r < 0.33)] = 1.0 - 2.0 ** -24
    t[(r >= 0.33) & (r < 0.35)] = 1.0 - 2.0 ** -12
    if positives:
        t[(r >= 0.35) & (r < 0.37)] = 1.0
        t[0] = 1.0
    t = t.astype(np.float32)
    if not positives:
        t[t == 1.0] = np.float32(1.0 - 2.0 ** -24)
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(t)


def focal_reference(x, t, alpha, gamma, scale, dtype, upstream=1.0):
    xg = x.detach().clone().to(dtype).requires_grad_(True)
    tt = t.to(dtype)
    npos = float(t.eq(1).sum())
    loss = R.gaussian_focal(R.clip_sigmoid(xg), tt, alpha, gamma, max(npos, 1.0)) * scale
    (loss * upstream).backward()
    return loss.detach(), xg.grad, npos


def focal_kinks(x):
    """-> beyond [n] bool (clamped in float64: the gradient there is an exact zero), near [n] bool (within the margin)."""
    x = x.double().numpy()
    return np.abs(x) > X_CLAMP, np.abs(np.abs(x) - X_CLAMP) < FOCAL_MARGIN


def focal_errors(loss, grad, l64, g64, x):
    """-> e: loss, gradient where 1 - sigmoid cancels (logit > 4) and elsewhere; element-wise relative (no term of the
    derivative cancels against another)."""
    beyond, near = focal_kinks(x)
    g, g64 = grad.detach().double().cpu().numpy(), g64.double().numpy()
    xs = x.numpy()
    cmp = ~near & ~beyond
    e = {'focal.loss': abs(float(loss) - float(l64)) / abs(float(l64))}
    for k, sel in (('focal.grad', cmp & (xs <= 4)), ('focal.grad_hi', cmp & (xs > 4))):
        e[k] = _rel((g - g64)[sel], np.abs(g64[sel]) + 1e-30)       # below 1e-30 fp32 runs out of exponent
    return e, float(near.mean())


def within(e, e32, floors):
    """The convolution tests' rule: an error may be the floor of its kind or twice what fp32 torch itself has."""
    return [(k, e[k], e32[k], floors[k]) for k in e if not e[k] <= max(floors[k], 2 * e32[k])]
