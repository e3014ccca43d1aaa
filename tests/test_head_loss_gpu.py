"""The loss kernels (gga_amd/csrc/head_loss.hip: gather, Boundary Projection, Semantic Ratio, Point-to-Box Alignment, each with
a hand-derived gradient; heatmap_focal.hip) against float64 autograd of the torch restatement (oracle/torch_ref.py) at the
edges where such kernels go wrong. Cases, kink filter and comparison code: tests/_head_cases.py; the same cases on the CPU:
tests/test_head_cases.py.

Tolerances: every compared error ``e`` (per slot / element, relative to the magnitude of what cancels there) must satisfy
``e <= max(floor, 2 * e32)`` with ``e32`` the error of fp32 torch on the same inputs against float64 - the rule of the
convolution tests. The floors are the table of EXPERIMENTS.md 6g ("Loss kernels against float64"), which lists the measured
``e`` and ``e32`` per term."""
import numpy as np
import pytest
import torch

import _head_cases as HC
from gga_amd import functional as F
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# EXPERIMENTS.md 6g. An error below its floor passes whatever fp32 torch does on that case.
FLOORS = {'box.rot': 1e-6, 'box.lw': 1e-6, 'box.uv': 1e-6, 'box.xy': 1e-6, 'box.pal': 1e-6,
          'loss.bpl': 3e-6, 'loss.srl': 3e-6, 'loss.pal_min': 3e-6, 'loss.pal_x': 3e-6, 'loss.pal_y': 3e-6,
          'grad.pred': 1e-4, 'grad.maps': 1e-4,       # measured 7.3e-5 where fp32 torch has 2.8e-5: the (R - u k M8) / depth cancellation
          'focal.loss': 3e-6, 'focal.grad': 3e-6, 'focal.grad_hi': 3e-6}


def run_kernels(case, channels_last=False, terms=False, pred_override=None):
    """gather_pred + box_losses (or box_loss_terms) + backward with HC.UPSTREAM -> the dict HC.reference gives, on the CPU."""
    prm = F.loss_params(case['B'], case['K'], HC.CFG[case['c']], **HC.WEIGHTS)
    maps = [case[k].to(DEV) for k in ('reg', 'height', 'dim', 'rot')]
    if channels_last:
        maps = [m.contiguous(memory_format=torch.channels_last) for m in maps]
    maps = [m.requires_grad_(True) for m in maps]
    ind, mask = case['ind'].to(DEV), case['mask'].to(DEV)
    if pred_override is None:
        pred = F.gather_pred(*maps, ind, mask)
        pred.retain_grad()
    else:
        pred = pred_override.to(DEV).requires_grad_(True)
    has = case['slot'].numel() > 0
    args = (pred, ind, mask, case['anno'].to(DEV), case['l2i'].to(DEV), case['bmask'].to(DEV),
            case['xy'].to(DEV) if has else None, case['off'].to(DEV) if has else None, case['slot'].to(DEV) if has else None, prm)
    if terms:
        ts, box = F.box_loss_terms(*args)
        losses = torch.stack(list(ts))
    else:
        losses, box = F.box_losses(*args)
    (losses * torch.tensor(HC.UPSTREAM, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return dict(losses=losses.detach().cpu(), box_out=box.detach().cpu(), g_pred=pred.grad.cpu(),
                g_maps=[m.grad.cpu() for m in maps] if pred_override is None else None)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ('losses', 'box_out', 'g_pred')) and all(
        torch.equal(x, y) for x, y in zip(a['g_maps'], b['g_maps']))


@pytest.mark.parametrize('name', list(HC.BOX_CASES))
@pytest.mark.parametrize('c', ['second', 'pp'])
def test_box_losses_vs_float64(c, name):
    """box_out columns, the five losses, d/d pred and (through gather_pred) d/d maps of every case of HC.BOX_CASES: generic,
    rotation (norms 0.1..5, four quadrants, next to +-pi), behind the camera (1..7 and 8 clamped corners), map borders, shared
    cells, population (one live slot, all K live, K = 1, B = 1, B = 16) and the in-box-point layouts (0..5000 points per
    object, 1 / 4 / 5 objects, masked and slot-less entries, live slots without an entry). Floors: EXPERIMENTS.md 6g."""
    case = HC.make_box_case(c, name)
    r64 = HC.reference(case, torch.float64, scales=True)
    cond = HC.conditioning(case, r64)
    assert cond['share'] <= HC.CAP and cond['pal_share'] <= HC.CAP, (cond['share'], cond['pal_share'])
    for k, v in HC.MIN_COUNTS.get(name, {}).items():
        assert cond['counts'].get(k, 0) >= v, (k, cond['counts'])
    e32 = HC.box_errors(HC.reference(case, torch.float32), r64, cond, case)
    got = run_kernels(case)
    e = HC.box_errors(got, r64, cond, case)
    for k in e:
        print(f'{c}/{name} {k}: e {e[k]:.3e} e32 {e32[k]:.3e} floor {FLOORS[k]:.0e}')
    print(f"{c}/{name}: left out {cond['share']:.4f} of {cond['n_live']} live slots, {cond['pal_share']:.4f} of "
          f"{cond['n_pal']} objects; compared {cond['counts']}")
    assert all(torch.isfinite(v).all() for v in (got['losses'], got['box_out'], got['g_pred']))
    assert HC.off_cells_are_zero(got['g_maps'], case)
    dead = ~case['mask'].reshape(-1).bool()
    assert float(got['g_pred'].reshape(-1, 8)[dead].abs().sum()) == 0.0
    assert HC.within(e, e32, FLOORS) == []


@pytest.mark.parametrize('c', ['second', 'pp'])
def test_shared_cells_in_channels_last_maps_and_by_terms(c):
    """Maps handed over in channels-last memory, and the five-scalar entry point: bit for bit what the plain call gives on the
    shared-cell case (two and three live slots on a cell, the same cell in two frames, a dead slot on a live cell)."""
    case = HC.make_box_case(c, 'shared')
    plain = run_kernels(case)
    assert _same(plain, run_kernels(case, channels_last=True))
    assert _same(plain, run_kernels(case, terms=True))


@pytest.mark.parametrize('c', ['second', 'pp'])
def test_no_live_slot(c):
    """avg = 1e-4 + eps: all five losses and every gradient are exact zeros, nothing non-finite; the in-box-point entries of
    masked-out slots still fill their box_out columns."""
    case = HC.empty_case(c)
    got = run_kernels(case)
    assert float(got['losses'].abs().sum()) == 0.0 and float(got['g_pred'].abs().sum()) == 0.0
    assert all(float(g.abs().sum()) == 0.0 for g in got['g_maps'])
    assert torch.isfinite(got['box_out']).all()
    r64 = HC.reference(case, torch.float64, scales=True)
    cond = HC.conditioning(case, r64)
    e32 = HC.box_errors(HC.reference(case, torch.float32), r64, cond, case)
    e = HC.box_errors(got, r64, cond, case)
    assert float(r64['box_out'][..., 9].abs().sum()) > 0
    assert HC.within({k: v for k, v in e.items() if k.startswith('box.')}, e32, FLOORS) == []


@pytest.mark.parametrize('c', ['second', 'pp'])
def test_dead_slots_hold_anything(c):
    """pred rows of dead slots filled with large and non-finite values change no loss and no gradient of a live slot: bit
    identical to the run with zeros there (the kernels skip a dead slot; the reference multiplies it by a zero weight, which
    would make 0 * inf = NaN of the same rows - the kernels' behaviour is what is pinned)."""
    case = HC.make_box_case(c, 'mixed')
    pred = R.gather_pred(case['reg'], case['height'], case['dim'], case['rot'], case['ind']).contiguous()
    dead = ~case['mask'].bool()
    zeros, wild = pred.clone(), pred.clone()
    zeros[dead] = 0.0
    fill = torch.tensor([float('inf'), -float('inf'), float('nan'), 1e30, -1e30, 3e38, 88.0, -1e-40])
    n_dead = int(dead.sum())
    wild[dead] = fill.repeat(n_dead + 8)[3:3 + n_dead * 8].view(n_dead, 8)
    a, b = run_kernels(case, pred_override=zeros), run_kernels(case, pred_override=wild)
    assert torch.isfinite(a['losses']).all() and torch.equal(a['losses'], b['losses'])
    assert torch.equal(a['g_pred'], b['g_pred'])
    assert float(b['g_pred'][dead].abs().sum()) == 0.0
    live = case['mask'].bool()
    assert torch.equal(a['box_out'][live], b['box_out'][live])


# ----------------------------------------------------------------------------- exact ties, resolved by rule
def _tie_case(pred_rows, anno_rows, M, xy=None, counts=None, c='second'):
    """B = 1, K = len(rows), all live, cell 0 of the map (X = pc_range[0] = 0 exactly), every weight on."""
    K = len(pred_rows)
    pred = torch.tensor(pred_rows, dtype=torch.float32).view(1, K, 8)
    case = dict(c=c, B=1, K=K, ind=torch.zeros(1, K, dtype=torch.int64), mask=torch.ones(1, K, dtype=torch.uint8),
                anno=torch.tensor(anno_rows, dtype=torch.float32).view(1, K, 5),
                l2i=torch.tensor(M, dtype=torch.float32).view(1, 1, 4, 4).repeat(1, K, 1, 1).contiguous(),
                bmask=torch.ones(1, K, 4, dtype=torch.uint8))
    if xy is None:
        case.update(xy=torch.zeros(0, 2), off=torch.zeros(1, dtype=torch.int32), slot=torch.zeros(0, dtype=torch.int32))
    else:
        case.update(xy=torch.tensor(xy, dtype=torch.float32), off=torch.tensor(np.concatenate([[0], np.cumsum(counts)]),
                    dtype=torch.int32), slot=torch.arange(K, dtype=torch.int32))
    return case, pred


def _tie_check(case, pred, up):
    """Kernel against the fp32 torch restatement on the CPU (first index on a tie): the given upstream weights only."""
    p = pred.clone().requires_grad_(True)
    losses, box, _ = R.box_loss_terms(p, case['ind'], case['mask'], case['anno'], case['l2i'], case['bmask'], case['xy'],
                                      case['off'], case['slot'], HC.CFG[case['c']], **HC.WEIGHTS)
    (losses * torch.tensor(up)).sum().backward()
    prm = F.loss_params(case['B'], case['K'], HC.CFG[case['c']], **HC.WEIGHTS)
    pg = pred.to(DEV).requires_grad_(True)
    has = case['slot'].numel() > 0
    lk, bk = F.box_losses(pg, case['ind'].to(DEV), case['mask'].to(DEV), case['anno'].to(DEV), case['l2i'].to(DEV),
                          case['bmask'].to(DEV), case['xy'].to(DEV) if has else None, case['off'].to(DEV) if has else None,
                          case['slot'].to(DEV) if has else None, prm)
    (lk * torch.tensor(up, device=DEV)).sum().backward()
    np.testing.assert_allclose(lk.detach().cpu().numpy(), losses.detach().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(bk.cpu().numpy(), box.detach().numpy(), rtol=1e-5, atol=1e-6)
    assert float(p.grad.abs().max()) > 0
    np.testing.assert_allclose(pg.grad.cpu().numpy(), p.grad.numpy(), rtol=1e-5, atol=1e-7 * float(p.grad.abs().max()))
    return p.grad


_M_SIDE = [[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 1]]        # u = y, v = z, depth 1


def test_tie_length_equals_width():
    """l == w exactly: torch.min and torch.max both return index 0, so the reference takes BOTH the shorter and the longer
    side from l, and the whole SRL gradient goes to the length channel. (The kernel gave the width channel -coef * w before
    this test: `l >= w` alone decided both.)"""
    rows = [[0, 0, 0, 0.0, 0.0, 0, 0, 1], [0, 0, 0, 1.0, 1.0, 0, 0, 1], [0, 0, 0, -2.0, -2.0, 0, 1, 0], [0, 0, 0, 0.5, 0.5, 0, 0, 2]]
    anno = [[0, 0, 0, 0, 0.5], [0, 0, 0, 0, 2.0], [0, 0, 0, 0, 0.25], [0, 0, 0, 0, 4.0]]
    case, pred = _tie_case(rows, anno, _M_SIDE)
    g = _tie_check(case, pred, [0.0, 1.0, 0.0, 0.0, 0.0])
    assert float(g[..., 4].abs().max()) == 0.0 and float(g[..., 3].abs().min()) > 0


def test_tie_first_corner_on_equal_u():
    """rot = 0 and u = y: the four corners of a box side project to the same u, bit for bit; the side is the FIRST of them,
    and d u / d rot = +-l / 2 tells which one was taken."""
    rows = [[0, 0, 0, 1.0, 0.0, 0, 0, 1], [0, 0, 0, 0.0, 1.0, 0, 0, 2], [0, 0.5, -1, 2.0, 0.0, 1, 0, 4]]
    anno = [[-8, -8, 8, 8, 1], [8, 8, -8, -8, 1], [-8, 8, 8, -8, 1]]
    case, pred = _tie_case(rows, anno, _M_SIDE)
    g = _tie_check(case, pred, [1.0, 0.0, 0.0, 0.0, 0.0])
    assert float(g[..., 6].abs().min()) > 0                       # the rotation channel carries the choice


def test_tie_first_minimum_of_the_four_distances():
    """Points with two and four equal distances to the sides of a box at the origin (all of them powers of two)."""
    rows = [[0, 0, 0, 0.0, 0.0, 0, 0, 1], [0, 0, 0, 1.0, 0.0, 0, 0, 1], [0, 0, 0, 0.0, 0.0, 0, 0, 4]]
    anno = [[0, 0, 0, 0, 1]] * 3
    c = 'second'
    y0 = float(HC.CFG[c]['point_cloud_range'][1])        # cell 0, offsets 0: X = 0 and Y = pc_range[1], exactly
    pts = [[[0, 0], [0.25, 0.25], [-0.25, 0.25], [0.25, -0.25], [-0.25, -0.25], [0.125, 0.0]],
           [[0, 0], [1.0, 0.25]],
           [[0, 0], [0.375, 0.375], [-0.375, -0.375]]]
    xy = np.concatenate([np.asarray(p, np.float64) + [0, y0] for p in pts])
    case, pred = _tie_case(rows, anno, _M_SIDE, xy, [len(p) for p in pts], c)
    _tie_check(case, pred, [0.0, 0.0, 1.0, 0.5, 0.25])


# ----------------------------------------------------------------------------- focal loss
def _focal_check(x, t, alpha, gamma):
    l64, g64, npos64 = HC.focal_reference(x, t, alpha, gamma, 5.0, torch.float64, 0.7)
    l32, g32, _ = HC.focal_reference(x, t, alpha, gamma, 5.0, torch.float32, 0.7)
    xg = x.to(DEV).requires_grad_(True)
    loss, npos = F.gaussian_focal_loss(xg, t.to(DEV), alpha, gamma, 5.0)
    (loss * 0.7).backward()
    assert float(npos.detach()) == npos64
    g = xg.grad.cpu()
    beyond, near = HC.focal_kinks(x)
    assert torch.isfinite(g).all() and torch.isfinite(loss)
    assert float(g[torch.from_numpy(beyond & ~near)].abs().sum()) == 0.0          # clamp backward: an exact zero
    e32, _ = HC.focal_errors(l32, g32, l64, g64, x)
    e, share = HC.focal_errors(loss.detach().cpu(), g, l64, g64, x)
    assert share <= HC.FOCAL_CAP
    for k in e:
        print(f'focal n={x.numel()} ({alpha}, {gamma}) {k}: e {e[k]:.3e} e32 {e32[k]:.3e} floor {FLOORS[k]:.0e}')
    assert HC.within(e, e32, FLOORS) == []
    return npos64


@pytest.mark.parametrize('pair', HC.FOCAL_PAIRS)
@pytest.mark.parametrize('name', list(HC.FOCAL_SIZES))
def test_focal_loss_vs_float64(name, pair):
    """Logits over [-30, 30] plus +-100 with a dense band around the clamp at +-9.2102, targets 0 / 1 / just below 1 / spread;
    n of 1, 2, 3, 5, 4k+1..3, a head map of the bench shape, and one n beyond 4096 * 1024 elements (both grid-stride loops take
    a second trip). Floors: EXPERIMENTS.md 6g."""
    x, t = HC.focal_case(name)
    assert _focal_check(x, t, *pair) > 0


@pytest.mark.parametrize('name', ['n3', 'n4k3', 'head'])
def test_focal_loss_without_a_positive(name):
    """npos = 0: the average factor is 1."""
    x, t = HC.focal_case(name, positives=False)
    for pair in HC.FOCAL_PAIRS:
        assert _focal_check(x, t, *pair) == 0


def test_focal_loss_refuses_a_misaligned_view():
    """A contiguous view that starts 4 bytes into its allocation: the argument check of the entry point turns it into a Python
    exception (the kernels read float4); nothing is launched."""
    x, t = HC.focal_case('n4k1')
    base = torch.zeros(x.numel() + 1, device=DEV)
    base[1:] = x.to(DEV)
    view = base[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        F.gaussian_focal_loss(view, t.to(DEV), 0.0, 4.0, 1.0)
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        F.gaussian_focal_loss(x.to(DEV), view, 0.0, 4.0, 1.0)
    loss, _ = F.gaussian_focal_loss(view.clone(), t.to(DEV), 0.0, 4.0, 1.0)          # a copy is aligned again
    assert torch.isfinite(loss)
