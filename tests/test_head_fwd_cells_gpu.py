"""Forward of the head's regression output convs on the tiles that hold a gathered cell (gga_head_cell_tiles,
gga_head_conv3x3_fwd_tiles): the tile map against a numpy restatement, the tiled launch bit for bit against the dense one
on the active tiles and all-zero elsewhere, ``gather_pred`` equal on both, and the whole train step with the switch on and
off. Every comparison is ``torch.equal``: both paths run the same instructions per tile. Run with ``-m gpu`` on an MI355X."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from gga_amd import _lib
from gga_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TR, TW = 13, 32          # the forward tile
WIDE = 320               # pixel stride of the buffer the branches' inputs are column blocks of
COUTS = (('reg', 2), ('height', 1), ('dim', 3), ('rot', 2))          # the four maps gather_pred reads: cout 1, 2, 3
SHAPES = [(2, 13, 32), (2, 14, 33), (2, 27, 72)]
PATTERNS = ('corners', 'tile_edges', 'double', 'dead_frame', 'dead_slots', 'every_tile')


def _tiles(H, W):
    return -(-H // TR), -(-W // TW)


def _cells(pattern, B, H, W):
    """(ind [B, K] int64, mask [B, K] uint8) of a pattern; a dead slot has ind = 0, mask = 0, as pack_targets leaves it."""
    ty, tx = _tiles(H, W)
    K = max(8, ty * tx)
    ind, mask = np.zeros((B, K), np.int64), np.zeros((B, K), np.uint8)

    def put(b, cells, first=0):
        for k, (y, x) in enumerate(cells):
            ind[b, first + k], mask[b, first + k] = y * W + x, 1

    if pattern == 'corners':
        for b in range(B):
            put(b, [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)])
    elif pattern == 'tile_edges':              # both sides of a tile edge: rows 12 / 13, columns 31 / 32 (clipped to the image)
        ys, xs = sorted({min(12, H - 1), min(13, H - 1)}), sorted({min(31, W - 1), min(32, W - 1)})
        put(0, [(y, x) for y in ys for x in xs])
        put(B - 1, [(ys[-1], xs[-1])], first=2)
    elif pattern == 'double':                   # two slots on one cell
        put(0, [(H - 1, W // 2), (H - 1, W // 2)])
        put(B - 1, [(H // 2, W - 1), (0, 1), (H // 2, W - 1)], first=1)
    elif pattern == 'dead_frame':               # frame 0 has no live slot: only ind = 0 is marked there
        put(B - 1, [(H - 1, W - 1)])
    elif pattern == 'dead_slots':               # dead slots point at cell 0 while the live one sits in the last tile
        for b in range(B):
            put(b, [(H - 1, W - 1)], first=K - 1)
    else:
        assert pattern == 'every_tile'          # K >= number of tiles, one cell in every tile
        for b in range(B):
            put(b, [(min(i * TR + (i + j) % TR, H - 1), min(j * TW + (3 * i + j) % TW, W - 1)) for i in range(ty) for j in range(tx)])
    return ind, mask


def _map_ref(ind, H, W):
    """The tile that contains each index, all K slots: [B, tiles_y, tiles_x] bool."""
    ty, tx = _tiles(H, W)
    ref = np.zeros((ind.shape[0], ty, tx), bool)
    for b in range(ind.shape[0]):
        for i in ind[b]:
            if 0 <= i < H * W:
                ref[b, (i // W) // TR, (i % W) // TW] = True
    return ref


def _cell_tiles(ind_dev, H, W):
    L = _lib.lib()
    B, K = ind_dev.shape
    ty, tx = _tiles(H, W)
    assert L.gga_head_cell_tiles_count(B, H, W) == B * ty * tx
    act = torch.zeros((B, ty, tx), dtype=torch.uint8, device=DEV)
    _lib.check(L.gga_head_cell_tiles(F._p(ind_dev), B, K, H, W, F._p(act), F._stream()), 'gga_head_cell_tiles')
    return act


def _pixels(act, H, W):
    """[B, tiles_y, tiles_x] -> [B, 1, H, W] bool: the pixels of the active tiles."""
    return (act > 0).repeat_interleave(TR, 1).repeat_interleave(TW, 2)[:, None, :H, :W]


_INPUTS = {}


def _inputs(B, H, W):
    """The wide buffer and the four branches' parameters of a shape (made once, never written)."""
    if (B, H, W) not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * H + W)
        big = torch.randn(B, H, W, WIDE, generator=g).to(DEV)
        prm = []
        for _, cout in COUTS:
            ss = torch.cat([torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3]).to(DEV)
            prm.append((ss, (torch.randn(cout, 64, 3, 3, generator=g) * 0.1).to(DEV), torch.randn(cout, generator=g).to(DEV)))
        _INPUTS[(B, H, W)] = (big, prm)
    return _INPUTS[(B, H, W)]


_DENSE = {}


def _dense(B, H, W):
    """gga_head_conv3x3_fwd of the four branches (column blocks 0 .. 3 of the wide buffer), computed once per shape."""
    if (B, H, W) not in _DENSE:
        L = _lib.lib()
        big, prm = _inputs(B, H, W)
        ys = []
        for blk, ((_, cout), (ss, w, b)) in enumerate(zip(COUTS, prm)):
            y = torch.full((B, cout, H, W), float('nan'), device=DEV)
            _lib.check(L.gga_head_conv3x3_fwd(big.data_ptr() + 4 * 64 * blk, WIDE, F._p(ss), F._p(w), F._p(b), B, H, W, 64, cout,
                                              F._p(y), F._stream()), 'gga_head_conv3x3_fwd')
            assert bool(torch.isfinite(y).all())
            ys.append(y)
        _DENSE[(B, H, W)] = ys
    return _DENSE[(B, H, W)]


def _tiled(B, H, W, act):
    L = _lib.lib()
    big, prm = _inputs(B, H, W)
    ys = []
    for blk, ((_, cout), (ss, w, b)) in enumerate(zip(COUTS, prm)):
        y = torch.zeros((B, cout, H, W), device=DEV)
        _lib.check(L.gga_head_conv3x3_fwd_tiles(big.data_ptr() + 4 * 64 * blk, WIDE, F._p(ss), F._p(w), F._p(b), B, H, W, 64, cout,
                                                F._p(act), F._p(y), F._stream()), 'gga_head_conv3x3_fwd_tiles')
        ys.append(y)
    return ys


def _check(B, H, W, ind, mask):
    ind_dev, mask_dev = torch.from_numpy(ind).to(DEV), torch.from_numpy(mask).to(DEV)
    act = _cell_tiles(ind_dev, H, W)
    ref = _map_ref(ind, H, W)
    assert np.array_equal(act.cpu().numpy(), ref.astype(np.uint8))            # exactly 0 / 1
    px = _pixels(act, H, W)
    dense, tiled = _dense(B, H, W), _tiled(B, H, W, act)
    for (name, cout), yd, yt in zip(COUTS, dense, tiled):
        on = px.expand(-1, cout, -1, -1)
        assert torch.equal(yt[on], yd[on]), name                               # the dense launch's values, bit for bit
        assert bool((yt.view(torch.int32)[~on] == 0).all()), name              # every other word untouched: +0.0
    pd, pt = F.gather_pred(*dense, ind_dev, mask_dev), F.gather_pred(*tiled, ind_dev, mask_dev)
    assert torch.equal(pd, pt)                                                  # all slots, dead ones included
    return ref


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('pattern', PATTERNS)
def test_tiled_forward_equals_dense_on_gathered_tiles(shape, pattern):
    B, H, W = shape
    ind, mask = _cells(pattern, B, H, W)
    ref = _check(B, H, W, ind, mask)
    ty, tx = _tiles(H, W)
    if pattern == 'every_tile':
        assert ref.all()
    elif pattern == 'dead_frame':
        assert ref[0].sum() == 1 and ref[0, 0, 0]                               # only the tile of ind = 0
    elif pattern == 'dead_slots':
        assert ref[:, 0, 0].all() and ref[:, -1, -1].all() and ref.sum() == ref.shape[0] * (1 if ty * tx == 1 else 2)
    elif pattern == 'tile_edges' and ty > 1 and tx > 1:
        assert ref[0, :2, :2].all() and ref[0].sum() == 4


def test_tiled_forward_at_the_head_map_size():
    # 4 x 248 x 216 with K = 500: more tiles (560) than persistent workgroups, 40 live slots per frame and 460 dead ones
    B, H, W, K = 4, 248, 216, 500
    g = np.random.default_rng(7)
    ind, mask = np.zeros((B, K), np.int64), np.zeros((B, K), np.uint8)
    ind[:, :40] = g.integers(0, H * W, (B, 40))
    mask[:, :40] = 1
    ref = _check(B, H, W, ind, mask)
    assert ref.sum() <= B * 41 < ref.size                                       # 40 cells and the dead slots' tile, of 20 x 7 per frame
    _INPUTS.pop((B, H, W)), _DENSE.pop((B, H, W))                               # (274 MB)


def test_cell_tiles_ignores_indices_outside_the_map():
    B, H, W = 2, 27, 72
    ind = np.array([[-1, H * W, 5 * W + 40, -(1 << 40)], [H * W + 7, 1 << 40, -1, H * W - 1]], np.int64)
    act = _cell_tiles(torch.from_numpy(ind).to(DEV), H, W)
    assert np.array_equal(act.cpu().numpy(), _map_ref(ind, H, W).astype(np.uint8)) and int(act.sum()) == 2


def test_cell_tiles_of_all_tasks_in_one_launch():
    # F.head_cell_tiles on the slices of one [T, B, K] tensor (what get_targets uploads: one launch) and on separate tensors
    T, B, H, W, K = 3, 2, 27, 72, 12
    ind = np.random.default_rng(3).integers(0, H * W, (T, B, K))
    ind[:, :, 6:] = 0
    dev = torch.from_numpy(ind).to(DEV)
    ref = [_map_ref(ind[t], H, W).astype(np.uint8).reshape(-1) for t in range(T)]
    for inds in ([dev[t] for t in range(T)], [dev[t].clone() for t in range(T)]):
        maps = F.head_cell_tiles(inds, H, W)
        assert len(maps) == T
        for t in range(T):
            assert np.array_equal(maps[t].cpu().numpy(), ref[t])


def _pp_step(model, data, cells_on, monkeypatch):
    """forward_train + backward of a copy of ``model``; returns (losses, gradients, buffers, head outputs, cells)."""
    from gga_amd import dense_heads
    monkeypatch.setattr(dense_heads, 'FWD_CELLS', cells_on)
    m = copy.deepcopy(model)
    seen = {}
    hook = m.pts_bbox_head.register_forward_hook(
        lambda mod, args, kwargs, out: seen.update(out=out, cells=kwargs.get('cells')), with_kwargs=True)
    torch.manual_seed(11)                               # the SRL draws come from the CPU generator
    losses = m.forward_train(**data)
    total, _ = m._parse_losses(losses)
    total.backward()
    hook.remove()
    torch.cuda.synchronize()
    return (losses, {n: p.grad for n, p in m.named_parameters()}, dict(m.named_buffers()), seen['out'], seen['cells'])


def test_train_step_with_and_without_the_switch(monkeypatch):
    from gga_amd import Config, build_model, synthetic
    from gga_amd.cnn import to_channels_last
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_pointpillars_config.py'))
    torch.manual_seed(1)
    model = build_model(cfg.model)
    model.train()
    with torch.no_grad():                               # (as tests/test_model_gpu.py: regression outputs of O(1))
        for th in model.pts_bbox_head.task_heads:
            for name in ('reg', 'height', 'dim', 'rot'):
                getattr(th, name)[-1].weight.mul_(0.05)
    batch = synthetic.make_batch(2, start=50, n_points=5000, pc_range=synthetic.RANGE_PP, n_obj_range=(4, 8), n_ibp_range=(10, 200))
    model.pts_middle_encoder.channels_last = True
    model = to_channels_last(model.to(DEV))
    data = dict(batch, points=[p.to(DEV) for p in batch['points']])
    l_on, g_on, b_on, out_on, cells = _pp_step(model, data, True, monkeypatch)
    l_off, g_off, b_off, out_off, cells_off = _pp_step(model, data, False, monkeypatch)
    assert cells is not None and cells_off is None      # the switch chooses the call order
    assert len(l_on) == 18 and set(l_on) == set(l_off)
    for k in l_on:
        assert torch.equal(l_on[k], l_off[k]), k
    assert len(g_on) == len(g_off) > 0
    for n in g_on:
        assert (g_on[n] is None) == (g_off[n] is None), n
        if g_on[n] is not None:
            assert torch.equal(g_on[n], g_off[n]), n
    for n in b_on:
        assert torch.equal(b_on[n], b_off[n]), n
    # the maps: the heat-map whole, the regression maps equal on the active tiles and zero elsewhere
    n_on = 0
    for t, (pd_on, pd_off) in enumerate(zip(out_on, out_off)):
        pd_on, pd_off = pd_on[0], pd_off[0]
        assert torch.equal(pd_on['heatmap'], pd_off['heatmap'])
        B, _, H, W = pd_on['heatmap'].shape
        ref = torch.from_numpy(_map_ref(cells[t].cpu().numpy(), H, W)).to(DEV)
        px = _pixels(ref, H, W)
        n_on += int(ref.sum())
        for name, cout in COUTS:
            on = px.expand(-1, cout, -1, -1)
            assert torch.equal(pd_on[name][on], pd_off[name][on]), (t, name)
            assert bool((pd_on[name].view(torch.int32)[~on] == 0).all()), (t, name)
    assert 0 < n_on < 3 * 2 * 20 * 7 // 4
