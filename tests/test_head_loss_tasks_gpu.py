"""The loss kernels over all tasks of a head in one launch (F.gaussian_focal_loss_tasks, F.gather_pred_tasks,
F.box_loss_terms_tasks: the gga_task_table entry points of include/gga_hip.h) against one call per task on the same inputs:
every loss, every intermediate and every gradient bit for bit (torch.equal) - a task's bits do not depend on which other tasks
share its grid. What a task's call computes is checked against float64 in tests/test_head_loss_gpu.py - F.gaussian_focal_loss,
F.gather_pred and F.box_loss_terms are the one-task calls of the same autograd Functions.

Shapes: B = 2, K = 12, H x W = 20 x 72 (two 8 x 32 tile rows and a partial third, two tile columns and a partial third),
3 tasks with 1, 2 and 1 heat-map classes."""
import types

import numpy as np
import pytest
import torch

from gga_amd import _lib
from gga_amd import functional as F
from gga_amd.dense_heads import CenterHead_GGA

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

B, K, H, W = 2, 12, 20, 72
CFG = dict(grid_size=[2 * W, 2 * H, 1], out_size_factor=2, voxel_size=[0.16, 0.16, 4.0],
           point_cloud_range=[0.0, -3.2, -3.0, 23.04, 3.2, 1.0], code_weights=[0.5, 0.8, 0.3, 1.1, 0.7])
WEIGHTS = dict(l1_loss_weight=0.35, w_bpl=0.3, w_srl=0.17, w_pal=0.12)
FOCAL = dict(alpha=0.0, gamma=4.0, scale=5.0)
CORNERS = [0, W - 1, (H - 1) * W, H * W - 1]


def up_heat(t):
    return 1.0 + 0.25 * t


def up_box(t):
    return [1.0 + 0.1 * t, 0.7, 1.3 - 0.2 * t, 0.45, 1.9]


def make_task(seed, classes=1, live=(4, 5), cells=None, counts=(0, 1, 300), H=H, W=W):
    """One task's inputs on the CPU (maps of H x W, the module's size unless given). live[b]: live slots of frame b (the
    first ones, as the target assignment fills them);
    cells[b]: ind of the frame's first slots (the rest are drawn); counts: in-box points of the objects, cycled over the live
    slots - every other dead slot gets an entry too (its box_out columns are filled, its losses are not)."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    maps = dict(heatmap=f(B, classes, H, W) * 2.0, reg=rng.uniform(0, 1, (B, 2, H, W)).astype(np.float32),
                height=f(B, 1, H, W) * 0.4 - 1.0, dim=f(B, 3, H, W) * 0.3 + 0.6, rot=f(B, 2, H, W))
    target = (rng.uniform(0, 1, (B, classes, H, W)) ** 4).astype(np.float32)
    ind = rng.integers(0, H * W, (B, K)).astype(np.int64)
    mask = np.zeros((B, K), np.uint8)
    for b in range(B):
        mask[b, :live[b]] = 1
        if cells is not None:
            ind[b, :len(cells[b])] = cells[b]
        for k in range(live[b]):
            target[b, rng.integers(classes), ind[b, k] // W, ind[b, k] % W] = 1.0
    anno = np.concatenate([rng.uniform(0, 1200, (B, K, 4)), rng.uniform(0.2, 0.9, (B, K, 1))], -1).astype(np.float32)
    l2i = np.tile(np.array([[600., -700., 0., 40.], [180., 0., -700., 2.], [1., 0., 0., 0.27], [0., 0., 0., 1.]], np.float32), (B, K, 1, 1))
    l2i[..., :3, :] += f(B, K, 3, 4) * 0.01
    bmask = rng.integers(0, 2, (B, K, 4)).astype(np.uint8)
    xy, off, slot = [], [0], []
    for b in range(B):
        for k in range(K):
            if mask[b, k] or k % 2:
                n = counts[len(slot) % len(counts)] if mask[b, k] else 3
                cx, cy = (ind[b, k] % W) * 0.32, (ind[b, k] // W) * 0.32 - 3.2
                xy.append(np.stack([cx + rng.uniform(-2, 2, n), cy + rng.uniform(-2, 2, n)], 1).astype(np.float32))
                off.append(off[-1] + n)
                slot.append(b * K + k)
    t = torch.from_numpy
    return dict({k: t(v) for k, v in maps.items()}, target=t(target), ind=t(ind), mask=t(mask), anno=t(anno), l2i=t(l2i),
                bmask=t(bmask), xy=t(np.concatenate(xy, 0) if xy else np.zeros((0, 2), np.float32)),
                off=t(np.asarray(off, np.int32)), slot=t(np.asarray(slot, np.int32)))


def on_device(task):
    d = {k: v.to(DEV) for k, v in task.items()}
    for k in ('heatmap', 'reg', 'height', 'dim', 'rot'):
        d[k].requires_grad_(True)
    return d


def collect(ds, heat, npos, preds, terms, boxes):
    total = 0
    for t, d in enumerate(ds):
        preds[t].retain_grad()
        total = total + up_heat(t) * heat[t] + sum(u * l for u, l in zip(up_box(t), terms[t]))
    total.backward()
    torch.cuda.synchronize()
    out = []
    for t, d in enumerate(ds):
        out.append(dict(heat=heat[t].detach().cpu(), npos=npos[t].detach().cpu(), pred=preds[t].detach().cpu(),
                        terms=torch.stack([x.detach() for x in terms[t]]).cpu(), box=boxes[t].detach().cpu(),
                        g_pred=preds[t].grad.cpu(), **{'g_' + k: d[k].grad.cpu() for k in ('heatmap', 'reg', 'height', 'dim', 'rot')}))
    return out


def box_args(d, pred):
    has = d['slot'].numel() > 0
    return (pred, d['ind'], d['mask'], d['anno'], d['l2i'], d['bmask'], d['xy'], d['off'], d['slot'] if has else None)


def run_per_task(tasks):
    ds = [on_device(t) for t in tasks]
    prm = F.loss_params(B, K, CFG, **WEIGHTS)
    heat, npos, preds, terms, boxes = [], [], [], [], []
    for d in ds:
        h, n = F.gaussian_focal_loss(d['heatmap'], d['target'], **FOCAL)
        pred = F.gather_pred(d['reg'], d['height'], d['dim'], d['rot'], d['ind'], d['mask'])
        ts, box = F.box_loss_terms(*box_args(d, pred), prm)
        heat.append(h), npos.append(n), preds.append(pred), terms.append(ts), boxes.append(box)
    return collect(ds, heat, npos, preds, terms, boxes)


def run_tasks(tasks):
    ds = [on_device(t) for t in tasks]
    prm = F.loss_params(B, K, CFG, **WEIGHTS)
    heat, npos = F.gaussian_focal_loss_tasks([d['heatmap'] for d in ds], [d['target'] for d in ds], **FOCAL)
    preds = F.gather_pred_tasks([(d['reg'], d['height'], d['dim'], d['rot']) for d in ds], [d['ind'] for d in ds],
                                [d['mask'] for d in ds])
    terms, boxes = F.box_loss_terms_tasks([box_args(d, p) for d, p in zip(ds, preds)], prm)
    return collect(ds, heat, npos, preds, terms, boxes)


def same(a, b):
    """(task, key) of everything that differs between two results."""
    return [(t, k) for t, (x, y) in enumerate(zip(a, b)) for k in x if not torch.equal(x[k], y[k])]


def three_tasks():
    """Task 0: no live slot. Task 1 (2 heat-map classes): frame 0 with all K slots live, objects in the four corners of the
    map. Task 2: two and three live slots on one cell (and a dead slot on a live cell), a corner cell shared across frames."""
    shared = [[5 * W + 40, 777, 5 * W + 40, 9 * W + 3, 777, 777, 777], [H * W - 1, 31, 31, 0, 200, 201, 0]]
    return [make_task(1, 1, live=(0, 0)),
            make_task(2, 2, live=(K, 3), cells=[CORNERS + [W // 2, 8 * W - 1, 8 * W, 16 * W + 31, 16 * W + 32], CORNERS[:2]]),
            make_task(3, 1, live=(6, 5), cells=shared)]


@pytest.fixture(scope='module')
def per_task():
    tasks = three_tasks()
    return tasks, run_per_task(tasks)


def test_three_tasks_in_one_launch(per_task):
    """Losses, num_pos, pred, box_out, d/d pred and d/d of all five maps of every task: the launch over three tasks (the
    middle one with two heat-map classes: its own workgroup count in the focal kernels) against three calls."""
    tasks, ref = per_task
    got = run_tasks(tasks)
    assert same(got, ref) == []
    # the cases are what they claim to be
    assert float(ref[0]['terms'].abs().sum()) == 0.0 and all(float(ref[0]['g_' + k].abs().sum()) == 0.0 for k in ('reg', 'height', 'dim', 'rot'))
    assert int(ref[1]['npos']) > 0 and float(ref[1]['g_reg'].abs().sum()) > 0
    assert all(torch.isfinite(ref[t]['g_' + k]).all() for t in range(3) for k in ('heatmap', 'reg', 'height', 'dim', 'rot'))
    for t in (1, 2):
        assert torch.isfinite(ref[t]['g_pred']).all() and float(ref[t]['box'][..., 9:].abs().sum()) > 0


def test_shared_cells_add_in_slot_order(per_task):
    """The first live slot of a cell holds the fp32 sum over the cell's live slots added in slot order; a dead slot on the cell
    adds nothing. Checked on the batched launch's maps for the cells of task 2 that two and three slots share."""
    tasks, _ = per_task
    got = run_tasks(tasks)[2]
    ind, mask, gp = tasks[2]['ind'], tasks[2]['mask'], got['g_pred']
    maps = torch.cat([got['g_reg'], got['g_height'], got['g_dim'], got['g_rot']], 1).reshape(B, 8, H * W)
    shared = 0
    for b in range(B):
        for cell in set(ind[b][mask[b].bool()].tolist()):
            ks = [k for k in range(K) if mask[b, k] and int(ind[b, k]) == cell]
            acc = gp[b, ks[0]].clone()
            for k in ks[1:]:
                acc = acc + gp[b, k]
            assert torch.equal(maps[b, :, cell], acc), (b, cell, ks)
            shared += len(ks) > 1
    assert shared >= 3
    live = torch.zeros(B, H * W, dtype=torch.bool)
    for b in range(B):
        live[b, ind[b][mask[b].bool()]] = True
    assert float(maps.transpose(1, 2)[~live].abs().sum()) == 0.0


@pytest.mark.parametrize('n', [1, _lib.MAX_TASKS])
def test_one_task_and_a_full_table(n):
    """n_tasks = 1 and n_tasks = GGA_MAX_TASKS (heat-map classes 1..3, live slots 0..K per frame, every in-box count)."""
    tasks = [make_task(10 + t, 1 + t % 3, live=((5 * t) % (K + 1), (3 * t + 2) % (K + 1)), counts=(300, 0, 1, 65)) for t in range(n)]
    assert same(run_tasks(tasks), run_per_task(tasks)) == []


def test_more_tasks_than_a_table_holds_are_refused():
    tasks = [make_task(t) for t in range(_lib.MAX_TASKS + 1)]
    with pytest.raises(ValueError, match='tasks'):
        run_tasks(tasks)


def test_head_loss_takes_the_batched_path_with_the_same_values(per_task):
    """CenterHead_GGA.loss_from_targets: the 18 loss entries and the gradients of all maps through the task-batched functions
    equal those of its task-by-task loop (what it falls back to when the tasks' shapes differ)."""
    tasks, _ = per_task
    head = types.SimpleNamespace(train_cfg=CFG, loss_cls=types.SimpleNamespace(alpha=0.0, gamma=4.0, loss_weight=1.0),
                                 loss_bbox=types.SimpleNamespace(loss_weight=0.25))
    res = {}
    for batched in (True, False):
        head._tasks_share_a_launch = CenterHead_GGA._tasks_share_a_launch if batched else (lambda *a: False)
        ds = [on_device(t) for t in tasks]
        preds = [[{k: d[k] for k in ('heatmap', 'reg', 'height', 'dim', 'rot')}] for d in ds]
        assert CenterHead_GGA._tasks_share_a_launch(preds, [d['ind'] for d in ds])
        losses = CenterHead_GGA.loss_from_targets(head, preds, [d['target'] for d in ds], [d['anno'] for d in ds],
                                                  [d['ind'] for d in ds], [d['mask'] for d in ds], [d['l2i'] for d in ds],
                                                  [(d['xy'], d['off'], d['slot']) for d in ds], [d['bmask'] for d in ds])
        assert len(losses) == 18
        keys = [k for k in losses if 'distance' not in k]           # the head's total: heat-map, bbox and ratio terms
        sum(losses[k] for k in keys).backward()
        torch.cuda.synchronize()
        res[batched] = ([(k, v.detach().cpu()) for k, v in losses.items()],
                        [d[k].grad.cpu() for d in ds for k in ('heatmap', 'reg', 'height', 'dim', 'rot')])
    assert [k for k, _ in res[True][0]] == [k for k, _ in res[False][0]]
    for (k, a), (_, b) in zip(res[True][0], res[False][0]):
        assert torch.isfinite(a) and torch.equal(a, b), k
    assert all(torch.equal(a, b) for a, b in zip(res[True][1], res[False][1]))
    # maps of another size in one task: the loop
    odd = [[dict(p[0])] for p in preds]
    odd[1][0]['reg'] = odd[1][0]['reg'][:, :, :-1]
    assert not CenterHead_GGA._tasks_share_a_launch(odd, [d['ind'] for d in ds])


def test_tasks_of_different_map_sizes_go_task_by_task_through_the_head():
    """Three tasks whose middle one has maps of 19 x 72 instead of 20 x 72 (the same width, so the same fm_w and one ``prm``):
    CenterHead_GGA.loss_from_targets, unpatched, takes one launch group per task. Its 18 entries and the gradients of all
    fifteen maps equal F.gaussian_focal_loss / F.gather_pred / F.box_loss_terms called task by task on fresh copies."""
    tasks = [make_task(21, 1, live=(4, 5)), make_task(22, 2, live=(K, 3), H=H - 1), make_task(23, 1, live=(6, 5))]
    assert tasks[1]['reg'].shape[2:] == (H - 1, W) and int(tasks[1]['ind'].max()) < (H - 1) * W
    head = types.SimpleNamespace(train_cfg=CFG, loss_cls=types.SimpleNamespace(alpha=0.0, gamma=4.0, loss_weight=1.0),
                                 loss_bbox=types.SimpleNamespace(loss_weight=0.25),
                                 _tasks_share_a_launch=CenterHead_GGA._tasks_share_a_launch)
    maps = ('heatmap', 'reg', 'height', 'dim', 'rot')
    ds = [on_device(t) for t in tasks]
    preds = [[{k: d[k] for k in maps}] for d in ds]
    assert not CenterHead_GGA._tasks_share_a_launch(preds, [d['ind'] for d in ds])
    losses = CenterHead_GGA.loss_from_targets(head, preds, [d['target'] for d in ds], [d['anno'] for d in ds],
                                              [d['ind'] for d in ds], [d['mask'] for d in ds], [d['l2i'] for d in ds],
                                              [(d['xy'], d['off'], d['slot']) for d in ds], [d['bmask'] for d in ds])
    sum(v for k, v in losses.items() if 'distance' not in k).backward()
    # the same, task by task
    rs = [on_device(t) for t in tasks]
    prm = F.loss_params(B, K, CFG, l1_loss_weight=0.25)
    ref = {}
    for t, d in enumerate(rs):
        heat, _ = F.gaussian_focal_loss(d['heatmap'], d['target'], **FOCAL)
        pred = F.gather_pred(d['reg'], d['height'], d['dim'], d['rot'], d['ind'], d['mask'])
        (bpl, srl, pmin, px, py), _ = F.box_loss_terms(*box_args(d, pred), prm)
        ref.update({f'task{t}.distancex': px, f'task{t}.distancey': py, f'task{t}.distancemin': pmin,
                    f'task{t}.loss_heatmap': heat, f'task{t}.loss_bbox': bpl, f'task{t}.loss_ratio': srl})
    sum(v for k, v in ref.items() if 'distance' not in k).backward()
    torch.cuda.synchronize()
    assert len(losses) == 18 and list(losses) == list(ref)
    for k in ref:
        assert torch.isfinite(losses[k]) and torch.equal(losses[k], ref[k]), k
    for t, (d, r) in enumerate(zip(ds, rs)):
        for k in maps:
            assert d[k].grad.shape == tasks[t][k].shape and torch.equal(d[k].grad, r[k].grad), (t, k)
    assert all(float(d['reg'].grad.abs().sum()) > 0 for d in ds)
