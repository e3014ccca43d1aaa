#!/usr/bin/env python
"""Anchor3DHead per step: targets + loss forward + backward on the device path (``functional.anchor_targets`` and
``functional.anchor_losses``: one upload, four kernels, nothing read back) against the eager path (``GGA_ANCHOR_TARGETS=0``: the
reference's loop over frames and assigners, launch for launch, and its gathered eager losses), and ``get_bboxes`` for the whole
batch against the loop over frames.

Size: batch 16 on the two KITTI maps - 200 x 176 (configs/gga/gga_kitti_retrain_second.py) and 248 x 216
(gga_kitti_retrain_pointpillars.py), 6 anchors per cell - with 5 / 20 / 60 objects per frame; ``nms_pre = 100``. The head's
inputs are seeded maps (no trunk). Per path and size the wall time of a step that ends in a device synchronise; the two paths
alternate inside one run; median and min .. max of ``--reps`` steps after ``--warmup``. Before timing, the two paths' losses are
compared at the size timed. Needs the GPU: there is no fallback.

    python tools_dev/bench_anchor_head.py [--reps 10] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gga_amd import Config  # noqa: E402
from gga_amd import anchor_head as AH  # noqa: E402
from gga_amd.box3d import LiDARInstance3DBoxes  # noqa: E402
from gga_amd.registry import build_head  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {'second': (200, 176), 'pointpillars': (248, 216)}


def make_batch(rng, batch, n_obj):
    boxes, labels = [], []
    for _ in range(batch):
        label = rng.randint(0, 3, n_obj)
        size = np.array([[0.8, 0.6, 1.73], [1.76, 0.6, 1.73], [3.9, 1.6, 1.56]])[label] * rng.uniform(0.8, 1.2, (n_obj, 3))
        b = np.concatenate([rng.uniform(1, 68, (n_obj, 1)), rng.uniform(-39, 39, (n_obj, 1)), rng.uniform(-2, -1, (n_obj, 1)), size,
                            rng.uniform(-3.1, 3.1, (n_obj, 1))], 1).astype(np.float32)
        boxes.append(LiDARInstance3DBoxes(torch.from_numpy(b)))
        labels.append(torch.from_numpy(label.astype(np.int64)))
    return boxes, labels


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--objects', type=int, nargs='+', default=[5, 20, 60])
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_anchor_head needs the GPU'
    dev = torch.device('cuda:0')
    rows = []
    for name, (H, W) in LAYOUTS.items():
        cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'gga', f'gga_kitti_retrain_{name}.py'))
        hc = dict(cfg.model['bbox_head'], train_cfg=cfg.model['train_cfg'], test_cfg=cfg.model['test_cfg'])
        torch.manual_seed(0)
        head = build_head(hc).to(dev)
        g = torch.Generator().manual_seed(1)
        B = args.batch
        maps = [(torch.randn((B, 6 * c, H, W), generator=g) * s + o).to(dev).contiguous(memory_format=torch.channels_last)
                for c, s, o in ((3, 1.0, -3.0), (7, 0.3, 0.0), (2, 1.0, 0.0))]
        metas = [dict(box_type_3d=LiDARInstance3DBoxes) for _ in range(B)]

        def train_step(gt, lb):
            leaves = [m.detach().requires_grad_(True) for m in maps]
            losses = head.loss([leaves[0]], [leaves[1]], [leaves[2]], gt, lb, metas)
            sum(v[0] for v in losses.values()).backward()
            return {k: v[0].detach() for k, v in losses.items()}

        for n_obj in args.objects:
            gt, lb = make_batch(np.random.RandomState(n_obj), B, n_obj)
            vals = {}
            for on in (True, False):
                AH.DEVICE_TARGETS = on
                vals[on] = {k: float(v) for k, v in train_step(gt, lb).items()}
            rel = max(abs(vals[True][k] - vals[False][k]) / max(abs(vals[False][k]), 1e-12) for k in vals[True])
            ms = {True: [], False: []}
            for it in range(args.warmup + args.reps):
                for on in (True, False):
                    AH.DEVICE_TARGETS = on
                    t, _ = timed(lambda: train_step(gt, lb), dev)
                    if it >= args.warmup:
                        ms[on].append(t)
            row = dict(what='targets+loss+backward', layout=name, map=[H, W], batch=B, objects=n_obj, device_ms=stats(ms[True]),
                       eager_ms=stats(ms[False]), ratio=float(np.median(ms[False]) / np.median(ms[True])), losses_rel_diff=rel)
            rows.append(row)
            print(json.dumps(row), flush=True)
        AH.DEVICE_TARGETS = True
        ms = {True: [], False: []}
        same = None
        for it in range(args.warmup + args.reps):
            res = {}
            for on in (True, False):
                AH.DETECT_BATCHED = on
                t, res[on] = timed(lambda: head.get_bboxes([maps[0]], [maps[1]], [maps[2]], metas), dev)
                if it >= args.warmup:
                    ms[on].append(t)
            if same is None:
                same = all(torch.equal(a[0].tensor.cpu(), b[0].tensor.cpu()) and torch.equal(a[1].cpu(), b[1].cpu())
                           for a, b in zip(res[True], res[False]))
                kept = [len(a[1]) for a in res[True]]
        AH.DETECT_BATCHED = True
        row = dict(what='get_bboxes', layout=name, map=[H, W], batch=B, nms_pre=head.test_cfg['nms_pre'], batched_ms=stats(ms[True]),
                   loop_ms=stats(ms[False]), ratio=float(np.median(ms[False]) / np.median(ms[True])), identical=bool(same),
                   detections=int(sum(kept)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
