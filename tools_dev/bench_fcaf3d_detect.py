#!/usr/bin/env python
"""A/B of the two paths of ``FCAF3DHead.detect``: the batch-wide ``gga_multiclass_nms3d`` (``GGA_FCAF3D_DETECT_BATCHED=1``) and
the per-scene, per-class loop (``=0``), on the same synthetic head outputs, in one process.

Shapes: B = 8 scenes, 18 classes, axis-aligned (the ScanNet config) and B = 1 and 8, 10 classes, oriented (the SUN RGB-D
config); four levels of 1000 locations per scene each, so ``nms_pre = 1000`` keeps 4 x 1000 candidates per scene. A scene holds
``--objects`` boxes; every location sits inside one of them and regresses that box with a few centimetres of jitter, scores its
class with a logit around 0 and the other classes with logits around ``--off-logit`` (a few of those pass ``score_thr = 0.01``,
as with a trained detector).

Per shape: both paths warmed up, then timed alternately (host clock around ``detect`` + a device synchronise), median / p10 /
p90 over ``--reps``; the detections of the two paths compared for equality; synchronising calls per ``detect`` counted with
torch's sync debug mode; the device time of the ``gga_multiclass_nms3d`` call alone from events around it; kernel launches
per ``detect`` counted from a profiler trace taken afterwards, in a pass of its own. One JSON line per shape. Needs a GPU."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from gga_amd import fcaf3d as MF  # noqa: E402

SHAPES = [dict(name='scannet_b8', B=8, C=18, oriented=False), dict(name='sunrgbd_b8', B=8, C=10, oriented=True),
          dict(name='sunrgbd_b1', B=1, C=10, oriented=True)]
SWITCH = 'GGA_FCAF3D_DETECT_BATCHED'


def make_levels(B, C, oriented, per_level, n_objects, off_logit, seed, dev):
    rng = np.random.default_rng(seed)
    levels = []
    objects = []
    for _ in range(B):
        size = rng.uniform([0.4, 0.4, 0.4], [2.0, 1.6, 1.2], (n_objects, 3))
        ctr = np.concatenate([rng.uniform(0, 8, (n_objects, 2)), size[:, 2:] / 2 + rng.uniform(0, 0.3, (n_objects, 1))], 1)
        objects.append((ctr, size, rng.uniform(-np.pi / 2, np.pi / 2, n_objects), rng.integers(0, C, n_objects)))
    for _ in range(4):
        centre, box, cls, xyz, scene = [], [], [], [], []
        for b, (ctr, size, yaw, label) in enumerate(objects):
            k = rng.integers(0, n_objects, per_level)
            off = rng.uniform(-0.3, 0.3, (per_level, 3)) * size[k]
            loc = ctr[k] + off
            lower, upper = size[k] / 2 + off, size[k] / 2 - off                      # distances to the faces, then a few cm of jitter
            reg = np.stack([lower, upper], 2).reshape(per_level, 6) + rng.normal(0, 0.03, (per_level, 6))
            if oriented:
                q = np.log(np.maximum(size[k, 1] / size[k, 0], 1e-3))
                a = yaw[k] + rng.normal(0, 0.05, per_level)
                reg = np.concatenate([reg, (np.sin(2 * a) * q)[:, None], (np.cos(2 * a) * q)[:, None]], 1)
            logits = rng.normal(off_logit, 1.0, (per_level, C))
            logits[np.arange(per_level), label[k]] = rng.normal(0.0, 1.5, per_level)
            centre.append(rng.normal(0.5, 1.0, (per_level, 1))), box.append(reg), cls.append(logits), xyz.append(loc)
            scene.append(np.full(per_level, b))
        f32 = lambda parts: torch.from_numpy(np.concatenate(parts).astype(np.float32)).to(dev)
        levels.append(MF.LevelOutput(f32(centre), f32(box), f32(cls), f32(xyz), torch.from_numpy(np.concatenate(scene)).to(dev)))
    return levels


def make_head(C, oriented, dev):
    return MF.FCAF3DHead(n_classes=C, in_channels=(64, 128, 256, 512), out_channels=128, n_reg_outs=8 if oriented else 6, voxel_size=.01,
                         pts_prune_threshold=100000, pts_assign_threshold=27, pts_center_threshold=18,
                         bbox_loss=dict(type='RotatedIoU3DLoss' if oriented else 'AxisAlignedIoULoss'),
                         test_cfg=dict(nms_pre=1000, iou_thr=.5, score_thr=.01)).to(dev)


def run(head, levels, metas, batched):
    os.environ[SWITCH] = '1' if batched else '0'
    with torch.no_grad():
        return head.detect(levels, metas)


def time_entry_point(fn, reps=10):
    """Median device time (events around the call on its stream) of ``functional.multiclass_nms3d`` inside ``fn``."""
    from gga_amd import functional as F
    real, spans = F.multiclass_nms3d, []

    def timed(*a, **k):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = real(*a, **k)
        stop.record()
        spans.append((start, stop))
        return out

    F.multiclass_nms3d = timed
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    finally:
        F.multiclass_nms3d = real
    return round(float(np.median([a.elapsed_time(b) for a, b in spans])), 3)


def count_syncs(fn):
    torch.cuda.set_sync_debug_mode(1)
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            fn()
        return sum('synchroniz' in str(w.message).lower() for w in seen)
    finally:
        torch.cuda.set_sync_debug_mode(0)


def count_launches(fn):
    """Kernels (and device memsets / copies) of one call, from a profiler trace; None when the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return n or None
    except Exception as exc:          # a build without device tracing
        print(f'# launches not measured: {type(exc).__name__}: {exc}', file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--per-level', type=int, default=1000)
    ap.add_argument('--objects', type=int, default=40)
    ap.add_argument('--off-logit', type=float, default=-6.0)
    ap.add_argument('--shapes', nargs='*', default=[s['name'] for s in SHAPES])
    ap.add_argument('--no-launch-count', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_fcaf3d_detect.py needs a GPU: a timing on the CPU says nothing about the device path')
    dev = torch.device('cuda:0')
    was = os.environ.get(SWITCH)
    for shape in SHAPES:
        if shape['name'] not in args.shapes:
            continue
        B, C, oriented = shape['B'], shape['C'], shape['oriented']
        head = make_head(C, oriented, dev)
        levels = make_levels(B, C, oriented, args.per_level, args.objects, args.off_logit, 7, dev)
        metas = [dict(box_type_3d=MF.DepthInstance3DBoxes)] * B
        for _ in range(args.warmup):
            out_b, out_l = run(head, levels, metas, True), run(head, levels, metas, False)
        torch.cuda.synchronize()
        same = all(torch.equal(a[0].tensor, b[0].tensor) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) for a, b in zip(out_b, out_l))
        times = {True: [], False: []}
        for _ in range(args.reps):
            for batched in (True, False):
                torch.cuda.synchronize()
                t = time.perf_counter()
                run(head, levels, metas, batched)
                torch.cuda.synchronize()
                times[batched].append((time.perf_counter() - t) * 1e3)
        score = torch.cat([l.cls.sigmoid() * l.centre.sigmoid() for l in levels])
        scene = torch.cat([l.scene for l in levels])
        per_segment = torch.stack([(score[scene == b] > 0.01).sum(0) for b in range(B)]).float()
        rec = dict(shape=shape['name'], scenes=B, classes=C, oriented=oriented, candidates_per_scene=4 * args.per_level,
                   detections=sum(len(o[1]) for o in out_b), same_detections=bool(same),
                   candidates_per_segment_mean=round(float(per_segment.mean()), 1), candidates_per_segment_max=int(per_segment.max()),
                   non_empty_segments=int((per_segment > 0).sum()))
        for batched, key in ((True, 'batched'), (False, 'loop')):
            t = np.array(times[batched])
            rec[key] = dict(median_ms=round(float(np.median(t)), 3), p10_ms=round(float(np.percentile(t, 10)), 3),
                            p90_ms=round(float(np.percentile(t, 90)), 3), min_ms=round(float(t.min()), 3),
                            syncs=count_syncs(lambda: run(head, levels, metas, batched)))
        rec['batched']['nms_entry_point_device_ms'] = time_entry_point(lambda: run(head, levels, metas, True))
        if not args.no_launch_count:
            for batched, key in ((True, 'batched'), (False, 'loop')):
                rec[key]['device_events'] = count_launches(lambda: run(head, levels, metas, batched))
        rec['speedup_median'] = round(rec['loop']['median_ms'] / rec['batched']['median_ms'], 2)
        print(json.dumps(rec), flush=True)
    if was is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = was


if __name__ == '__main__':
    main()
