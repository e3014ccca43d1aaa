#!/usr/bin/env python
"""Times ``indoor_eval`` at SUN RGB-D val size - 5050 frames, 10 classes, ground truths and detections drawn like
``FCAF3DHead.forward_test`` output (synthetic.make_indoor_eval_case) - on the device path against this module's host path, and
the two kernel entry points alone with events. Warm-up first, medians of repeated runs, the clock
around a synchronised region.

    python tools_dev/bench_indoor_eval.py [--frames 5050] [--repeat 7] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))

from gga_amd import indoor_eval as IE, synthetic      # noqa: E402
from gga_amd.fcaf3d import DepthInstance3DBoxes      # noqa: E402
import _indoor_eval_ref as R      # noqa: E402


def timed(fn, repeat, sync=True):
    out = []
    for _ in range(repeat):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=5050)
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--out')
    args = ap.parse_args()
    gts, dts = synthetic.make_indoor_eval_case(7, args.frames, dt_range=(0, 120))
    results = R.as_results(dts, DepthInstance3DBoxes)
    label2cat = dict(enumerate(synthetic.INDOOR_CLASSES))
    batch = IE._columns(gts, results, None, None)
    pairs = int(((batch.det_off[1:] - batch.det_off[:-1]) * (batch.gt_off[1:] - batch.gt_off[:-1])).sum())
    res = dict(frames=args.frames, detections=len(batch.det), ground_truths=len(batch.gt), pairs=pairs, repeat=args.repeat)
    run = lambda device: IE.match_and_flag(batch.det, batch.det_off, batch.gt, batch.gt_off, batch.det_pos, R.THRESHOLDS, device)
    dev, host = run('cuda:0'), run('cpu')          # warm-up and agreement
    res['host_flags_equal'] = bool(np.array_equal(dev[2], host[2]))
    res['match_and_flag_ms'] = dict(device=timed(lambda: run('cuda:0'), args.repeat),
                                    host=timed(lambda: run('cpu'), max(args.repeat // 2, 1), sync=False))
    full = lambda device: IE.indoor_eval(gts, results, R.THRESHOLDS, label2cat, logger='silent', device=device)
    a, b = full('cuda:0'), full('cpu')
    res['ret_dict_equal'] = list(a) == list(b) and all(x == y or (x != x and y != y) for x, y in zip(a.values(), b.values()))
    res['indoor_eval_ms'] = dict(device=timed(lambda: full('cuda:0'), args.repeat), host=timed(lambda: full('cpu'), max(args.repeat // 2, 1), sync=False))
    # the launches alone, with events (device-resident operands)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    from gga_amd import _lib, functional as F
    import ctypes as C
    L = _lib.lib()
    d = [up(batch.det), up(batch.det_off), up(batch.gt), up(batch.gt_off), up(batch.det_pos)]
    n, m, s = len(batch.det), len(batch.gt), len(batch.det_off) - 1
    iou, jmax = torch.empty(n, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda')
    tp = torch.empty(2 * n, dtype=torch.uint8, device='cuda')
    ws = torch.empty(int(L.gga_indoor_eval_workspace_bytes(m, 8)), dtype=torch.uint8, device='cuda')
    thr = (C.c_float * 8)(0.25, 0.5)

    def events(fn):
        ms = []
        for _ in range(args.repeat + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(ms[2:]))
    match = lambda: _lib.check(L.gga_indoor_eval_match(F._p(d[0]), F._p(d[1]), n, F._p(d[2]), F._p(d[3]), m, s, F._p(iou), F._p(jmax), F._stream()), 'match')
    res['kernel_us'] = dict(match=events(match),
                            assign=events(lambda: _lib.check(L.gga_indoor_eval_assign(F._p(iou), F._p(jmax), F._p(d[4]), F._p(d[1]), n, F._p(d[3]), m, s,
                                                                                        C.byref(thr), 2, F._p(tp), F._p(ws), ws.numel(), F._stream()), 'assign')))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
