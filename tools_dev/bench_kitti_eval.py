#!/usr/bin/env python
"""Time ``gga_amd.kitti_eval.kitti_eval`` on the synthetic set of the KITTI val split's size (3769 frames, about 10 labels and
15 detections each): wall time per call, kernel launches per call (torch profiler), one JSON line. Kernel times come from

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools_dev/bench_kitti_eval.py --calls 1

(the kitti_eval_* rows of the kernel stats). Not a bench.py leg."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=3769)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--count-launches', action='store_true')
    args = ap.parse_args()
    import torch
    from gga_amd import synthetic
    from gga_amd.kitti_eval import kitti_eval
    gts, dts = synthetic.make_kitti_eval_case(7, args.frames, n_gt=10, n_dt=15)
    classes = ['Car', 'Pedestrian', 'Cyclist']
    kitti_eval(gts, dts, classes)                       # warm-up: library load, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        text, _ = kitti_eval(gts, dts, classes)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    out = dict(frames=args.frames, labels=sum(len(g['name']) for g in gts), detections=sum(len(d['name']) for d in dts),
               kitti_eval_wall_s=sorted(times)[len(times) // 2], calls=args.calls)
    if args.count_launches:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            kitti_eval(gts, dts, classes)
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'emcpy' not in e.name and 'emset' not in e.name]
        out['kernel_launches'] = len(kernels)
        out['own_kernel_launches'] = sum('kitti_eval' in e.name or 'image_box_match' in e.name for e in kernels)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
