#!/usr/bin/env python
"""Result formatting of a val-split sized test run: the per-frame host loop (``bbox2result_kitti(device=None)``) against the
device path (``kitti_format.format_kitti_dets``: one upload, one launch, one download), 3769 synthetic frames with about 13
detections each and KITTI-shaped calibration (the generator of tests/test_kitti_format_gpu.py).

    python tools_dev/bench_kitti_format.py                 # both legs + the kernel's own time, each in a child under a timeout
    python tools_dev/bench_kitti_format.py --leg host      # one leg in this process: median of --runs after --warmup

The kernel's own time comes from a ``rocprofv3 --kernel-trace --stats`` run of the device leg (a run of its own: the timed
legs are not profiled). Prints one JSON line."""
import argparse
import copy
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def leg(name, frames, runs, warmup):
    import torch
    from test_kitti_format_gpu import CLASSES, make_dataset, make_run
    infos, outs = make_run(n_frames=frames, seed=11, max_dets=26)
    ds = make_dataset(infos)
    device = None if name == 'host' else 'cuda:0'
    times = []
    for i in range(warmup + runs):
        mine = copy.deepcopy(outs)
        if device:
            torch.cuda.synchronize()
        t = time.perf_counter()
        annos = ds.bbox2result_kitti(mine, CLASSES, device=device)
        if device:
            torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t)
    return dict(leg=name, frames=frames, detections=sum(len(o['scores_3d']) for o in outs), valid=sum(len(a['score']) for a in annos),
                median_ms=1e3 * statistics.median(times), min_ms=1e3 * min(times), max_ms=1e3 * max(times), runs=runs)


def child(args, name, timeout, profile_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), '--leg', name, '--frames', str(args.frames), '--runs', str(args.runs), '--warmup', str(args.warmup)]
    if profile_dir:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', profile_dir, '--'] + cmd
    run = subprocess.run(['timeout', '-k', '10', str(timeout)] + cmd, capture_output=True, text=True)
    if run.returncode != 0:
        raise SystemExit(f'{name} leg failed ({run.returncode}):\n{run.stdout[-1000:]}\n{run.stderr[-2000:]}')
    return json.loads([l for l in run.stdout.splitlines() if l.startswith('{')][-1])


def kernel_time(profile_dir):
    """Mean duration of ``kitti_format_kernel`` from rocprofv3's kernel statistics (ns -> us)."""
    import csv
    for path in glob.glob(os.path.join(profile_dir, '**', '*kernel_stats.csv'), recursive=True):
        for row in csv.DictReader(open(path)):
            if 'kitti_format_kernel' in row.get('Name', ''):
                return dict(calls=int(row['Calls']), mean_us=float(row['AverageNs']) / 1e3, max_us=float(row['MaxNs']) / 1e3)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=['host', 'device'])
    ap.add_argument('--frames', type=int, default=3769)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=240)
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.leg, args.frames, args.runs, args.warmup)), flush=True)
        return
    host = child(args, 'host', args.timeout)
    device = child(args, 'device', args.timeout)
    with tempfile.TemporaryDirectory() as d:
        child(args, 'device', args.timeout, profile_dir=d)
        kernel = kernel_time(d)
    print(json.dumps(dict(host=host, device=device, kernel=kernel, host_over_device=host['median_ms'] / device['median_ms'])), flush=True)


if __name__ == '__main__':
    main()
