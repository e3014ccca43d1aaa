#!/usr/bin/env python
"""Supervised CenterPoint targets + loss per step: the device path (``CenterHead.get_targets``: one upload, one launch; the
losses one launch per stage) against a host restatement of the reference's per-object loop
(mmdet3d/models/dense_heads/centerpoint_head.py:435-583: tensors on the device, a handful of tiny operations, host reads and
host-to-device copies per object) feeding the same loss kernels.

Size: batch 16, the 200 x 176 map of configs/gga/gga_kitti_retrain_centerpoint.py, 3 tasks, 5 / 20 / 60 objects per frame.
Per path and size: host ms (the host clock until the last call has returned, no synchronise: how long the host is busy) and
device ms (events around the step, synchronised). The two paths alternate inside one run; the median of ``--reps`` steps after
``--warmup``. Needs the GPU: there is no fallback.

    python tools_dev/bench_center_targets.py [--reps 30] [--step] [--json out.json]
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
from gga_amd.box3d import LiDARInstance3DBoxes  # noqa: E402
from gga_amd.dense_heads import gaussian_radius_np  # noqa: E402
from gga_amd.registry import build_head  # noqa: E402

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'gga', 'gga_kitti_retrain_centerpoint.py')


def make_batch(rng, batch, n_obj):
    boxes, labels = [], []
    for _ in range(batch):
        label = rng.randint(0, 3, n_obj)
        size = np.array([[0.8, 0.6, 1.7], [1.8, 0.6, 1.7], [3.9, 1.6, 1.5]])[label] * rng.uniform(0.8, 1.2, (n_obj, 3))
        b = np.concatenate([rng.uniform(1, 69, (n_obj, 1)), rng.uniform(-39, 39, (n_obj, 1)), rng.uniform(-2, -1, (n_obj, 1)), size,
                            rng.uniform(-3.1, 3.1, (n_obj, 1))], 1).astype(np.float32)
        boxes.append(LiDARInstance3DBoxes(torch.from_numpy(b)))
        labels.append(torch.from_numpy(label.astype(np.int64)))
    return boxes, labels


def gaussian_patch(radius):
    d = 2 * radius + 1
    y, x = np.ogrid[-radius:radius + 1, -radius:radius + 1]
    h = np.exp(-(x * x + y * y) / (2 * (d / 6) ** 2))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    return h


def loop_targets(head, gt_bboxes_3d, gt_labels_3d, dev):
    """The reference's loop, restated: per frame and task fresh device tensors, per object its scalars as 0-d device tensors
    (every comparison and ``int()`` reads one back), a numpy patch uploaded and max-ed into the heat map, and the slot's
    entries written one tensor at a time."""
    tc = head.train_cfg
    K = tc['max_objs'] * tc['dense_reg']
    osf = tc['out_size_factor']
    fw, fh = head._feature_map_size()
    pc, vs = torch.tensor(tc['point_cloud_range']), torch.tensor(tc['voxel_size'])
    per_frame = []
    for boxes, labels in zip(gt_bboxes_3d, gt_labels_3d):
        labels = labels.to(dev)
        box = torch.cat((boxes.gravity_center, boxes.tensor[:, 3:]), dim=1).to(dev)
        out, flag = [], 0
        for names in head.class_names:
            sel = [torch.where(labels == flag + i) for i in range(len(names))]
            tb = torch.cat([box[m] for m in sel], dim=0)
            tcls = torch.cat([labels[m] - flag for m in sel]).long()
            flag += len(names)
            heat = box.new_zeros((len(names), fh, fw))
            anno = box.new_zeros((K, 8))
            ind = labels.new_zeros(K, dtype=torch.int64)
            mask = box.new_zeros(K, dtype=torch.uint8)
            for k in range(min(tb.shape[0], K)):
                w, l = tb[k][3] / vs[0] / osf, tb[k][4] / vs[1] / osf
                if w > 0 and l > 0:
                    radius = max(tc['min_radius'], int(gaussian_radius_np(l.double().cpu().numpy(), w.double().cpu().numpy(), tc['gaussian_overlap'])))
                    cx, cy = (tb[k][0] - pc[0]) / vs[0] / osf, (tb[k][1] - pc[1]) / vs[1] / osf
                    center = torch.tensor([cx, cy], dtype=torch.float32, device=dev)
                    ci = center.to(torch.int32)
                    if not (0 <= ci[0] < fw and 0 <= ci[1] < fh):
                        continue
                    x, y = int(ci[0]), int(ci[1])
                    left, right, top, bottom = min(x, radius), min(fw - x, radius + 1), min(y, radius), min(fh - y, radius + 1)
                    patch = torch.from_numpy(gaussian_patch(radius)[radius - top:radius + bottom, radius - left:radius + right]).to(dev, torch.float32)
                    view = heat[tcls[k]][y - top:y + bottom, x - left:x + right]
                    torch.max(view, patch, out=view)
                    ind[k] = y * fw + x
                    mask[k] = 1
                    anno[k] = torch.cat([center - torch.tensor([x, y], device=dev), tb[k][2].unsqueeze(0), tb[k][3:6].log(),
                                         torch.sin(tb[k][6]).unsqueeze(0), torch.cos(tb[k][6]).unsqueeze(0)])
            out.append((heat, anno, ind, mask))
        per_frame.append(out)
    T = len(head.class_names)
    return tuple([torch.stack([f[t][j] for f in per_frame]) for t in range(T)] for j in range(4))


GGA_CFG = os.path.join(os.path.dirname(CFG), 'gga_kitti_config.py')


def step_time(path, dev, batch, steps, warmup):
    """Train-step time of a config on two resident synthetic batches, stepped as bench.py steps its workloads (``train.Runner``,
    the next batch's front prefetched); a ``CenterPoint`` model gets the frames' boxes and labels and none of the GGA fields."""
    from gga_amd import build_model, synthetic
    from gga_amd.cnn import to_channels_last
    from gga_amd.train import Runner, setup_multi_processes
    cfg = Config.fromfile(path)
    setup_multi_processes(cfg)
    cfg.model.pts_middle_encoder['channels_last'] = True
    torch.manual_seed(0)
    model = build_model(cfg.model).to(dev)
    with torch.no_grad():
        for th in model.pts_bbox_head.task_heads:
            for name in ('reg', 'height', 'dim', 'rot'):
                getattr(th, name)[-1].weight.mul_(0.05)
    model = to_channels_last(model).train()
    runner = Runner(model, cfg, max_iters=1000, distributed=False, device=dev)
    keys = synthetic.BATCH_KEYS if cfg.model['type'] != 'CenterPoint' else ('points', 'gt_labels_3d', 'gt_bboxes_3d')
    batches = []
    for i in range(2):
        b = synthetic.make_batch(batch, start=i * batch, pc_range=tuple(cfg.model.pts_voxel_layer.point_cloud_range))
        b['points'] = [p.to(dev) for p in b['points']]
        batches.append({k: b[k] for k in tuple(keys) + ('img_metas',)})
    torch.cuda.synchronize()
    runner.inputs_ready(*batches)
    for i in range(warmup):
        runner.step(batches[i % 2], next_data=batches[(i + 1) % 2])
    torch.cuda.synchronize()
    runner.freeze_gc()
    t0 = time.perf_counter()
    for i in range(steps):
        out = runner.step(batches[(warmup + i) % 2], next_data=batches[(warmup + i + 1) % 2])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps * 1e3
    loss = float(out['loss'].detach())
    assert loss == loss, f'loss is NaN ({path})'
    return dict(config=os.path.basename(path), batch=batch, steps=steps, step_ms=dt, loss=loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--objects', type=int, nargs='+', default=[5, 20, 60])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--step', action='store_true', help='also time the train step of the new config beside gga_kitti_config.py')
    ap.add_argument('--step-batch', type=int, default=8)
    ap.add_argument('--step-steps', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_center_targets needs the GPU')
    dev = torch.device('cuda:0')
    model = Config.fromfile(CFG).model
    head = build_head(dict(model['pts_bbox_head'], train_cfg=model['train_cfg']['pts'], test_cfg=model['test_cfg']['pts'])).to(dev)
    fw, fh = head._feature_map_size()
    gen = torch.Generator(device=dev).manual_seed(0)
    preds = [[{k: torch.randn(args.batch, c, fh, fw, device=dev, generator=gen) for k, c in
               (('heatmap', n), ('reg', 2), ('height', 1), ('dim', 3), ('rot', 2))}] for n in head.num_classes]
    rows = []
    for n_obj in args.objects:
        boxes, labels = make_batch(np.random.RandomState(n_obj), args.batch, n_obj)
        paths = dict(device=lambda: head.get_targets(boxes, labels, device=dev), loop=lambda: loop_targets(head, boxes, labels, dev))
        # the two paths build the same targets: heat maps, cells and masks exactly; anno_box to the rounding of the loop's
        # device arithmetic (its cell coordinates of up to 200 come from torch's division on the device, an ulp of which is
        # 1.5e-5 of the in-cell offset; the kernel's offsets are the CPU reference's bits, tests/test_center_head_gpu.py)
        a, b = paths['device'](), paths['loop']()
        for t in range(len(head.num_classes)):
            assert torch.equal(a[0][t], b[0][t]) and torch.equal(a[2][t], b[2][t]) and torch.equal(a[3][t], b[3][t])
            assert torch.allclose(a[1][t], b[1][t], rtol=1e-6, atol=1e-4), float((a[1][t] - b[1][t]).abs().max())
        times = {k: [] for k in paths}
        for rep in range(args.warmup + args.reps):
            for name, targets in paths.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                losses = head.loss_from_targets(preds, *targets())
                e1.record()
                host = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
                assert len(losses) == 2 * len(head.num_classes)
                if rep >= args.warmup:
                    times[name].append((host, e0.elapsed_time(e1)))
        row = dict(batch=args.batch, objects_per_frame=n_obj, map=[fh, fw], tasks=len(head.num_classes), reps=args.reps)
        for name, v in times.items():
            v = np.asarray(v)
            row[f'{name}_host_ms'], row[f'{name}_device_ms'] = float(np.median(v[:, 0])), float(np.median(v[:, 1]))
            row[f'{name}_host_ms_p10_p90'] = [float(np.percentile(v[:, 0], 10)), float(np.percentile(v[:, 0], 90))]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.step:
        for _ in range(2):          # each config twice, alternating: the spread beside the difference
            for path in (GGA_CFG, CFG):
                rows.append(step_time(path, dev, args.step_batch, args.step_steps, 4))
                print(json.dumps(rows[-1]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
