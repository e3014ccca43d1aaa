"""Test-time augmentation on the PointPillars config, 6 views (3 scales x horizontal flip) of F frames: frames/s of
``GGA.aug_test`` in three forms - fused (one batch of V * F clouds, one merge launch), GGA_TTA_MERGE=0 (the same batch, the
maps merged by the per-view eager sequence) and the reference's form (per frame, V forward passes at batch 1, the eager merge,
get_bboxes per scale, the box merge) - and the number of device kernels the merge step launches in each.
Usage: tta_bench.py [--frames 1 4] [--iters 30] [--warmup 5]; prints one JSON line per (F, form)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch

from gga_amd import Config, build_model, synthetic
from gga_amd import functional as F
from gga_amd.box3d import LiDARInstance3DBoxes
from gga_amd.cnn import to_channels_last
from gga_amd.pipelines import GlobalRotScaleTrans, PointsRangeFilter, RandomFlip3D
from gga_amd.points import LiDARPoints
from gga_amd.tta import merge_aug_bboxes_3d

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = [(s, h) for s in (0.95, 1.0, 1.05) for h in (False, True)]


def make_views(frames, n_frames, dev, pc_range):
    inner = [GlobalRotScaleTrans(rot_range=[0, 0], scale_ratio_range=[1., 1.], translation_std=[0, 0, 0]),
             RandomFlip3D(sync_2d=False), PointsRangeFilter(point_cloud_range=list(pc_range))]
    points, metas = [], []
    for scale, hflip in VIEWS:
        pv, mv = [], []
        for f in range(n_frames):
            d = dict(points=LiDARPoints(frames['points'][f].cpu().clone(), points_dim=4), flip=True, pcd_scale_factor=scale,
                     pcd_horizontal_flip=hflip, pcd_vertical_flip=False)
            for t in inner:
                d = t(d)
            pv.append(d['points'].tensor.to(dev))
            mv.append(dict(box_type_3d=LiDARInstance3DBoxes, pcd_scale_factor=scale, pcd_horizontal_flip=hflip, pcd_vertical_flip=False))
        points.append(pv)
        metas.append(mv)
    return points, metas


def reference_form(model, points, metas):
    """What the reference's aug_test does, once per frame (it takes one sample per call)."""
    head = model.pts_bbox_head
    group, hflip, vflip, first = model._tta_views(metas)
    results = []
    for f in range(len(points[0])):
        views = [[head(model.extract_feat([points[v][f]], None, None)[1])] for v in range(len(points))]
        merged = model._tta_merge_views_eager(views, group, hflip, vflip)
        aug = []
        for s in range(len(first)):
            one = [[{k: x[s:s + 1] for k, x in task[0].items()}] for task in merged]
            b, sc, lb = head.get_bboxes(one, [metas[first[s]][f]], rescale=True)[0]
            aug.append(dict(boxes_3d=b, scores_3d=sc, labels_3d=lb))
        results.append(merge_aug_bboxes_3d(aug, [[metas[v][f]] for v in first], head.test_cfg))
    return results


def kernels_of(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    # every kernel on the device's timeline, whoever launched it (the HIP entry points are called through ctypes: no
    # framework op owns their kernels)
    return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA
               and not ev.name.lower().startswith(('memcpy', 'memset')))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tta_bench.py measures on the GPU; none is visible')
    dev = torch.device('cuda:0')
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_pointpillars_config.py'))
    cfg.model.pts_middle_encoder['channels_last'] = True          # the form apis.generate_pseudo_labels runs
    torch.manual_seed(0)
    model = to_channels_last(build_model(cfg.model).to(dev)).eval()
    with torch.no_grad():
        for th in model.pts_bbox_head.task_heads:
            for name in ('reg', 'height', 'dim', 'rot'):
                getattr(th, name)[-1].weight.mul_(0.05)
            th.dim[-1].bias.fill_(1.0)
    model.pts_bbox_head.test_cfg['use_rotate_nms'] = True
    model.pts_bbox_head.test_cfg['max_num'] = 500
    pc_range = tuple(cfg.model.pts_voxel_layer.point_cloud_range)
    for n_frames in args.frames:
        frames = synthetic.make_batch(n_frames, pc_range=pc_range)
        points, metas = make_views(frames, n_frames, dev, pc_range)
        group, hflip, vflip, _ = model._tta_views(metas)
        with torch.no_grad():
            outs = model.pts_bbox_head(model.extract_feat([p for view in points for p in view], None, None)[1])
        launches = dict(fused=kernels_of(lambda: F.tta_merge_maps(outs, group, hflip, vflip, n_frames)),
                        eager=kernels_of(lambda: model._tta_merge_maps_eager(outs, group, hflip, vflip, n_frames)))
        launches['reference'] = launches['eager']
        forms = dict(fused=lambda: (setattr(type(model), 'TTA_MERGE', True), model.aug_test(points, metas, rescale=True))[1],
                     eager=lambda: (setattr(type(model), 'TTA_MERGE', False), model.aug_test(points, metas, rescale=True))[1],
                     reference=lambda: reference_form(model, points, metas))
        with torch.no_grad():
            for fn in forms.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in forms}
            for _ in range(3):                                  # the forms alternate: three windows each
                for name, fn in forms.items():
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        out = fn()                              # (the results are on the host: every call ends synchronised)
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / args.iters)
        for name in forms:
            best = min(times[name])
            print(json.dumps(dict(frames=n_frames, views=len(VIEWS), form=name, ms_per_call=[round(1e3 * t, 3) for t in times[name]],
                                  frames_per_s=round(n_frames / best, 2), merge_kernels=launches[name],
                                  detections=[len(r['pts_bbox']['scores_3d'] if 'pts_bbox' in r else r['scores_3d']) for r in out])),
                  flush=True)


if __name__ == '__main__':
    main()
