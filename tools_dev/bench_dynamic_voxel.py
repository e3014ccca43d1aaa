#!/usr/bin/env python
"""Measurements of the dynamic-voxelization front (EXPERIMENTS.md, "Dynamic voxelization"): 16 frames x 20 000 synthetic
points on the PointPillars grid, one device.

    python tools_dev/bench_dynamic_voxel.py encoders        # device time of forward + backward: fused / eager / plain torch
    python tools_dev/bench_dynamic_voxel.py front           # the dynamic and the hard front once each per iteration (for a
                                                            # kernel trace: run under `rocprofv3 --kernel-trace --stats`)
    python tools_dev/bench_dynamic_voxel.py steps           # train-step time of the dv-PointPillars config beside the hard one
Each mode prints one JSON line."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, N = 16, 20000
VS, RNG = [0.16, 0.16, 4], [0, -39.68, -3, 69.12, 39.68, 1]
CFG = {'hard': 'gga_kitti_pointpillars_config.py', 'dynamic': 'gga_kitti_dv_pointpillars_config.py'}


def frames(device):
    from gga_amd import synthetic
    b = synthetic.make_batch(B, n_points=N, pc_range=tuple(RNG))
    return [p.to(device).float().contiguous() for p in b['points']]


def device_ms(fn, warm=5, reps=20):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(times), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4))


def encoder(fused):
    import torch
    from gga_amd import voxel_encoders as VE
    from gga_amd.registry import VOXEL_ENCODERS
    VE.DYNAMIC_PFN_FUSED = fused
    torch.manual_seed(0)
    return VOXEL_ENCODERS.build(dict(type='DynamicPillarFeatureNet', in_channels=4, feat_channels=[64], voxel_size=VS,
                                     point_cloud_range=RNG)).cuda().train()


def plain_torch_step(m, pts, coors):
    """The test restatement moved to the device: torch.unique + index_reduce, framework Linear / BatchNorm."""
    import torch
    keep = (coors[:, 1:] >= 0).all(1)
    pts, coors = pts[keep], coors[keep].long()
    vc, inv, cnt = torch.unique(coors, dim=0, return_inverse=True, return_counts=True)
    mean = torch.zeros((vc.shape[0], 3), device=pts.device).index_add_(0, inv, pts[:, :3]) / cnt[:, None]
    c = coors.float()
    centre = torch.stack([c[:, 3] * m.vx + m.x_offset, c[:, 2] * m.vy + m.y_offset, c[:, 1] * m.vz + m.z_offset], 1)
    f = torch.cat([pts, pts[:, :3] - mean[inv], pts[:, :3] - centre], 1)
    y = m.pfn_layers[0](f)
    out = torch.zeros((vc.shape[0], y.shape[1]), device=y.device).index_reduce(0, inv, y, 'amax', include_self=False)
    return out


def mode_encoders():
    import torch
    from gga_amd import voxel_encoders as VE
    from gga_amd.voxel_layer import Voxelization
    layer = Voxelization(voxel_size=VS, point_cloud_range=RNG, max_num_points=-1, max_voxels=(-1, -1))
    fr = frames('cuda')
    cat, coors = layer.forward_batch(fr)
    vm = coors.voxel_map
    m_vox, kept = vm.host_counts()
    pop = (vm.voxel_start[1:m_vox + 1] - vm.voxel_start[:m_vox]).float()
    out = dict(mode='encoders', frames=B, points=int(cat.shape[0]), kept=kept, voxels=m_vox,
               points_per_voxel=dict(median=float(pop.median()), mean=round(float(pop.mean()), 2), max=int(pop.max())))

    def step(m, fwd):
        def run():
            for p in m.parameters():
                p.grad = None
            y = fwd()
            y.backward(torch.ones_like(y))
        return run

    out['map_ms'] = device_ms(lambda: layer.forward_batch(fr))
    mf = encoder(True)
    out['fused_capacity'] = device_ms(step(mf, lambda: mf(cat, coors, capacity=True)[0]))
    out['fused_exact_rows'] = device_ms(step(mf, lambda: mf(cat, coors)[0]))
    me = encoder(False)
    out['eager'] = device_ms(step(me, lambda: me(cat, coors)[0]))
    VE.DYNAMIC_PFN_FUSED = True
    mt = encoder(False)
    out['plain_torch'] = device_ms(step(mt, lambda: plain_torch_step(mt, cat, coors)))
    print(json.dumps(out))


def mode_front():
    import torch
    from gga_amd.registry import VOXEL_ENCODERS
    from gga_amd.voxel_layer import Voxelization
    fr = frames('cuda')
    dyn = Voxelization(voxel_size=VS, point_cloud_range=RNG, max_num_points=-1, max_voxels=(-1, -1))
    hard = Voxelization(voxel_size=VS, point_cloud_range=RNG, max_num_points=32, max_voxels=(16000, 40000)).train()
    md = encoder(True)
    torch.manual_seed(0)
    mh = VOXEL_ENCODERS.build(dict(type='PillarFeatureNet', in_channels=4, feat_channels=[64], voxel_size=VS,
                                   point_cloud_range=RNG)).cuda().train()
    for _ in range(8):
        cat, coors = dyn.forward_batch(fr)
        y = md(cat, coors, capacity=True)[0]
        y.backward(torch.ones_like(y))
        voxels, npts, hc, _ = hard.forward_batch(fr, sync=False)
        z = mh(voxels, npts, hc)
        z.backward(torch.ones_like(z))
    torch.cuda.synchronize()
    print(json.dumps(dict(mode='front', iterations=8, frames=B, points=int(cat.shape[0]))))


def mode_steps():
    import argparse
    import torch
    import bench
    torch.set_num_threads(1)            # the process setup of bench.py's headline: one math thread
    args = argparse.Namespace(nchw=False, head_init_scale=0.05)
    out = dict(mode='steps', frames=B, warmup=5, steps=20)
    for name, cfg in CFG.items():
        path = os.path.join(REPO, 'configs', 'gga', cfg)
        times = []
        for rep in range(3):
            r = bench.run_workload(path, B, 20, 5, args, 0, 1, torch.device('cuda:0'))
            times.append(r['dt'] / 20 * 1e3)
            del r
            torch.cuda.empty_cache()
        out[name] = dict(ms_per_step_median=round(statistics.median(times), 3), runs=[round(t, 3) for t in times])
    print(json.dumps(out))


if __name__ == '__main__':
    {'encoders': mode_encoders, 'front': mode_front, 'steps': mode_steps}[sys.argv[1]]()
