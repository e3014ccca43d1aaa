#!/usr/bin/env python
"""The PointNet++ point operators (gga_amd/pointnet2.py) at the shapes of the reference's
configs/votenet/votenet_16x8_sunrgbd-3d-10class.py: 16 frames of 20 000 points, set abstraction levels of 2048 / 1024 / 512 / 256
centres with radii 0.2 / 0.4 / 0.8 / 1.2 and 64 / 32 / 16 / 16 samples over 1 / 128 / 256 / 256 feature channels, two feature
propagation levels (512 <- 256 and 1024 <- 512 points, 256 channels), and the vote aggregation (256 proposals, radius 0.3, 16
samples of 1024 seeds, 256 channels).

Measured: every op on its own, and QueryAndGroup as one launch against the composition of the separate ops
(``GGA_SA_GROUP_FUSED=0``), forward and forward + backward. Protocol: device events around each call on the current stream,
synchronised; ``--warmup`` untimed calls of every variant first, then ``--reps`` timed ones with the variants of a comparison
alternating inside one run; the median and the spread (min .. max) in milliseconds. Points: half on the floor and two walls of
a 5 x 5 x 2.5 m room, half anywhere in it, from a seed. Needs the GPU: there is no fallback.

Sections (``--sections``, default all three): ``ops`` = the above; ``pool`` = ``pointnet2.group_max_pool`` against ``F.max_pool2d``
at the five pool shapes of the config (the four levels and the vote aggregation) in contiguous and channels-last memory, forward
and forward + backward, with the achieved fraction of the HBM peak; ``modules`` = the first set abstraction level and the whole
``PointNet2SASSG`` backbone, forward + backward, with ``GGA_SA_POOL`` 1 and 0.

    python tools_dev/bench_votenet.py [--reps 30] [--warmup 5] [--batch 16] [--sections ops,pool,modules] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as tF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gga_amd import pointnet2 as P  # noqa: E402

SA = [(2048, 0.2, 64, 1), (1024, 0.4, 32, 128), (512, 0.8, 16, 256), (256, 1.2, 16, 256)]      # centres, radius, samples, channels in
FP = [(512, 256, 256), (1024, 512, 256)]                                                           # target n, source m, channels
VOTE = (256, 0.3, 16, 256)
POOL = [(128, 2048, 64), (256, 1024, 32), (256, 512, 16), (256, 256, 16), (128, 256, 16)]        # C, M, K: SA1-4, vote aggregation
HBM_PEAK_TB_S = 8.0
BACKBONE = dict(type='PointNet2SASSG', in_channels=4, num_points=(2048, 1024, 512, 256), radius=(0.2, 0.4, 0.8, 1.2),
                num_samples=(64, 32, 16, 16), sa_channels=((64, 64, 128), (128, 128, 256), (128, 128, 256), (128, 128, 256)),
                fp_channels=((256, 256), (256, 256)), norm_cfg=dict(type='BN2d'),
                sa_cfg=dict(type='PointSAModule', pool_mod='max', use_xyz=True, normalize_xyz=True))


def room(rng, batch, n):
    pts = rng.uniform([0, 0, 0], [5, 5, 2.5], (batch, n, 3))
    kind = rng.integers(0, 6, (batch, n))
    pts[..., 2] = np.where(kind == 0, 0.0, pts[..., 2])
    pts[..., 0] = np.where(kind == 1, 0.0, pts[..., 0])
    pts[..., 1] = np.where(kind == 2, 5.0, pts[..., 1])
    return (pts + rng.normal(0, 0.005, pts.shape)).astype(np.float32)


def timed(variants, warmup, reps):
    """variants: {name: callable}. -> {name: (median, min, max)} ms; the variants alternate within every repetition."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--json', default=None)
    ap.add_argument('--sections', default='ops,pool,modules', help='comma-separated: ops, pool, modules')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_votenet.py measures on the GPU only'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    B = args.batch
    rows = []

    def report(name, res):
        for variant, (med, lo, hi) in res.items():
            rows.append(dict(op=name, variant=variant, ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4)))
            print(f'{name:44s} {variant:22s} {med:9.4f} ms  ({lo:.4f} .. {hi:.4f})', flush=True)

    def run(name, **variants):
        report(name, timed(variants, args.warmup, args.reps))

    xyz = torch.from_numpy(room(rng, B, args.points)).to(dev)
    sections = args.sections.split(',')
    assert set(sections) <= {'ops', 'pool', 'modules'}, args.sections
    if 'ops' in sections:
        bench_ops(args, run, rng, xyz)
    if 'pool' in sections:
        bench_pool(args, run, rows)
    if 'modules' in sections:
        bench_modules(args, run, xyz)
    write_json(args, rows)


def bench_ops(args, run, rng, xyz):
    dev, B = xyz.device, args.batch
    feats = torch.randn(B, 1, args.points, device=dev)
    levels = []                                             # (xyz, features) going into each set abstraction level
    for M, radius, K, C in SA:
        N = xyz.shape[1]
        run(f'furthest_point_sample {N}->{M}', register=lambda: P.furthest_point_sample(xyz, M))
        if N <= 2048:
            was = P.FPS_GENERAL

            def general():
                P.FPS_GENERAL = True
                try:
                    return P.furthest_point_sample(xyz, M)
                finally:
                    P.FPS_GENERAL = was
            run(f'furthest_point_sample {N}->{M}', general=general)
        fps = P.furthest_point_sample(xyz, M)
        xyz_t = xyz.transpose(1, 2).contiguous()
        run(f'gather_points [3,{N}]->{M}', fwd=lambda: P.gather_points(xyz_t, fps))
        centre = P.gather_points(xyz_t, fps).transpose(1, 2).contiguous()
        run(f'ball_query N={N} M={M} r={radius} K={K}', fwd=lambda: P.ball_query(0, radius, K, xyz, centre))
        idx = P.ball_query(0, radius, K, xyz, centre)
        run(f'grouping_operation C={C} N={N} M={M} K={K}', fwd=lambda: P.grouping_operation(feats, idx))
        levels.append((f'SA{len(levels) + 1}', xyz, centre, feats, radius, K))
        xyz, feats = centre, torch.randn(B, SA[len(levels)][3] if len(levels) < len(SA) else 256, M, device=dev)
    seeds = levels[1][2]                                    # 1024 points
    M, radius, K, C = VOTE
    votes = seeds + torch.randn_like(seeds) * 0.1
    centre = P.gather_points(votes.transpose(1, 2).contiguous(), P.furthest_point_sample(votes, M)).transpose(1, 2).contiguous()
    levels.append(('vote aggregation', votes, centre, torch.randn(B, C, votes.shape[1], device=dev), radius, K))

    for n, m, C in FP:
        target, source = torch.from_numpy(room(rng, B, n)).to(dev), torch.from_numpy(room(rng, B, m)).to(dev)
        run(f'three_nn n={n} m={m}', fwd=lambda: P.three_nn(target, source))
        dist, idx = P.three_nn(target, source)
        w = 1.0 / (dist + 1e-8)
        w = w / w.sum(2, keepdim=True)
        f = torch.randn(B, C, m, device=dev, requires_grad=True)
        run(f'three_interpolate C={C} n={n} m={m}', fwd=lambda: P.three_interpolate(f.detach(), idx, w))
        g = torch.randn(B, C, n, device=dev)
        run(f'three_interpolate C={C} n={n} m={m}', fwd_bwd=lambda: P.three_interpolate(f, idx, w).backward(g))

    for name, p, c, f, radius, K in levels:
        N, M, C = p.shape[1], c.shape[1], f.shape[1]
        tag = f'QueryAndGroup {name} N={N} M={M} K={K} C={C}'
        p, c, f = (t.detach().clone().requires_grad_(True) for t in (p, c, f))
        g = torch.randn(B, 3 + C, M, K, device=dev)

        def fwd(fused):
            with torch.no_grad():
                return P.query_and_group(p, c, f, 0, radius, K, True, True, fused=fused)

        def fwd_bwd(fused):
            p.grad = c.grad = f.grad = None
            P.query_and_group(p, c, f, 0, radius, K, True, True, fused=fused)[0].backward(g)
        a, b = fwd(True), fwd(False)
        assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]), f'{tag}: fused and composed forward differ'
        run(tag + ' fwd', fused=lambda: fwd(True), composed=lambda: fwd(False))
        run(tag + ' fwd+bwd', fused=lambda: fwd_bwd(True), composed=lambda: fwd_bwd(False))

def bench_pool(args, run, rows):
    """The group max pool against F.max_pool2d at the five pool shapes of the VoteNet config, in both memory layouts; the rate
    is the kernel's own traffic (4*B*C*M*K + 5*B*C*M bytes each way) over the median, as a fraction of the 8 TB/s HBM peak
    (about 6.3 TB/s is what a float4 copy reaches on this part)."""
    dev = torch.device('cuda:0')
    eager = lambda t: tF.max_pool2d(t, kernel_size=[1, t.shape[3]]).squeeze(-1).contiguous()      # noqa: E731
    for C, M, K in POOL:
        for layout, fmt in (('nchw', torch.contiguous_format), ('channels_last', torch.channels_last)):
            x = torch.randn(args.batch, C, M, K, device=dev).contiguous(memory_format=fmt).requires_grad_(True)
            g = torch.randn(args.batch, C, M, device=dev)
            assert torch.equal(P.group_max_pool(x), eager(x))

            def fwd(fn):
                with torch.no_grad():
                    return fn(x)

            def fwd_bwd(fn):
                x.grad = None
                fn(x).backward(g)
            tag = f'group_max_pool [{args.batch},{C},{M},{K}] {layout}'
            nbytes = 4 * x.numel() + 5 * g.numel()
            for name, fn, passes in (('fwd', fwd, 1), ('fwd+bwd', fwd_bwd, 2)):
                first = len(rows)
                run(f'{tag} {name}', kernel=lambda: fn(P.group_max_pool), max_pool2d=lambda: fn(eager))
                for r in rows[first:]:
                    r['tb_per_s'] = round(passes * nbytes / (r['ms'] * 1e-3) / 1e12, 3)
                    r['of_hbm_peak'] = round(r['tb_per_s'] / HBM_PEAK_TB_S, 3)
                    print(f'    {r["variant"]:12s} {r["tb_per_s"]:.3f} TB/s of the kernel\'s own traffic = {r["of_hbm_peak"]:.3f} of '
                          f'{HBM_PEAK_TB_S} TB/s', flush=True)
            del x, g
            torch.cuda.empty_cache()


def bench_modules(args, run, xyz):
    """The first set abstraction level and the whole backbone of the VoteNet config, forward + backward, with the pool kernel
    (GGA_SA_POOL=1) and with F.max_pool2d (GGA_SA_POOL=0)."""
    from gga_amd.pointnet_modules import PointSAModule
    from gga_amd.registry import build_backbone
    dev = xyz.device
    torch.manual_seed(0)
    M, radius, K, _ = SA[0]
    sa = PointSAModule(mlp_channels=[1, 64, 64, 128], num_point=M, radius=radius, num_sample=K, normalize_xyz=True).to(dev).train()
    feats = torch.randn(xyz.shape[0], 1, xyz.shape[1], device=dev, requires_grad=True)
    g = torch.randn(xyz.shape[0], 128, M, device=dev)
    backbone = build_backbone(BACKBONE).to(dev).train()
    points = torch.cat([xyz, torch.randn(xyz.shape[0], xyz.shape[1], 1, device=dev)], dim=2).requires_grad_(True)
    gb = torch.randn(xyz.shape[0], 256, SA[1][0], device=dev)
    was = P.SA_POOL

    def level(own):
        P.SA_POOL = own
        feats.grad = None
        sa.zero_grad(set_to_none=True)
        sa(xyz, feats)[1].backward(g)

    def whole(own):
        P.SA_POOL = own
        points.grad = None
        backbone.zero_grad(set_to_none=True)
        backbone(points)['fp_features'][-1].backward(gb)
    try:
        run(f'PointSAModule SA1 N={xyz.shape[1]} M={M} K={K} fwd+bwd', pool_kernel=lambda: level(True), max_pool2d=lambda: level(False))
        run(f'PointNet2SASSG N={xyz.shape[1]} fwd+bwd', pool_kernel=lambda: whole(True), max_pool2d=lambda: whole(False))
    finally:
        P.SA_POOL = was


def write_json(args, rows):
    if args.json:
        with open(args.json, 'w') as fh:
            for r in rows:
                fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
