#!/usr/bin/env python
"""The per-frame point stage of the data preparation (tools/create_data_gga.py kitti) two ways, on synthetic frames of real
KITTI size (120 000 points; 4, 8 and 16 objects):

* ``per_call`` (``GGA_PREP_ONE_PASS=0``, the form before ``gga_frame_point_tests``): the image frustum and the box counts of
  ``calculate_num_points_in_gt``, one launch per object frustum as in ``calculate_rga``, the image frustum once more for
  the reduced cloud - each with its own float64 copy, upload and download of the cloud;
* ``one_pass``: ``kitti_converter.prepare_frame_points`` - one upload of the float32 file, one ``gga_frame_point_tests``.

Both are timed in this process, alternating, after a warm-up, with a host clock around work that ends in a download
(uploads and downloads included); their results are compared first. Then the entry point alone (buffers on the device,
device events around ``--iters`` calls) against its byte floor, ``N*stride*4`` read + ``N*ceil(P/32)*4`` + the reduced rows
written, at 8 TB/s; and the whole ``create_kitti_info_file`` in frames/s over a ``--tree-frames`` tree for both forms
(label generation included: region growing dominates it). One JSON line per measurement.

    python tools_dev/bench_data_prep.py [--rounds 30] [--iters 200] [--tree-frames 32] [--tree-points 120000]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM = 8.0e12


def make_frame(n_points, n_obj, seed):
    """An info dict (calib, annos of ``n_obj`` objects in view + one DontCare, image shape) and its cloud [n_points, 4] f32:
    a full turn of the scanner (ground and clutter uniform in azimuth), so that about a fifth of it lies in the image."""
    import numpy as np
    from gga_amd import synthetic
    rng = np.random.default_rng(seed)
    calib = {k: v.copy() for k, v in synthetic.KITTI_CALIB.items()}
    l2c = calib['R0_rect'] @ calib['Tr_velo_to_cam']
    n_g = n_points // 2
    az, r = rng.uniform(-np.pi, np.pi, n_g), rng.uniform(3, 70, n_g)
    pts = [np.stack([r * np.cos(az), r * np.sin(az), -1.72 + rng.normal(0, 0.02, n_g)], 1)]
    names, loc, dims, rot = [], [], [], []
    per_obj = 400
    for i in range(n_obj):
        cx, cy, yaw = rng.uniform(8, 45), rng.uniform(-6, 6), rng.uniform(-np.pi, np.pi)
        l, h, w = 3.9, 1.56, 1.6
        u = np.stack([rng.uniform(-l / 2, l / 2, per_obj), rng.uniform(-w / 2, w / 2, per_obj), rng.uniform(0.1, h, per_obj)], 1)
        c, s = np.cos(yaw), np.sin(yaw)
        pts.append(np.stack([cx + c * u[:, 0] - s * u[:, 1], cy + s * u[:, 0] + c * u[:, 1], -1.72 + u[:, 2]], 1))
        names.append('Car'); loc.append((l2c @ np.array([cx, cy, -1.72, 1.0]))[:3]); dims.append([l, h, w]); rot.append(-yaw - np.pi / 2)
    rest = n_points - n_g - n_obj * per_obj
    az, r = rng.uniform(-np.pi, np.pi, rest), rng.uniform(3, 70, rest)
    pts.append(np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-1.5, 1.5, rest)], 1))
    xyz = np.concatenate(pts)[rng.permutation(n_points)]
    points_v = np.concatenate([xyz, rng.uniform(0, 1, (n_points, 1))], 1).astype(np.float32)
    annos = dict(name=np.array(names + ['DontCare']), dimensions=np.concatenate([np.array(dims), -np.ones((1, 3))]),
                 location=np.concatenate([np.array(loc), -1000 * np.ones((1, 3))]), rotation_y=np.array(rot + [-10.0]))
    info = dict(calib=calib, annos=annos, image=dict(image_shape=np.array([375, 1242], np.int32)))
    return info, points_v


def per_call_stage(info, points_v):
    """The stage as ``calculate_num_points_in_gt`` + ``calculate_rga`` + ``_create_reduced_point_cloud`` ask it."""
    import numpy as np
    from gga_amd import kitti_converter as KC
    from gga_amd import label_gen as LG
    from gga_amd.gt_database import points_in_rbbox
    calib, annos, shape = info['calib'], info['annos'], info['image']['image_shape']
    rect, Trv2c, P2 = calib['R0_rect'], calib['Tr_velo_to_cam'], calib['P2']
    inside = KC.remove_outside_points(points_v, rect, Trv2c, P2, shape)
    boxes, num_obj = KC._gt_boxes_lidar(info)
    counts = points_in_rbbox(inside[:, :3], boxes).sum(0)
    annos['num_points_in_gt'] = np.concatenate([counts, -np.ones([len(annos['dimensions']) - num_obj])]).astype(np.int32)
    boxes_img = LG.box2d_labels(annos, P2, KC._image_shape(info))[0]
    points_lidar = np.concatenate([points_v[..., :3], np.ones([len(points_v), 1])], axis=-1)
    frusta = [LG.points_in_frustm_indices(points_lidar, rect, Trv2c, P2, b).squeeze() for b in boxes_img]
    reduced = KC.remove_outside_points(points_v, rect, Trv2c, P2, shape)
    return frusta, reduced


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 3), p10=round(xs[len(xs) // 10], 3), p90=round(xs[(9 * len(xs)) // 10], 3))


def main():
    import numpy as np
    import torch
    from gga_amd import _lib, synthetic
    from gga_amd import functional as F
    from gga_amd import kitti_converter as KC
    from gga_amd import label_gen as LG
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--tree-frames', type=int, default=32)
    ap.add_argument('--tree-points', type=int, default=120000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    ms = lambda f: (torch.cuda.synchronize(), time.perf_counter(), f(), torch.cuda.synchronize(), time.perf_counter())

    for n_obj in (4, 8, 16):
        info, pts = make_frame(args.points, n_obj, seed=100 + n_obj)
        fa, ra = per_call_stage(info, pts)
        na = info['annos']['num_points_in_gt'].copy()
        fb, rb = KC.prepare_frame_points(info, pts)
        assert np.array_equal(na, info['annos']['num_points_in_gt']) and ra.tobytes() == rb.tobytes()
        assert all(np.array_equal(x, y) for x, y in zip(fa, fb)) and len(fa) == len(fb) == n_obj
        for _ in range(3):
            per_call_stage(info, pts), KC.prepare_frame_points(info, pts)
        ta, tb = [], []
        for _ in range(args.rounds):                # alternating, each ending in a download
            r = ms(lambda: per_call_stage(info, pts)); ta.append(1e3 * (r[4] - r[1]))
            r = ms(lambda: KC.prepare_frame_points(info, pts)); tb.append(1e3 * (r[4] - r[1]))
        # the entry point alone, against its byte floor
        surf = [KC._image_frustum(info), KC.rbbox_surfaces(KC._gt_boxes_lidar(info)[0])]
        surf += [LG.frustum_surfaces(info['calib']['R0_rect'], info['calib']['Tr_velo_to_cam'], info['calib']['P2'], b)
                 for b in LG.box2d_labels(info['annos'], info['calib']['P2'], (375, 1242))[0]]
        equ = [LG.surface_equ_3d(g[:, :, :3, :]) for g in surf]
        normal = torch.from_numpy(np.concatenate([e[0] for e in equ]).astype(np.float64)).to(dev)
        d = torch.from_numpy(np.concatenate([e[1] for e in equ]).astype(np.float64)).to(dev)
        P, n, stride = normal.shape[0], len(pts), pts.shape[1]
        words = (P + 31) // 32
        t_pts = torch.from_numpy(pts).to(dev)
        member = torch.empty((words, n), dtype=torch.int32, device=dev)
        counts, counts_r, n_red = (torch.empty(k, dtype=torch.int32, device=dev) for k in (P, P, 1))
        reduced = torch.empty((n, stride), dtype=torch.float32, device=dev)
        L = _lib.lib()
        ws = torch.empty(L.gga_frame_point_tests_workspace_bytes(n), dtype=torch.uint8, device=dev)
        call = lambda: _lib.check(L.gga_frame_point_tests(F._p(t_pts), n, stride, F._p(normal), F._p(d), P, 6, 0, F._p(member), F._p(counts),
                                                          F._p(counts_r), F._p(reduced), F._p(n_red), F._p(ws), ws.numel(), F._stream()),
                                  'gga_frame_point_tests')
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                call()
            b.record()
            torch.cuda.synchronize()
            rounds.append(1e3 * a.elapsed_time(b) / args.iters)
        k = int(n_red.item())
        nbytes = n * stride * 4 + n * words * 4 + k * stride * 4
        a_med, b_med = statistics.median(ta), statistics.median(tb)
        print(json.dumps(dict(measure='point_stage', points=n, objects=n_obj, polyhedra=P, per_call_ms=spread(ta), one_pass_ms=spread(tb),
                              ratio_per_call_over_one_pass=round(a_med / b_med, 2),
                              per_call_uploads=3 + n_obj, per_call_upload_MB=round((2 * n + k + n_obj * n) * 24 / 1e6, 2),
                              one_pass_upload_MB=round(n * stride * 4 / 1e6, 2),
                              one_pass_download_MB=round((n * words * 4 + k * stride * 4) / 1e6, 2),
                              entry_us=round(statistics.median(rounds), 2), entry_us_rounds=[round(r, 2) for r in rounds],
                              floor_us=round(1e6 * nbytes / HBM, 3), n_reduced=k)), flush=True)

    # the whole info-file step, label generation included, on a raw tree
    n_train = args.tree_frames * 3 // 4
    for form in ('per_call', 'one_pass', 'per_call', 'one_pass'):
        os.environ['GGA_PREP_ONE_PASS'] = '0' if form == 'per_call' else '1'
        with tempfile.TemporaryDirectory() as root:
            synthetic.write_kitti_raw_tree(root, n_train, args.tree_frames - n_train, 0, seed=7100, n_points=args.tree_points)
            torch.cuda.synchronize()
            t = time.perf_counter()
            KC.create_kitti_info_file(root, 'kitti', seed=0, logger=lambda s: None)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
        print(json.dumps(dict(measure='create_kitti_info_file', form=form, frames=args.tree_frames, points_per_frame=args.tree_points,
                              seconds=round(dt, 2), frames_per_s=round(args.tree_frames / dt, 2))), flush=True)


if __name__ == '__main__':
    main()
