#!/usr/bin/env python
"""The image batch of configs/gga/gga_pdg.py (12 KITTI-sized frames -> [12, 3, 384, 1248] float32) two ways:

* ``host``: what a batch costs when the loader normalises and pads on the CPU (``GGA_MONO_IMAGE_DEVICE=0``): the host
  arithmetic of 12 frames (one thread; the loader spreads it over its workers), and the upload of the 69 MB float32 batch;
* ``device``: the 17 MB uint8 buffer packed on the host, its upload, and ``gga_image_batch`` (``image_pipelines.image_batch``).

Cases: 1:1 (every KITTI frame; the whole test pipeline), a resize (frames of 370 x 1224 scaled to 375 x 1241), both storage
orders. Times are device events around ``--iters`` back-to-back calls after a warm-up (kernel alone: the buffer already on
the device) and a host clock around work that ends in a synchronise (end to end). The kernel's floor is its bytes over the
achievable HBM rate: out 4 B + in <= 4 x 1 B per element at 6.3 TB/s. Prints one JSON line per case.

    python tools_dev/bench_image_batch.py [--batch 12] [--iters 200]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM = 6.3e12


def main():
    import numpy as np
    import torch
    from gga_amd import _lib
    from gga_amd import functional as F
    from gga_amd.image_pipelines import DeferredImage, PackedImages, image_batch, normalize_table
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=12)
    ap.add_argument('--iters', type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    table = normalize_table([103.530, 116.280, 123.675], [1.0, 1.0, 1.0])
    rng = np.random.default_rng(0)

    def make(src_hw, dst_hw, flips):
        images = []
        for k in range(args.batch):
            d = DeferredImage(rng.integers(0, 256, src_hw + (3,), dtype=np.uint8))
            d.dst_h, d.dst_w, d.flip, d.table, d.reverse = dst_hw[0], dst_hw[1], bool(flips and k % 2), table, False
            d.pad_h, d.pad_w = -(-dst_hw[0] // 32) * 32, -(-dst_hw[1] // 32) * 32
            images.append(d)
        return images

    for name, src_hw, dst_hw, flips in (('same_size', (375, 1242), (375, 1242), False), ('same_size_half_flipped', (375, 1242), (375, 1242), True),
                                        ('resize', (370, 1224), (375, 1241), True)):
        images = make(src_hw, dst_hw, flips)
        t = time.perf_counter()
        packed = PackedImages(images)
        pack_ms = 1e3 * (time.perf_counter() - t)
        t = time.perf_counter()
        host = torch.from_numpy(np.stack([d.materialize() for d in images]))
        host_ms = 1e3 * (time.perf_counter() - t)
        n, hp, wp = len(packed), images[0].pad_h, images[0].pad_w
        for channels_last in (False, True):
            got = image_batch(packed, dev, channels_last)
            assert torch.equal(got.cpu().contiguous().view(torch.int32), host.view(torch.int32)), 'device and host batches differ'
            # kernel alone
            descs = (_lib.ImageDesc * n)()
            for k, (at, sh, sw, dh, dw, flip, _, _) in enumerate(packed.records):
                descs[k].src_offset, descs[k].src_h, descs[k].src_w, descs[k].dst_h, descs[k].dst_w, descs[k].flip = at, sh, sw, dh, dw, flip
            src = packed.buffer.to(dev)
            out = torch.empty_like(got)
            layout = F.LAYOUT_NHWC if channels_last else F.LAYOUT_NCHW
            call = lambda: _lib.check(_lib.lib().gga_image_batch(src.data_ptr(), src.numel(), descs, n, src.data_ptr(), 0, hp, wp, layout,
                                                                 out.data_ptr(), F._stream()), 'gga_image_batch')
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
            kernel_us = statistics.median(rounds)
            out_bytes, in_bytes = out.numel() * 4, n * src_hw[0] * src_hw[1] * 3 * (1 if src_hw == dst_hw else 4)
            # end to end: upload + launch, and the host path's upload of the float32 batch
            e2e, up = [], []
            pinned = host.pin_memory()
            for i in range(12):
                torch.cuda.synchronize()
                t = time.perf_counter()
                image_batch(packed, dev, channels_last)
                torch.cuda.synchronize()
                e2e.append(1e3 * (time.perf_counter() - t))
                t = time.perf_counter()
                (host if i % 2 else pinned).to(dev, non_blocking=True)
                torch.cuda.synchronize()
                up.append(1e3 * (time.perf_counter() - t))
            print(json.dumps(dict(case=name, layout='NHWC' if channels_last else 'NCHW', batch=n, out=[n, 3, hp, wp], out_MB=out_bytes / 1e6,
                                  src_MB=packed.buffer.numel() / 1e6, kernel_us=round(kernel_us, 2), kernel_us_rounds=[round(r, 2) for r in rounds],
                                  floor_us=round(1e6 * (out_bytes + in_bytes) / HBM, 2), achieved_TBps=round((out_bytes + in_bytes) / kernel_us / 1e6, 3),
                                  device_path_ms=round(statistics.median(e2e[2:]), 3), host_pack_ms=round(pack_ms, 2),
                                  host_arithmetic_ms_one_thread=round(host_ms, 1),
                                  upload_f32_pageable_ms=round(statistics.median(up[3::2]), 3), upload_f32_pinned_ms=round(statistics.median(up[2::2]), 3))),
                  flush=True)


if __name__ == '__main__':
    main()
