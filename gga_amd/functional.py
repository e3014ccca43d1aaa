"""Torch-facing wrappers over the C ABI (include/gga_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator), the current
HIP stream and autograd bookkeeping. Every op enqueues hand-written gfx950 kernels
from ``libgga_hip.so`` on ``torch.cuda.current_stream()`` through ctypes with raw
device pointers; nothing falls back to eager PyTorch or the CPU.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import LossParams, PfnParams, VoxelParams, check
import contextlib
import os

_DEFERRED_COUNTERS = None       # a list while a forward pass collects the BatchNorm counters it would increment


def count_batch(bn):
    """``num_batches_tracked += 1`` of a BatchNorm layer in training mode (torch/nn/modules/batchnorm.py,
    _BatchNorm.forward; the fused paths here all require ``momentum is not None``, so the counter is bookkeeping,
    not an input of the step). Inside :func:`deferred_batch_counters` the counters are only collected."""
    if _DEFERRED_COUNTERS is not None:
        _DEFERRED_COUNTERS.append(bn.num_batches_tracked)
    else:
        bn.num_batches_tracked += 1


@contextlib.contextmanager
def deferred_batch_counters():
    """One multi-tensor add for all the BatchNorm counters of a forward pass instead of one one-element kernel per
    layer (36 per PointPillars step). A layer applied several times is counted that many times."""
    global _DEFERRED_COUNTERS
    prev, _DEFERRED_COUNTERS = _DEFERRED_COUNTERS, []
    try:
        yield
    except BaseException:
        _DEFERRED_COUNTERS = prev          # a pass that raised updated no running statistics for certain: count nothing
        raise
    seen, _DEFERRED_COUNTERS = _DEFERRED_COUNTERS, prev
    if seen:
        uniq = {}
        for t in seen:
            uniq.setdefault(id(t), [t, 0])[1] += 1
        torch._foreach_add_([t for t, _ in uniq.values()], [n for _, n in uniq.values()])

LAYOUT_NCHW, LAYOUT_NHWC = 0, 1

_workspaces = {}
_cell_maps = {}


def _stream():
    # raw handle of the current stream of the current device (what torch.cuda.current_stream().cuda_stream returns,
    # without building a Stream object: ~800 calls per train step)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stamp(t):
    """What side data attached to ``t`` by its producer (per-channel sums, absmax, ``BnSource``, ``BnPartials``) is keyed
    by: it changes when ``t`` is written again or is made to stand for other memory."""
    return (t._version, t.data_ptr(), t.numel())


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('gga_amd ops run on the GPU only (got a CPU tensor); '
                               'there is no CPU fallback in the product path')


def _workspace(key, nbytes, device):
    """Grow-only scratch buffer per (purpose, device, stream)."""
    k = (key, device, torch.cuda.current_stream().cuda_stream)
    w = _workspaces.get(k)
    if w is None or w.numel() < nbytes:
        w = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _workspaces[k] = w
    return w


# ----------------------------------------------------------------------------- a1/a2
def voxel_params(voxel_size, point_cloud_range, max_points, max_voxels):
    prm = VoxelParams()
    prm.voxel_size[:] = [float(v) for v in voxel_size]
    prm.pc_range[:] = [float(v) for v in point_cloud_range]
    prm.max_points, prm.max_voxels = int(max_points), int(max_voxels)
    return prm


def voxel_grid_size(prm):
    g = (C.c_int32 * 3)()
    _lib.lib().gga_voxel_grid_size(C.byref(prm), C.byref(g))
    return list(g)


@torch.no_grad()
def _hard_voxelize(points, offsets, counts, voxel_size, point_cloud_range, max_points, max_voxels, sync):
    """``gga_hard_voxelize_batch`` on frames concatenated in ``points`` at the int64 row ``offsets``; ``counts``: None, or the
    device-side point counts of frames stored at capacity offsets."""
    B, ndim, dev = len(offsets) - 1, points.shape[1], points.device
    prm = voxel_params(voxel_size, point_cloud_range, max_points, max_voxels)
    cap = B * int(max_voxels)
    voxels = torch.empty((cap, int(max_points), ndim), dtype=torch.float32, device=dev)
    coors = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    num_points = torch.empty((cap,), dtype=torch.int32, device=dev)
    voxel_num = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = _workspace('vox', L.gga_hard_voxelize_workspace_bytes(B, int(offsets[-1])), dev)
    check(L.gga_hard_voxelize_batch(_p(points), ndim, offsets.ctypes.data_as(C.POINTER(C.c_int64)), _p(counts), B,
                                    C.byref(prm), _p(voxels), _p(coors), _p(num_points), _p(voxel_num),
                                    _p(ws), ws.numel(), _stream()), 'gga_hard_voxelize_batch')
    if sync:
        m = int(voxel_num[-1].item())
        return voxels[:m], num_points[:m], coors[:m], voxel_num
    coors.num_valid = voxel_num[B:]           # device count travels with the coordinates (see num_valid_of)
    return voxels, num_points, coors, voxel_num


@torch.no_grad()
def hard_voxelize_batch(points, voxel_size, point_cloud_range, max_points, max_voxels, sync=True):
    """Batched hard voxelization (mvx_two_stage_gga.py:211-236 in one call).

    points: list of [N_b, C] f32 CUDA tensors. Returns ``voxels [M,P,C]``,
    ``num_points [M]``, ``coors [M,4] (b,z,y,x)``, ``voxel_num [B+1]`` (device).
    With ``sync=True`` the outputs are trimmed to the exact M (one 4-byte D2H read, the
    reference syncs once per frame); with ``sync=False`` they keep the capacity
    ``B*max_voxels`` (rows >= M zero) and ``voxel_num[-1]`` carries M on the device.
    """
    _need_cuda(*points)
    offs = np.zeros(len(points) + 1, np.int64)
    offs[1:] = np.cumsum([p.shape[0] for p in points])
    cat = points[0].contiguous() if len(points) == 1 else torch.cat(points, 0)
    if cat.dtype != torch.float32:
        cat = cat.float()
    return _hard_voxelize(cat, offs, None, voxel_size, point_cloud_range, max_points, max_voxels, sync)


def num_valid_of(coors):
    """Device i32 [1] count of the rows that exist in capacity-sized voxel buffers (set by the
    ``sync=False`` voxelizer calls), or None for exact-sized ones."""
    return getattr(coors, 'num_valid', None)


class PreparedPoints:
    """Frames at capacity offsets with device-side counts: the hand-over from
    ``points_prepare_batch`` to ``hard_voxelize_prepared``."""

    def __init__(self, points, capacity_offsets, counts):
        self.points, self.capacity_offsets, self.counts = points, capacity_offsets, counts

    def __len__(self):
        return len(self.capacity_offsets) - 1

    def to_list(self):
        """Per-frame tensors (synchronises: reads the counts back)."""
        n = self.counts.cpu().tolist()
        return [self.points[int(o):int(o) + k] for o, k in zip(self.capacity_offsets[:-1], n)]


def upload(host, device):
    """Host array / CPU tensor -> device without draining the launch queue: a copy from pageable
    memory blocks the host until everything queued before it has run (the loss targets are
    uploaded after the forward pass was queued, so the host lost its lead exactly where the
    many small loss kernels start); staged through the caching pinned allocator the copy is
    just another stream operation."""
    t = torch.from_numpy(host) if isinstance(host, np.ndarray) else host
    dev = torch.device(device)
    if dev.type == 'cuda' and t.device.type == 'cpu' and t.numel():
        t = t.pin_memory()
    return t.to(dev, non_blocking=True)


def upload_many(arrays, device, align=256):
    """Host arrays {name: ndarray} -> {name: device tensor} through ONE pinned staging buffer and ONE copy: every copy on the
    compute stream is ~15-25 us of stream time with the device idle (the head's nine target arrays after the forward pass: 0.46 ms
    per step in a kernel + memory-copy trace, tools_dev/trace_region.py), whatever its size. The tensors are views of one device
    byte buffer (256-byte aligned)."""
    dev = torch.device(device)
    items, total = [], 0
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        items.append((k, a, total))
        total += -(-max(a.nbytes, 1) // align) * align
    stage = torch.empty(total, dtype=torch.uint8, pin_memory=dev.type == 'cuda')
    sv = stage.numpy()
    for k, a, o in items:
        if a.nbytes:
            sv[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    d = stage.to(dev, non_blocking=True)
    out = {}
    for k, a, o in items:
        dt = torch.from_numpy(np.empty(0, a.dtype)).dtype
        out[k] = d[o:o + a.nbytes].view(dt).view(a.shape)
    return out


_CONSTS = {}


def const_tensor(data, device, dtype=torch.float32):
    """Device tensor of a small host constant (nested lists / tuples / a numpy array), uploaded once per (value, device,
    dtype): ``x.new_tensor(list)`` inside the step is a copy from pageable memory, i.e. a host wait for everything queued
    so far (91 of them per PGD step kept the host 40 ms behind). The result is shared: do not write into it."""
    key = (data.tobytes() + str(data.shape).encode() if isinstance(data, np.ndarray) else repr(data), str(device), dtype)
    t = _CONSTS.get(key)
    if t is None:
        if len(_CONSTS) > 4096:
            _CONSTS.clear()
        t = _CONSTS[key] = upload(torch.as_tensor(np.asarray(data), dtype=dtype), device)
        if t.is_cuda:                      # once per constant: it may be read from another stream right away
            torch.cuda.current_stream(t.device).synchronize()
    return t


def _cat_rows(parts, ndim, dev, dtype=torch.float32):
    parts = [torch.as_tensor(p, dtype=dtype).reshape(-1, ndim) for p in parts]
    offs = np.zeros(len(parts) + 1, np.int64)
    offs[1:] = np.cumsum([p.shape[0] for p in parts])
    cat = torch.cat(parts, 0) if parts else torch.zeros((0, ndim), dtype=dtype)
    return cat.to(dev, non_blocking=True).contiguous(), offs


@torch.no_grad()
def points_prepare_batch(scene, sampled, centers, min_distance, point_cloud_range, shuffle_seeds, device):
    """Device-side tail of the point pipeline for a batch (``gga_points_prepare_batch``): per frame
    drop scene points within ``min_distance`` (BEV) of a pasted object's centre, put the pasted
    objects' points in front, apply the strict range filter, permute by seed (0 = keep order).
    scene / sampled: lists of [n, C] f32 (host or device), centers: list of [k, 2] f64.
    -> ``PreparedPoints`` (no synchronisation)."""
    dev = torch.device(device)
    B = len(scene)
    ndim = int(scene[0].shape[1])
    d_scene, o_scene = _cat_rows(scene, ndim, dev)
    d_samp, o_samp = _cat_rows(sampled, ndim, dev)
    d_ctr, o_ctr = _cat_rows([np.asarray(c, np.float64).reshape(-1, 2) for c in centers], 2, dev, torch.float64)
    _need_cuda(d_scene)
    cap = (o_scene + o_samp).astype(np.int64)
    total = int(cap[-1])
    rng = torch.as_tensor(np.asarray(point_cloud_range, np.float32)).to(dev)
    seeds = (C.c_uint64 * B)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in shuffle_seeds])
    out = torch.empty((max(total, 1), ndim), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    L = _lib.lib()
    max_rows = int(np.max(np.diff(cap))) if B else 0
    ws = _workspace('pprep', L.gga_points_prepare_workspace_bytes(B, total, max_rows), dev)
    as64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    with torch.cuda.device(dev):
        check(L.gga_points_prepare_batch(_p(d_scene), as64(o_scene), _p(d_samp), as64(o_samp), _p(d_ctr), as64(o_ctr), B, ndim,
                                         float(min_distance), _p(rng), seeds, _p(out), _p(counts), _p(ws), ws.numel(),
                                         _stream()), 'gga_points_prepare_batch')
    return PreparedPoints(out, cap, counts)


def hard_voxelize_prepared(prep, voxel_size, point_cloud_range, max_points, max_voxels, sync=True):
    """``hard_voxelize_batch`` on a ``PreparedPoints`` (frames at capacity offsets, counts on the device)."""
    _need_cuda(prep.points, prep.counts)
    return _hard_voxelize(prep.points, np.ascontiguousarray(prep.capacity_offsets, np.int64), prep.counts, voxel_size,
                          point_cloud_range, max_points, max_voxels, sync)


@torch.no_grad()
def voxel_mean(voxels, num_points, num_features):
    _need_cuda(voxels, num_points)
    voxels = voxels.contiguous()
    m, P, ndim = voxels.shape
    out = torch.empty((m, num_features), dtype=torch.float32, device=voxels.device)
    if m == 0:
        return out
    num_points = num_points.contiguous()     # keep every converted tensor alive until the launch is enqueued
    check(_lib.lib().gga_voxel_mean(_p(voxels), _p(num_points), m, P, ndim, num_features,
                                    _p(out), _stream()), 'gga_voxel_mean')
    return out



# ----------------------------------------------------------------------------- a2'
class _FusedPFN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, voxels, num_points, coors, weight, gamma, beta, running_mean, running_var, prm, num_valid=None):
        _need_cuda(voxels, num_points, coors, weight)
        voxels, coors = voxels.contiguous(), coors.contiguous()
        m, P, _ = voxels.shape
        dev = voxels.device
        L = _lib.lib()
        out = torch.empty((m, 64), dtype=torch.float32, device=dev)
        argmax = torch.empty((m, 64), dtype=torch.uint8, device=dev)
        saved = torch.empty(_lib.PFN_SAVED_DOUBLES, dtype=torch.float64, device=dev)
        ws = _workspace('pfn', L.gga_pfn_workspace_bytes(m), dev)
        w = weight.contiguous()
        check(L.gga_pfn_fwd(_p(voxels), _p(num_points), _p(coors), m, _p(num_valid), P, C.byref(prm), _p(w), _p(gamma),
                            _p(beta), _p(running_mean), _p(running_var), _p(out), _p(argmax), _p(saved),
                            _p(ws), ws.numel(), _stream()), 'gga_pfn_fwd')
        ctx.save_for_backward(voxels, num_points, coors, w, gamma, out, argmax, saved)
        ctx.prm, ctx.num_valid = prm, num_valid
        return out

    @staticmethod
    def backward(ctx, g):
        voxels, num_points, coors, w, gamma, out, argmax, saved = ctx.saved_tensors
        m, P, _ = voxels.shape
        L = _lib.lib()
        gw, gg, gb = torch.empty_like(w), torch.empty_like(gamma), torch.empty_like(gamma)
        ws = _workspace('pfn', L.gga_pfn_workspace_bytes(m), g.device)
        g = g.contiguous()
        check(L.gga_pfn_bwd(_p(voxels), _p(num_points), _p(coors), m, _p(ctx.num_valid), P, C.byref(ctx.prm), _p(w),
                            _p(gamma), _p(out), _p(argmax), _p(saved), _p(g), _p(gw), _p(gg), _p(gb), _p(ws),
                            ws.numel(), _stream()), 'gga_pfn_bwd')
        return None, None, None, gw, gg, gb, None, None, None, None


def pfn_params(voxel_size, offsets, eps, momentum, training):
    prm = PfnParams()
    prm.voxel_size[:] = [float(v) for v in voxel_size]
    prm.offsets[:] = [float(v) for v in offsets]
    prm.eps, prm.momentum = float(eps), float(momentum)
    prm.training, prm.in_features, prm.channels = int(bool(training)), 4, 64
    return prm


def fused_pfn(voxels, num_points, coors, weight, gamma, beta, running_mean, running_var, prm, num_valid=None):
    """Fused PillarFeatureNet: [M,P,4] -> [M,64] (running stats updated in place when training).
    ``num_valid``: device i32 count of the pillars that exist when the buffers are capacity-sized
    (``hard_voxelize_batch(sync=False)``); the output rows past it are zero."""
    return _FusedPFN.apply(voxels, num_points, coors, weight, gamma, beta, running_mean, running_var, prm, num_valid)


# ----------------------------------------------------------------------------- a3
def _cell_map(device, batch, ny, nx):
    k = (device, batch, ny, nx, torch.cuda.current_stream().cuda_stream)
    m = _cell_maps.get(k)
    if m is None:
        nbytes = _lib.lib().gga_pillar_scatter_map_bytes(batch, ny, nx)
        m = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=device)
        _cell_maps[k] = m
    return m


class _PillarScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, coors, batch, ny, nx, layout, num_valid, unique=False):
        _need_cuda(feats, coors)
        feats = feats.contiguous()
        coors = coors.contiguous()
        if coors.dtype != torch.int32:
            coors = coors.int()
        m, Cc = feats.shape
        if layout == LAYOUT_NCHW:
            canvas = torch.empty((batch, Cc, ny, nx), dtype=torch.float32, device=feats.device)
        else:
            canvas = torch.empty((batch, Cc, ny, nx), dtype=torch.float32, device=feats.device,
                                 memory_format=torch.channels_last)
        # unique coordinates + NHWC need no winner map (fill + row copies)
        cmap = None if (unique and layout == LAYOUT_NHWC) else _cell_map(feats.device, batch, ny, nx)
        check(_lib.lib().gga_pillar_scatter_fwd(_p(feats), _p(coors), m, _p(num_valid), batch, Cc, ny, nx,
                                                layout, int(bool(unique)), _p(cmap), _p(canvas), _stream()),
              'gga_pillar_scatter_fwd')
        ctx.save_for_backward(coors, num_valid)
        ctx.geom = (m, batch, Cc, ny, nx, layout)
        return canvas

    @staticmethod
    def backward(ctx, grad):
        coors, num_valid = ctx.saved_tensors
        m, batch, Cc, ny, nx, layout = ctx.geom
        if layout == LAYOUT_NCHW:
            grad = grad.contiguous()
        else:
            grad = grad.contiguous(memory_format=torch.channels_last)
        gf = torch.empty((m, Cc), dtype=torch.float32, device=grad.device)
        check(_lib.lib().gga_pillar_scatter_bwd(_p(grad), _p(coors), m, _p(num_valid), batch, Cc, ny, nx,
                                                layout, _p(gf), _stream()), 'gga_pillar_scatter_bwd')
        return gf, None, None, None, None, None, None, None


class _SparseBEV(torch.autograd.Function):
    """[n, C] features of distinct sites (b, z, y, x) -> [B, C * D, H, W] in channels-last memory, channel c * D + z
    (gga_sparse_bev_nhwc_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, feats, coors, B, D, H, W):
        _need_cuda(feats, coors)
        feats, coors = feats.contiguous(), coors.contiguous()
        n, C_ = feats.shape
        out = torch.empty((B, H, W, C_ * D), dtype=torch.float32, device=feats.device)
        check(_lib.lib().gga_sparse_bev_nhwc_fwd(_p(feats), _p(coors), n, B, C_, D, H, W, _p(out), _stream()), 'gga_sparse_bev_nhwc_fwd')
        ctx.save_for_backward(coors)
        ctx.geom = (n, B, C_, D, H, W)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        coors, = ctx.saved_tensors
        n, B, C_, D, H, W = ctx.geom
        g = g.contiguous(memory_format=torch.channels_last)
        gf = torch.empty((n, C_), dtype=torch.float32, device=g.device)
        check(_lib.lib().gga_sparse_bev_nhwc_bwd(_p(g), _p(coors), n, B, C_, D, H, W, _p(gf), _stream()), 'gga_sparse_bev_nhwc_bwd')
        return gf, None, None, None, None, None


def sparse_bev_channels_last(feats, coors, batch_size, D, H, W):
    """``SparseConvTensor.dense().view(N, C * D, H, W)`` of middle_encoders/sparse_encoder.py:134-138 as a channels-last tensor,
    without the NCHW map and the two layout copies in between (f32 CUDA features with C % 4 == 0, int32 coors, distinct sites)."""
    return _SparseBEV.apply(feats, coors, int(batch_size), int(D), int(H), int(W))


def pillar_scatter(feats, coors, batch_size, ny, nx, channels_last=False, num_valid=None, unique=False):
    """[M,C] pillar features + coors (b,z,y,x) -> dense [B,C,ny,nx] canvas. ``unique``: the caller
    guarantees distinct (b,y,x) (voxelizer output, sparse sites); otherwise the highest row of a
    duplicated cell wins."""
    canvas = _PillarScatter.apply(feats, coors, int(batch_size), int(ny), int(nx),
                                  LAYOUT_NHWC if channels_last else LAYOUT_NCHW, num_valid, bool(unique))
    if unique and channels_last:
        # lets the consumer's backward work on the pillars instead of the canvas (pillar_conv.py)
        from .pillar_conv import PillarSupport
        canvas.pillar_support = PillarSupport(feats, coors, num_valid)
    return canvas


# ----------------------------------------------------------------------------- a6/a7
_patch_tables = {}


def gaussian_patch_table(max_radius, device):
    """Patches for radius 0..max_radius with the reference's f64 formula
    (mmdet3d/core/utils/gaussian.py:6-22, sigma = diameter / 6), cast to f32."""
    k = (max_radius, device)
    if k not in _patch_tables:
        vals, offs = [], [0]
        for r in range(max_radius + 1):
            d = 2 * r + 1
            sigma = d / 6
            y, x = np.ogrid[-r:r + 1, -r:r + 1]
            h = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
            h[h < np.finfo(h.dtype).eps * h.max()] = 0
            vals.append(h.astype(np.float32).reshape(-1))
            offs.append(offs[-1] + d * d)
        _patch_tables[k] = (torch.from_numpy(np.concatenate(vals)).to(device),
                            torch.tensor(offs, dtype=torch.int32, device=device))
    return _patch_tables[k]


@torch.no_grad()
def heatmap_splat(objs, n_maps, H, W, device, max_radius=64):
    """objs: [n,4] int32 (map index, cx, cy, radius) host or device -> [n_maps,H,W] f32."""
    hm = torch.empty((n_maps, H, W), dtype=torch.float32, device=device)
    objs = torch.as_tensor(objs, dtype=torch.int32).reshape(-1, 4)
    if not objs.is_cuda and objs.numel() and int(objs[:, 3].max()) > max_radius:       # (a device tensor: the caller vouches for max_radius)
        max_radius = int(objs[:, 3].max())
    table, offs = gaussian_patch_table(max_radius, device)
    objs = upload(objs.contiguous(), device)
    check(_lib.lib().gga_heatmap_splat(_p(hm), n_maps, H, W, _p(objs), objs.shape[0], _p(table), _p(offs),
                                       max_radius, _stream()), 'gga_heatmap_splat')
    return hm


# ----------------------------------------------------------------------------- a8
def _task_table(n):
    """An empty gga_task_table for ``n`` tasks; the caller fills the fields its stage reads (pointers as ints)."""
    if not 1 <= n <= _lib.MAX_TASKS:
        raise ValueError(f'{n} tasks: the loss kernels take 1..{_lib.MAX_TASKS} per launch')
    tb = _lib.TaskTable()
    tb.n_tasks = n
    return tb


class _GaussianFocal(torch.autograd.Function):
    """The focal loss of all tasks of a head: one launch per kernel (gga_focal_loss_*), every task's loss and gradient bit for
    bit what a call with that task alone gives. Inputs: T logits, then T targets; outputs: T losses, then T num_pos."""

    @staticmethod
    def forward(ctx, alpha, gamma, scale, *maps):
        T = len(maps) // 2
        _need_cuda(*maps)
        maps = [m.contiguous() for m in maps]
        L = _lib.lib()
        dev = maps[0].device
        out = torch.empty((T, 2), dtype=torch.float32, device=dev)
        tb = _task_table(T)
        for t in range(T):
            e = tb.task[t]
            e.logits, e.target, e.n_heat, e.focal_out = _p(maps[t]), _p(maps[T + t]), maps[t].numel(), out.data_ptr() + 8 * t
        nbytes = L.gga_focal_loss_workspace_bytes(max(m.numel() for m in maps[:T]), T)
        ws = _workspace('focal', nbytes, dev)
        check(L.gga_focal_loss_fwd(C.byref(tb), alpha, gamma, scale, _p(ws), ws.numel(), _stream()), 'gga_focal_loss_fwd')
        ctx.save_for_backward(out, *maps)
        ctx.cfg = (alpha, gamma, scale)
        ctx.set_materialize_grads(False)     # no zero tensors (one fill launch each) for the gradients of the non-differentiable outputs
        return (*out[:, 0].unbind(0), *out[:, 1].unbind(0))

    @staticmethod
    def backward(ctx, *gs):
        out, *maps = ctx.saved_tensors
        T = len(maps) // 2
        live = [t for t in range(T) if gs[t] is not None]
        if not live:
            return (None,) * (3 + 2 * T)
        alpha, gamma, scale = ctx.cfg
        grads = [None] * T
        g = [None] * T
        tb = _task_table(len(live))
        for j, t in enumerate(live):
            grads[t] = torch.empty_like(maps[t])
            g[t] = gs[t].contiguous().float()
            e = tb.task[j]
            e.logits, e.target, e.n_heat, e.focal_out = _p(maps[t]), _p(maps[T + t]), maps[t].numel(), out.data_ptr() + 8 * t
            e.focal_grad, e.grad_logits = _p(g[t]), _p(grads[t])
        check(_lib.lib().gga_focal_loss_bwd(C.byref(tb), alpha, gamma, scale, _stream()), 'gga_focal_loss_bwd')
        return (None, None, None, *grads, *([None] * T))


def gaussian_focal_loss_tasks(logits, targets, alpha=2.0, gamma=4.0, scale=1.0):
    """clip_sigmoid + GaussianFocalLoss(reduction='mean', avg_factor=max(num_pos,1)), times ``scale``, of every task (lists of
    T maps of raw heat-map logits and T targets) in one launch per kernel -> (T losses, T num_pos) device scalars."""
    T = len(logits)
    out = _GaussianFocal.apply(float(alpha), float(gamma), float(scale), *logits, *targets)
    return out[:T], out[T:]


def gaussian_focal_loss(logits, target, alpha=2.0, gamma=4.0, scale=1.0):
    """``gaussian_focal_loss_tasks`` of one task. Returns (loss, num_pos) device scalars."""
    loss, num_pos = gaussian_focal_loss_tasks([logits], [target], alpha, gamma, scale)
    return loss[0], num_pos[0]


# ----------------------------------------------------------------------------- a9
class _GatherPred(torch.autograd.Function):
    """The gather of all tasks of a head (maps of one size, one K): one launch each way. Inputs: per task reg, height, dim,
    rot, ind, mask; outputs: T preds. The tables carry the maps' pointers - nothing is stacked."""

    @staticmethod
    def forward(ctx, *args):
        T = len(args) // 6
        _need_cuda(*args)
        B, _, H, W = args[0].shape
        K = args[4].shape[1]
        pred = torch.empty((T, B, K, 8), dtype=torch.float32, device=args[0].device)
        # NB: bind the NCHW copies to a name until the launch is queued. `_p(x.contiguous())` would free each temporary as soon
        # as its pointer is taken, and the next copy would be allocated over it (channels-last maps).
        keep = [a.contiguous() for a in args]
        tb = _task_table(T)
        for t in range(T):
            e = tb.task[t]
            e.reg, e.height, e.dim, e.rot, e.ind = (_p(a) for a in keep[6 * t:6 * t + 5])
            e.pred = _p(pred[t])
        check(_lib.lib().gga_gather_pred_fwd(C.byref(tb), B, K, H, W, _stream()), 'gga_gather_pred_fwd')
        ctx.save_for_backward(*[keep[6 * t + i] for t in range(T) for i in (4, 5)])
        ctx.geom = (T, B, K, H, W)
        return tuple(pred.unbind(0))

    @staticmethod
    def backward(ctx, *gs):
        T, B, K, H, W = ctx.geom
        im = ctx.saved_tensors
        dev = gs[0].device
        # one allocation, the tasks' four views one behind the other: the entry point clears them all with ONE memset
        hw = B * H * W
        flat = torch.empty(T * 8 * hw, dtype=torch.float32, device=dev)
        gs = [g.contiguous() for g in gs]
        tb = _task_table(T)
        out = []
        for t in range(T):
            f = flat[t * 8 * hw:(t + 1) * 8 * hw]
            maps = (f[:2 * hw].view(B, 2, H, W), f[2 * hw:3 * hw].view(B, 1, H, W), f[3 * hw:6 * hw].view(B, 3, H, W),
                    f[6 * hw:].view(B, 2, H, W))
            e = tb.task[t]
            e.grad_pred, e.ind, e.mask = _p(gs[t]), _p(im[2 * t]), _p(im[2 * t + 1])
            e.g_reg, e.g_height, e.g_dim, e.g_rot = (_p(m) for m in maps)
            out += [*maps, None, None]
        check(_lib.lib().gga_gather_pred_bwd(C.byref(tb), B, K, H, W, _stream()), 'gga_gather_pred_bwd')
        return tuple(out)


def gather_pred_tasks(maps, inds, masks):
    """cat(reg,height,dim,rot) gathered at ``ind`` (head:657-676) for every task in one launch: ``maps[t]`` = (reg, height,
    dim, rot) -> T preds [B,K,8]."""
    args = []
    for m, ind, mask in zip(maps, inds, masks):
        args += [*m, ind.contiguous(), mask.contiguous()]
    return _GatherPred.apply(*args)


def gather_pred(reg, height, dim, rot, ind, mask):
    """``gather_pred_tasks`` of one task -> pred [B,K,8]."""
    return gather_pred_tasks([(reg, height, dim, rot)], [ind], [mask])[0]


# ----------------------------------------------------------------------------- a10-a13
_loss_params_cache = {}


def loss_params(B, K, train_cfg, l1_loss_weight=0.25, w_bpl=0.3, w_srl=0.1, w_pal=0.1):
    """The POD the loss kernels take; built once per (config object, B, K, weights) - reading a Config costs more
    than the kernels' launches."""
    key = (id(train_cfg), int(B), int(K), float(l1_loss_weight), float(w_bpl), float(w_srl), float(w_pal))
    hit = _loss_params_cache.get(key)
    if hit is not None and hit[0] is train_cfg:
        return hit[1]
    prm = _build_loss_params(B, K, train_cfg, l1_loss_weight, w_bpl, w_srl, w_pal)
    _loss_params_cache[key] = (train_cfg, prm)
    return prm


def _build_loss_params(B, K, train_cfg, l1_loss_weight, w_bpl, w_srl, w_pal):
    prm = LossParams()
    prm.B, prm.K = int(B), int(K)
    prm.fm_w = int(train_cfg['grid_size'][0]) // int(train_cfg['out_size_factor'])
    prm.voxel_size[:] = [float(v) for v in train_cfg['voxel_size'][:2]]
    prm.out_size_factor = float(train_cfg['out_size_factor'])
    prm.pc_range[:] = [float(v) for v in train_cfg['point_cloud_range'][:2]]
    prm.code_weights[:] = [float(v) for v in train_cfg['code_weights'][:5]]
    prm.l1_loss_weight = float(l1_loss_weight)
    prm.w_bpl, prm.w_srl, prm.w_pal = float(w_bpl), float(w_srl), float(w_pal)
    return prm


_ZERO_SCALAR = {}


def _zero_scalar(dev):
    z = _ZERO_SCALAR.get(str(dev))
    if z is None:
        z = _ZERO_SCALAR[str(dev)] = torch.zeros((), dtype=torch.float32, device=dev)
    return z


class _BoxLossTerms(torch.autograd.Function):
    """The GGA losses of all tasks of a head (one ``prm``): one launch per kernel. Inputs: per task the nine tensors of
    ``box_loss_terms``; outputs: per task its five terms as five scalars, then the T ``box_out``. Scalars, not one [5] tensor: a
    head that puts two of them into the total loss and logs the other three gets no UnbindBackward (a zero fill per unused term
    and a stack, every step and task) - the terms nobody differentiates arrive in backward as None and the gradient vector is
    ONE stack over a cached zero."""

    @staticmethod
    def forward(ctx, prm, *args):
        T = len(args) // 9
        B, K = prm.B, prm.K
        n = B * K
        L = _lib.lib()
        _need_cuda(*[a for t in range(T) for a in args[9 * t:9 * t + 6]])
        dev = args[0].device
        losses = torch.empty((T, 5), dtype=torch.float32, device=dev)
        flat = torch.empty((T, n * (5 * 8 + 12)), dtype=torch.float32, device=dev)      # one allocation: the entry point clears it with one memset
        ws = _workspace('box', L.gga_box_losses_workspace_bytes(B, K, T), dev)
        tb = _task_table(T)
        keep, grads, boxes = [], [], []
        for t in range(T):
            pred, ind, mask, anno, l2i, bmask, xy, off, slot = args[9 * t:9 * t + 9]
            pred = pred.contiguous()
            keep.append(pred)
            grads.append(flat[t, :5 * n * 8].view(5, B, K, 8))
            boxes.append(flat[t, 5 * n * 8:].view(B, K, 12))
            e = tb.task[t]
            e.pred, e.ind, e.mask, e.anno_box, e.lidar2img, e.bound_mask = _p(pred), _p(ind), _p(mask), _p(anno), _p(l2i), _p(bmask)
            e.ibp_xy, e.ibp_offsets, e.ibp_slot = _p(xy), _p(off), _p(slot)
            e.n_ibp_obj = 0 if slot is None else int(slot.shape[0])
            e.losses, e.box_out, e.term_grads = losses.data_ptr() + 20 * t, _p(boxes[t]), _p(grads[t])
        check(L.gga_box_losses_fwd(C.byref(tb), C.byref(prm), _p(ws), ws.numel(), _stream()), 'gga_box_losses_fwd')
        ctx.save_for_backward(flat)
        ctx.geom = (T, B, K)
        ctx.mark_non_differentiable(*boxes)
        ctx.set_materialize_grads(False)     # the terms nobody differentiates arrive in backward as None
        return (*losses.view(-1).unbind(0), *boxes)

    @staticmethod
    def backward(ctx, *gs):
        (flat,) = ctx.saved_tensors
        T, B, K = ctx.geom
        gs = gs[:5 * T]
        if all(g is None for g in gs):
            return (None,) * (1 + 9 * T)
        dev = flat.device
        z = _zero_scalar(dev)
        g_losses = torch.stack([z if g is None else g.float().reshape(()) for g in gs])      # [5 T] scalars: ONE stack for all tasks
        out = torch.empty((T, B, K, 8), dtype=torch.float32, device=dev)
        tb = _task_table(T)
        for t in range(T):
            e = tb.task[t]
            e.term_grads, e.grad_losses, e.grad_pred = _p(flat[t]), g_losses.data_ptr() + 20 * t, _p(out[t])
        check(_lib.lib().gga_box_losses_bwd(C.byref(tb), B, K, _stream()), 'gga_box_losses_bwd')
        res = [None]
        for t in range(T):
            res += [out[t]] + [None] * 8
        return tuple(res)


def box_loss_terms_tasks(tasks, prm):
    """The GGA losses of every task in one launch per kernel. ``tasks[t]`` = (pred, ind, mask, anno_box, lidar2img, bound_mask,
    ibp_xy, ibp_offsets, ibp_slot) -> (T tuples of the five scalar terms (bpl, srl, pal_min, pal_x, pal_y - the final dict
    values), T ``box_out [B,K,12]`` (rot, l, w, box2d[4], X, Y, p2c_min/x/y))."""
    args = []
    for pred, ind, mask, anno, l2i, bmask, xy, off, slot in tasks:
        args += [pred, ind.contiguous(), mask.contiguous(), anno.contiguous(), l2i.contiguous(), bmask.contiguous(), xy, off, slot]
    T = len(tasks)
    out = _BoxLossTerms.apply(prm, *args)
    return [out[5 * t:5 * t + 5] for t in range(T)], out[5 * T:]


def box_loss_terms(pred, ind, mask, anno_box, lidar2img, bound_mask, ibp_xy, ibp_offsets, ibp_slot, prm):
    """``box_loss_terms_tasks`` of one task -> (the five scalar terms, ``box_out``)."""
    terms, box_out = box_loss_terms_tasks([(pred, ind, mask, anno_box, lidar2img, bound_mask, ibp_xy, ibp_offsets, ibp_slot)], prm)
    return terms[0], box_out[0]


def box_losses(pred, ind, mask, anno_box, lidar2img, bound_mask, ibp_xy, ibp_offsets, ibp_slot, prm):
    """``box_loss_terms`` with the five terms stacked -> (``losses [5]``, ``box_out``)."""
    terms, box_out = box_loss_terms(pred, ind, mask, anno_box, lidar2img, bound_mask, ibp_xy, ibp_offsets, ibp_slot, prm)
    return torch.stack(terms), box_out


# ----------------------------------------------------------------------------- supervised CenterPoint targets and loss
_center_params_cache = {}


def center_params(train_cfg, num_classes):
    """The POD of ``gga_center_targets`` for a head whose task t holds ``num_classes[t]`` classes; built once per
    (config object, layout)."""
    key = (id(train_cfg), tuple(int(n) for n in num_classes))
    hit = _center_params_cache.get(key)
    if hit is not None and hit[0] is train_cfg:
        return hit[1]
    T, n_cls = len(num_classes), int(sum(num_classes))
    if not 1 <= T <= _lib.MAX_TASKS or not 1 <= n_cls <= _lib.CENTER_MAX_CLASSES:
        raise ValueError(f'center targets: {T} tasks / {n_cls} classes; a launch takes 1..{_lib.MAX_TASKS} tasks and '
                         f'1..{_lib.CENTER_MAX_CLASSES} classes')
    prm = _lib.CenterParams()
    prm.pc_range[:] = [float(v) for v in train_cfg['point_cloud_range'][:2]]
    prm.voxel_size[:] = [float(v) for v in train_cfg['voxel_size'][:2]]
    prm.out_size_factor = float(train_cfg['out_size_factor'])
    prm.gaussian_overlap = float(train_cfg['gaussian_overlap'])
    prm.min_radius = int(train_cfg['min_radius'])
    prm.K = int(train_cfg['max_objs']) * int(train_cfg['dense_reg'])
    prm.W = int(train_cfg['grid_size'][0]) // int(train_cfg['out_size_factor'])
    prm.H = int(train_cfg['grid_size'][1]) // int(train_cfg['out_size_factor'])
    prm.n_tasks, prm.n_classes = T, n_cls
    c = 0
    for t, n in enumerate(num_classes):
        prm.task_classes[t], prm.task_class_base[t] = int(n), c
        for i in range(int(n)):
            prm.class_task[c], prm.class_index[c] = t, i
            c += 1
    _center_params_cache[key] = (train_cfg, prm)
    return prm


@torch.no_grad()
def center_targets(boxes, labels, frame_offsets, prm, max_radius=16):
    """The supervised CenterPoint targets of a batch in one launch (centerpoint_head.py:435-583). ``boxes [N,7]`` f32,
    ``labels [N]`` i64, ``frame_offsets [B+1]`` i32 on the device; ``max_radius``: a bound of the batch's gaussian radii (the
    patch table reaches it). -> ``heat`` (flat, task t = the [B, n_cls_t, H, W] block at B * class base of t * H * W),
    ``anno_box [T,B,K,8]``, ``ind [T,B,K]``, ``mask [T,B,K]``."""
    _need_cuda(boxes, labels, frame_offsets)
    dev = boxes.device
    B = frame_offsets.numel() - 1
    T, K = prm.n_tasks, prm.K
    if boxes.dtype != torch.float32 or labels.dtype != torch.int64 or frame_offsets.dtype != torch.int32:
        raise TypeError('center_targets: boxes f32, labels i64, frame_offsets i32')
    if boxes.numel() != labels.numel() * 7:
        raise ValueError('center_targets: boxes must be [N, 7] for labels [N]')
    max_radius = max(int(max_radius), prm.min_radius)
    table, offs = gaussian_patch_table(max_radius, dev)
    heat = torch.empty(B * prm.n_classes * prm.H * prm.W, dtype=torch.float32, device=dev)
    anno = torch.empty((T, B, K, 8), dtype=torch.float32, device=dev)
    ind = torch.empty((T, B, K), dtype=torch.int64, device=dev)
    mask = torch.empty((T, B, K), dtype=torch.uint8, device=dev)
    boxes, labels, frame_offsets = boxes.contiguous(), labels.contiguous(), frame_offsets.contiguous()
    check(_lib.lib().gga_center_targets(_p(boxes), _p(labels), _p(frame_offsets), B, C.byref(prm), _p(ind), _p(mask), _p(anno),
                                        _p(heat), _p(table), _p(offs), max_radius, _stream()), 'gga_center_targets')
    return heat, anno, ind, mask


def center_loss_weights(code_weights, loss_weight):
    w = _lib.CenterLossWeights()
    code_weights = [float(v) for v in code_weights]
    if len(code_weights) != 8:
        raise ValueError(f'center_reg_loss: {len(code_weights)} code_weights; the box code has 8 entries')
    w.code_weights[:] = code_weights
    w.loss_weight = float(loss_weight)
    return w


class _CenterRegLoss(torch.autograd.Function):
    """The code-weighted masked L1 of all tasks of a head: one launch each way (gga_center_reg_loss_*). Inputs: per task pred,
    anno_box, mask; outputs: T losses."""

    @staticmethod
    def forward(ctx, w, *args):
        T = len(args) // 3
        _need_cuda(*args)
        B, K = args[2].shape
        keep = [a.contiguous() for a in args]
        out = torch.empty((T, 2), dtype=torch.float32, device=args[0].device)
        tb = _lib.CenterLossTable()
        tb.n_tasks = T
        for t in range(T):
            e = tb.task[t]
            e.pred, e.anno_box, e.mask, e.loss = _p(keep[3 * t]), _p(keep[3 * t + 1]), _p(keep[3 * t + 2]), out.data_ptr() + 8 * t
        check(_lib.lib().gga_center_reg_loss_fwd(C.byref(tb), B, K, C.byref(w), _stream()), 'gga_center_reg_loss_fwd')
        ctx.save_for_backward(out, *keep)
        ctx.cfg = (w, T, B, K)
        ctx.set_materialize_grads(False)
        return tuple(out[:, 0].unbind(0))

    @staticmethod
    def backward(ctx, *gs):
        out, *keep = ctx.saved_tensors
        w, T, B, K = ctx.cfg
        live = [t for t in range(T) if gs[t] is not None]
        res = [None] * (1 + 3 * T)
        if not live:
            return tuple(res)
        tb = _lib.CenterLossTable()
        tb.n_tasks = len(live)
        g = []
        for j, t in enumerate(live):
            g.append(gs[t].contiguous().float())
            res[1 + 3 * t] = torch.empty((B, K, 8), dtype=torch.float32, device=out.device)
            e = tb.task[j]
            e.pred, e.anno_box, e.mask, e.loss = _p(keep[3 * t]), _p(keep[3 * t + 1]), _p(keep[3 * t + 2]), out.data_ptr() + 8 * t
            e.grad_loss, e.grad_pred = _p(g[-1]), _p(res[1 + 3 * t])
        check(_lib.lib().gga_center_reg_loss_bwd(C.byref(tb), B, K, C.byref(w), _stream()), 'gga_center_reg_loss_bwd')
        return tuple(res)


def center_reg_loss_tasks(preds, anno_boxes, masks, weights):
    """``loss_weight * sum(mask * [anno not NaN] * code_weights * |pred - anno|) / (sum(mask) + 1e-4 + eps)`` of every task
    (centerpoint_head.py:623-638 with L1Loss(reduction='mean')) in one launch each way; ``weights`` = ``center_loss_weights``.
    ``preds[t]`` [B,K,8] (``gather_pred_tasks``), ``anno_boxes[t]`` [B,K,8], ``masks[t]`` [B,K] u8 -> T device scalars."""
    if not 1 <= len(preds) <= _lib.MAX_TASKS:
        raise ValueError(f'{len(preds)} tasks: the loss kernels take 1..{_lib.MAX_TASKS} per launch')
    args = []
    for p, a, m in zip(preds, anno_boxes, masks):
        if p.shape != a.shape or p.shape[-1] != 8 or tuple(m.shape) != tuple(p.shape[:2]) or m.dtype != torch.uint8:
            raise ValueError('center_reg_loss: pred and anno_box [B,K,8] f32, mask [B,K] u8')
        args += [p, a, m]
    return _CenterRegLoss.apply(weights, *args)


# ----------------------------------------------------------------------------- Anchor3DHead: targets, losses, decode
def anchor_params(pos_iou_thr, neg_iou_thr, min_pos_iou, n_rot, num_classes, assign_per_class, pos_weight, dir_offset,
                  dir_limit_offset):
    """The POD of ``gga_anchor_targets``: one (pos_iou_thr, neg_iou_thr, min_pos_iou) per assigner = anchor-size group."""
    n_groups = len(pos_iou_thr)
    if not 1 <= n_groups <= _lib.ANCHOR_MAX_GROUPS or len(neg_iou_thr) != n_groups or len(min_pos_iou) != n_groups:
        raise ValueError(f'anchor targets: {n_groups} assigners; a launch takes 1..{_lib.ANCHOR_MAX_GROUPS}')
    prm = _lib.AnchorParams()
    prm.n_groups, prm.n_rot, prm.num_classes, prm.assign_per_class = n_groups, int(n_rot), int(num_classes), int(bool(assign_per_class))
    for g in range(n_groups):
        prm.pos_iou_thr[g], prm.neg_iou_thr[g], prm.min_pos_iou[g] = float(pos_iou_thr[g]), float(neg_iou_thr[g]), float(min_pos_iou[g])
    prm.pos_weight, prm.dir_offset, prm.dir_limit_offset = float(pos_weight), float(dir_offset), float(dir_limit_offset)
    return prm


@torch.no_grad()
def anchor_targets(anchors, prm, boxes, labels, frame_offsets, frame_offsets_host):
    """The Anchor3DHead targets of a batch (train_mixins.py:12-316) in two launches and no read-back. ``anchors [A,7]`` f32 in
    head order, ``boxes [N,7]`` f32, ``labels [N]`` i64, ``frame_offsets [B+1]`` i32 on the device, ``frame_offsets_host`` the
    same offsets as an int32 numpy array (checked by the entry point before the launch). -> dict of ``labels [B,A]`` i64,
    ``label_weights [B,A]``, ``bbox_targets [B,A,7]``, ``pos [B,A]`` u8, ``dir_targets [B,A]`` i64, ``dir_weights [B,A]``,
    ``pos_count [B]`` i32."""
    _need_cuda(anchors, boxes, labels, frame_offsets)
    if anchors.dtype != torch.float32 or boxes.dtype != torch.float32 or labels.dtype != torch.int64 or \
            frame_offsets.dtype != torch.int32:
        raise TypeError('anchor_targets: anchors and boxes f32, labels i64, frame_offsets i32')
    if anchors.dim() != 2 or anchors.shape[1] != 7 or boxes.numel() != labels.numel() * 7:
        raise ValueError('anchor_targets: anchors [A, 7], boxes [N, 7] for labels [N]')
    host = np.ascontiguousarray(frame_offsets_host, dtype=np.int32)
    if host.shape != (frame_offsets.numel(),):
        raise ValueError('anchor_targets: frame_offsets_host must hold the same B + 1 offsets as frame_offsets')
    dev, A, N, B = anchors.device, anchors.shape[0], labels.numel(), host.shape[0] - 1
    anchors, boxes, labels, frame_offsets = anchors.contiguous(), boxes.contiguous(), labels.contiguous(), frame_offsets.contiguous()
    out = dict(labels=torch.empty((B, A), dtype=torch.int64, device=dev), label_weights=torch.empty((B, A), dtype=torch.float32, device=dev),
               bbox_targets=torch.empty((B, A, 7), dtype=torch.float32, device=dev), pos=torch.empty((B, A), dtype=torch.uint8, device=dev),
               dir_targets=torch.empty((B, A), dtype=torch.int64, device=dev), dir_weights=torch.empty((B, A), dtype=torch.float32, device=dev),
               pos_count=torch.empty(B, dtype=torch.int32, device=dev))
    L = _lib.lib()
    ws = _workspace('anchor_targets', max(L.gga_anchor_targets_workspace_bytes(N, prm.n_groups), 256), dev)
    check(L.gga_anchor_targets(_p(anchors), A, C.byref(prm), _p(boxes), _p(labels), N, _p(frame_offsets), C.c_void_p(host.ctypes.data),
                               B, _p(out['labels']), _p(out['label_weights']), _p(out['bbox_targets']), _p(out['pos']),
                               _p(out['dir_targets']), _p(out['dir_weights']), _p(out['pos_count']), _p(ws), ws.numel(), _stream()),
          'gga_anchor_targets')
    return out


def _anchor_map(x, channels):
    """A prediction map [B, channels, H, W] as the anchor kernels read it: dense NCHW or channels-last memory (anything else is
    copied), and its (batch, channel, pixel) strides in elements."""
    if x.dim() != 4 or x.dtype != torch.float32 or x.shape[1] != channels:
        raise ValueError(f'anchor head: a float32 map [B, {channels}, H, W] expected, got {x.dtype} {tuple(x.shape)}')
    if not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
        x = x.contiguous()
    if x.is_contiguous():
        return x, (channels * x.shape[2] * x.shape[3], x.shape[2] * x.shape[3], 1)
    return x, (channels * x.shape[2] * x.shape[3], 1, channels)


def anchor_loss_params(shape, n_anchors, num_classes, strides, gamma, alpha, beta, code_weight, loss_weights, diff_rad_by_sin):
    B, H, W = shape
    prm = _lib.AnchorLossParams()
    prm.B, prm.HW, prm.n_anchors, prm.num_classes, prm.diff_rad_by_sin = int(B), int(H) * int(W), int(n_anchors), int(num_classes), int(bool(diff_rad_by_sin))
    for field, s in zip(('cls_stride', 'reg_stride', 'dir_stride'), strides):
        getattr(prm, field)[:] = [int(v) for v in s] if s is not None else [0, 0, 0]
    prm.gamma, prm.alpha, prm.beta = float(gamma), float(alpha), float(beta)
    code_weight = [1.0] * 7 if not code_weight else [float(v) for v in code_weight]
    if len(code_weight) != 7:
        raise ValueError(f'anchor loss: {len(code_weight)} code weights; the box code has 7 entries')
    prm.code_weight[:] = code_weight
    prm.loss_weight[:] = [float(v) for v in loss_weights]
    return prm


class _AnchorLoss(torch.autograd.Function):
    """The sigmoid focal, smooth-L1 and direction losses of a whole batch: ``gga_anchor_loss_fwd`` / ``_bwd``, one entry point
    each way. ``cfg`` = (n_anchors, num_classes, gamma, alpha, beta, code_weight, loss_weights, diff_rad_by_sin)."""

    @staticmethod
    def forward(ctx, cfg, targets, cls_score, bbox_pred, dir_cls_pred):
        n_anchors, num_classes = cfg[0], cfg[1]
        _need_cuda(cls_score, bbox_pred, dir_cls_pred)
        cls_score, s_cls = _anchor_map(cls_score, n_anchors * num_classes)
        bbox_pred, s_reg = _anchor_map(bbox_pred, n_anchors * 7)
        s_dir = None
        if dir_cls_pred is not None:
            dir_cls_pred, s_dir = _anchor_map(dir_cls_pred, n_anchors * 2)
        B, _, H, W = cls_score.shape
        if bbox_pred.shape[0] != B or tuple(bbox_pred.shape[2:]) != (H, W) or \
                (dir_cls_pred is not None and (dir_cls_pred.shape[0] != B or tuple(dir_cls_pred.shape[2:]) != (H, W))):
            raise ValueError('anchor loss: the three maps must share batch and map size')
        if tuple(targets['labels'].shape) != (B, H * W * n_anchors):
            raise ValueError(f"anchor loss: targets for {tuple(targets['labels'].shape)} anchors, maps for {(B, H * W * n_anchors)}")
        prm = anchor_loss_params((B, H, W), n_anchors, num_classes, (s_cls, s_reg, s_dir), *cfg[2:])
        out = torch.empty(4, dtype=torch.float32, device=cls_score.device)
        ws = _workspace('anchor_loss', _lib.ANCHOR_LOSS_WORKSPACE_BYTES, cls_score.device)
        t = targets
        check(_lib.lib().gga_anchor_loss_fwd(C.byref(prm), _p(cls_score), _p(bbox_pred), _p(dir_cls_pred), _p(t['labels']),
                                             _p(t['label_weights']), _p(t['pos']), _p(t['bbox_targets']), _p(t['dir_targets']),
                                             _p(t['dir_weights']), _p(t['pos_count']), _p(out), _p(ws), ws.numel(), _stream()),
              'gga_anchor_loss_fwd')
        saved = [out, cls_score, bbox_pred] + ([dir_cls_pred] if dir_cls_pred is not None else [])
        ctx.save_for_backward(*saved)
        ctx.prm, ctx.targets = prm, targets
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, *gs):
        out, cls_score, bbox_pred, *rest = ctx.saved_tensors
        dir_cls_pred = rest[0] if rest else None
        zero = _zero_scalar(out.device)
        grad_out = torch.stack([zero if g is None else g.reshape(()).float() for g in gs])
        g_cls, g_reg = torch.empty_like(cls_score), torch.empty_like(bbox_pred)
        g_dir = torch.empty_like(dir_cls_pred) if dir_cls_pred is not None else None
        assert g_cls.stride() == cls_score.stride() and g_reg.stride() == bbox_pred.stride()
        t = ctx.targets
        check(_lib.lib().gga_anchor_loss_bwd(C.byref(ctx.prm), _p(cls_score), _p(bbox_pred), _p(dir_cls_pred), _p(t['labels']),
                                             _p(t['label_weights']), _p(t['pos']), _p(t['bbox_targets']), _p(t['dir_targets']),
                                             _p(t['dir_weights']), _p(out), _p(grad_out), _p(g_cls), _p(g_reg), _p(g_dir), _stream()),
              'gga_anchor_loss_bwd')
        return None, None, g_cls, g_reg, g_dir


def anchor_losses(cls_score, bbox_pred, dir_cls_pred, targets, n_anchors, num_classes, gamma, alpha, beta, code_weight,
                  loss_weights, diff_rad_by_sin):
    """``loss_cls``, ``loss_bbox``, ``loss_dir`` of ``Anchor3DHead.loss_single`` (anchor3d_head.py:194-278) for the whole batch,
    from the maps as the head returns them ([B, n_anchors * C | 7 | 2, H, W], NCHW or channels-last memory) and the output of
    :func:`anchor_targets`. ``avg_factor`` = sum_b max(pos_count[b], 1) is read on the device. -> three device scalars."""
    cfg = (int(n_anchors), int(num_classes), gamma, alpha, beta, code_weight, loss_weights, diff_rad_by_sin)
    return _AnchorLoss.apply(cfg, targets, cls_score, bbox_pred, dir_cls_pred)


@torch.no_grad()
def anchor_decode(inds, anchors, scores, bbox_pred, dir_cls_pred, n_anchors):
    """``gga_anchor_decode``: the kept anchors ``inds [B,K]`` i64 of every frame -> (boxes [B*K,7] decoded by
    DeltaXYZWLHRBBoxCoder, scores [B*K,C] gathered from ``scores [B,A,C]``, direction bit [B*K] i64) in one launch."""
    _need_cuda(inds, anchors, scores, bbox_pred, dir_cls_pred)
    B, K = inds.shape
    A, nc = scores.shape[1], scores.shape[2]
    if inds.dtype != torch.int64 or scores.dtype != torch.float32 or scores.shape[0] != B or tuple(anchors.shape) != (A, 7):
        raise ValueError('anchor_decode: inds [B,K] i64, scores [B,A,C] f32, anchors [A,7]')
    bbox_pred, s_reg = _anchor_map(bbox_pred, n_anchors * 7)
    s_dir = None
    if dir_cls_pred is not None:
        dir_cls_pred, s_dir = _anchor_map(dir_cls_pred, n_anchors * 2)
    if bbox_pred.shape[0] != B or bbox_pred.shape[2] * bbox_pred.shape[3] * n_anchors != A:
        raise ValueError(f'anchor_decode: bbox_pred {tuple(bbox_pred.shape)} does not hold {A} anchors for {B} frames')
    dev = inds.device
    inds, anchors, scores = inds.contiguous(), anchors.float().contiguous(), scores.contiguous()
    boxes = torch.empty((B * K, 7), dtype=torch.float32, device=dev)
    out_scores = torch.empty((B * K, nc), dtype=torch.float32, device=dev)
    bits = torch.empty(B * K, dtype=torch.int64, device=dev)
    arr = lambda s: None if s is None else (C.c_int64 * 3)(*[int(v) for v in s])
    check(_lib.lib().gga_anchor_decode(_p(inds), B, K, _p(anchors), A, int(n_anchors), nc, _p(scores), _p(bbox_pred), arr(s_reg),
                                       _p(dir_cls_pred), arr(s_dir), _p(boxes), _p(out_scores), _p(bits), _stream()),
          'gga_anchor_decode')
    return boxes, out_scores, bits


# ----------------------------------------------------------------------------- fused BN (+res) (+ReLU)
class _BNActBlocks(torch.autograd.Function):
    """``cat([act_i(bn_i(x_i) + residual_i)], dim=1)`` over ``n >= 1`` column blocks (gga_bn_relu_fwd / gga_bn_relu_bwd, whose
    row strides let a block write its columns of the concatenated map and read its columns of the gradient in place).
    ``n = 1`` (``bn_act``): a [rows, C] or channels-last ``x``, optional residual and ReLU, the layer's own mode.
    ``n >= 2`` (``bn_relu_cat``): channels-last inputs of equal [B, ., H, W].
    ``cfg[i]`` = (eps, momentum, training, relu); tensors: the n inputs, then per block the residual, gamma, beta, running
    mean, running variance and the producer's per-channel sums of x (or None)."""

    @staticmethod
    def forward(ctx, n, cfg, *args):
        xs, res, gammas, betas, rms, rvs, partials = (args[i * n:(i + 1) * n] for i in range(7))
        L = _lib.lib()
        x0 = xs[0]
        dev = x0.device
        chans = [int(x.shape[1]) for x in xs]
        tot = sum(chans)
        rows = x0.numel() // chans[0]
        if n == 1:
            out = torch.empty_like(x0)                # same strides (channels-last stays channels-last)
        else:
            B, _, H, W = x0.shape
            out = torch.empty((B, tot, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        saved_all, bits_all = [], []
        off = 0
        from . import dense_conv
        amax = dense_conv.new_amax(dev)               # max |out| over all blocks, for the convolution that reads out
        for i in range(n):
            eps, momentum, training, relu = cfg[i]
            C = chans[i]
            saved = torch.empty(2 * C, dtype=torch.float32, device=dev)
            bits = torch.empty(L.gga_bn_relu_mask_bytes(rows, C), dtype=torch.uint8, device=dev) if relu else None
            ws = _workspace('bn', L.gga_bn_relu_workspace_bytes(rows, C), dev)
            pt = partials[i] if (training and partials[i] is not None) else None      # the producer of x already reduced the sums
            check(L.gga_bn_relu_fwd(_p(xs[i]), _p(res[i]), _p(gammas[i]), _p(betas[i]), _p(rms[i]), _p(rvs[i]), rows, C,
                                    eps, momentum, int(training), int(relu), out.data_ptr() + 4 * off, tot, _p(bits),
                                    _p(saved), _p(pt), int(pt.shape[0]) if pt is not None else 0, _p(amax), _p(ws), ws.numel(),
                                    _stream()), 'gga_bn_relu_fwd')
            saved_all.append(saved)
            bits_all.append(bits)
            off += C
        ctx.save_for_backward(*xs, *gammas, *saved_all, *bits_all)
        ctx.n, ctx.chans, ctx.rows, ctx.cfg = n, chans, rows, cfg
        ctx.has_res = [r is not None for r in res]
        if amax is None:
            amax = torch.empty(0, dtype=torch.int32, device=dev)
        ctx.mark_non_differentiable(amax, *saved_all)
        ctx.set_materialize_grads(False)     # no zero tensors (one fill launch each) for the gradients of the non-differentiable outputs
        return (out, amax, *saved_all)

    @staticmethod
    def backward(ctx, g, _gamax=None, *_gsaved):
        from . import dense_conv
        n, chans, rows, cfg, has_res = ctx.n, ctx.chans, ctx.rows, ctx.cfg, ctx.has_res
        t = ctx.saved_tensors
        xs, gammas, saved_all, bits_all = t[:n], t[n:2 * n], t[2 * n:3 * n], t[3 * n:4 * n]
        L = _lib.lib()
        done = getattr(g, '_gga_bn_bwd', None)       # the convolution that produced g masked it and reduced the sums
        given, off = [], 0
        for i in range(n):
            use = done is not None and cfg[i][3] and not has_res[i]
            given.append(done.take(g, saved_all[i].data_ptr(), off, chans[i]) if use else None)
            off += chans[i]
        # the incoming gradient must have the memory layout of the output ([rows, tot] row major)
        g = g.contiguous(memory_format=torch.channels_last) if g.dim() == 4 else g.contiguous()
        tot = off
        gxs, gres, ggs, gbs = [], [], [], []
        off = 0
        for i in range(n):
            C = chans[i]
            x = xs[i]
            training, relu = cfg[i][2:]
            gx = torch.empty_like(x)
            gr = torch.empty_like(x) if has_res[i] else None
            gg = torch.empty(C, dtype=torch.float32, device=x.device)
            gb = torch.empty(C, dtype=torch.float32, device=x.device)
            ws = _workspace('bn', L.gga_bn_relu_workspace_bytes(rows, C), x.device)
            amax = dense_conv.new_amax(x.device)         # max |gx| for the convolution backward that reads gx
            if given[i] is not None:
                check(L.gga_bn_relu_bwd_partials(g.data_ptr() + 4 * off, tot, _p(x), _p(gammas[i]), _p(saved_all[i]), rows, C,
                                                 int(training), _p(given[i]), int(given[i].shape[0]), _p(gx), _p(gg), _p(gb),
                                                 _p(amax), _p(ws), ws.numel(), _stream()), 'gga_bn_relu_bwd_partials')
            else:
                check(L.gga_bn_relu_bwd(g.data_ptr() + 4 * off, tot, _p(x), _p(bits_all[i]), _p(gammas[i]), _p(saved_all[i]),
                                        rows, C, int(relu), int(training), _p(gx), _p(gr), _p(gg), _p(gb), _p(amax), _p(ws),
                                        ws.numel(), _stream()), 'gga_bn_relu_bwd')
            dense_conv.set_amax(gx, amax)
            gxs.append(gx), gres.append(gr), ggs.append(gg), gbs.append(gb)
            off += C
        return (None, None, *gxs, *gres, *ggs, *gbs) + (None,) * (3 * n)


def attach_bn_partials(y, stats):
    """Remember the per-channel sums a convolution kernel left for its output ``y`` (valid while ``y`` is not written again)."""
    y.bn_partials = stats
    y._bn_partials_stamp = stamp(y)
    return y


def bn_partials_of(x):
    """The producer's per-channel sums of ``x`` ([tiles, 2, C] f64) if ``x`` still holds what the producer wrote, else None."""
    p = getattr(x, 'bn_partials', None)
    if p is None or getattr(x, '_bn_partials_stamp', None) != stamp(x):
        return None
    return p if (p.dim() == 3 and p.shape[0] >= 1 and p.shape[2] == x.shape[1]) else None


def channel_sums(x):
    """``x.sum`` over every dimension but the channels of a [rows, C] / channels-last [B, C, H, W] gradient (a convolution's
    bias gradient) - ``gga_column_sums`` where the layout allows it, the framework's reduction otherwise."""
    rc = _rows_channels(x) if (x.is_cuda and x.dtype == torch.float32) else None
    C = x.shape[1]
    if rc is None or rc[0] < 1 or not _bn_channels_ok(C) or x.data_ptr() % 16:
        return x.sum(tuple(d for d in range(x.dim()) if d != 1))
    L = _lib.lib()
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = _workspace('bn', L.gga_bn_relu_workspace_bytes(rc[0], C), x.device)
    check(L.gga_column_sums(_p(x), rc[0], C, _p(out), _p(ws), ws.numel(), _stream()), 'gga_column_sums')
    return out


def _rows_channels(x):
    """[rows, C] view of a 2-D contiguous or 4-D channels-last tensor, else None."""
    if x.dim() == 2 and x.is_contiguous():
        return x.shape[0], x.shape[1]
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not (x.shape[1] == 1):
        return x.shape[0] * x.shape[2] * x.shape[3], x.shape[1]
    return None


def _bn_channels_ok(C):
    """The channel counts the BatchNorm / GroupNorm kernels take (``bn_check`` of csrc/bn_relu.hip): a thread owns 4 channels
    and the channel groups tile a 256-thread workgroup."""
    return C >= 4 and C % 4 == 0 and C // 4 <= 256 and 256 % (C // 4) == 0


def _bn_module_ok(bn):
    """A BatchNorm module the fused kernels stand for: affine, with running statistics and a fixed momentum."""
    return bn.affine and bn.track_running_stats and bn.momentum is not None


def bn_act(x, bn, relu=True, residual=None):
    """``relu(bn(x) + residual)`` (each part optional) — one fused HIP pass pair when ``x`` is a CUDA
    f32 [rows, C] / channels-last tensor: training mode (batch statistics) or evaluation mode (running statistics,
    also under autograd: a frozen ``norm_eval`` backbone); the eager ops otherwise."""
    rc = _rows_channels(x) if (x.is_cuda and x.dtype == torch.float32) else None
    C = x.shape[1]
    ok = (rc is not None and rc[0] >= 1 and _bn_channels_ok(C) and _bn_module_ok(bn)
          and (residual is None or (residual.shape == x.shape and residual.stride() == x.stride())))
    if not ok:
        y = bn(x)
        if residual is not None:
            y = y + residual
        return torch.relu(y) if relu else y
    if bn.training:
        count_batch(bn)
    partials = bn_partials_of(x) if bn.training else None
    cfg = ((float(bn.eps), float(bn.momentum), bool(bn.training), bool(relu)),)
    y, amax, saved = _BNActBlocks.apply(1, cfg, x, residual, bn.weight, bn.bias, bn.running_mean, bn.running_var, partials)
    from . import dense_conv
    if amax.numel():
        dense_conv.set_amax(y, amax)
    if relu and residual is None and x.dim() in (2, 4) and y.requires_grad:
        # a 3x3 convolution that consumes y reduces this BatchNorm's backward sums in its backward-data epilogue
        y._gga_bn_src = dense_conv.BnSource(y, [(0, C, x.detach(), bn.weight.detach(), bn.bias.detach(), saved)])
    return y


class _GNAct(torch.autograd.Function):
    """``relu(group_norm(x))`` on a channels-last activation (gga_gn_relu_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, relu):
        from . import dense_conv
        L = _lib.lib()
        B, C, H, W = x.shape
        dev = x.device
        y = torch.empty_like(x)
        stat = torch.empty((B, groups, 2), dtype=torch.float32, device=dev)
        ss = torch.empty((B, 2, C), dtype=torch.float32, device=dev)
        ws = _workspace('gn', L.gga_gn_relu_workspace_bytes(B, C), dev)
        amax = dense_conv.new_amax(dev)
        check(L.gga_gn_relu_fwd(_p(x), _p(gamma), _p(beta), B, H * W, C, groups, eps, int(relu), _p(y), _p(stat), _p(ss), _p(amax),
                                _p(ws), ws.numel(), _stream()), 'gga_gn_relu_fwd')
        ctx.save_for_backward(x, gamma, stat, ss)
        ctx.cfg = (groups, relu)
        if amax is None:
            amax = torch.empty(0, dtype=torch.int32, device=dev)
        ctx.mark_non_differentiable(amax)
        ctx.set_materialize_grads(False)     # no zero tensors (one fill launch each) for the gradients of the non-differentiable outputs
        return y, amax

    @staticmethod
    def backward(ctx, gy, _gamax=None):
        from . import dense_conv
        x, gamma, stat, ss = ctx.saved_tensors
        groups, relu = ctx.cfg
        L = _lib.lib()
        B, C, H, W = x.shape
        gy = gy.contiguous(memory_format=torch.channels_last)
        gx = torch.empty_like(x)
        gg = torch.empty(C, dtype=torch.float32, device=x.device)
        gb = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = _workspace('gn', L.gga_gn_relu_workspace_bytes(B, C), x.device)
        amax = dense_conv.new_amax(x.device)
        check(L.gga_gn_relu_bwd(_p(gy), _p(x), _p(gamma), _p(stat), _p(ss), B, H * W, C, groups, int(relu), _p(gx), _p(gg), _p(gb),
                                _p(amax), _p(ws), ws.numel(), _stream()), 'gga_gn_relu_bwd')
        dense_conv.set_amax(gx, amax)
        return gx, gg, gb, None, None, None


def gn_act(x, gn, relu=True):
    """``relu(gn(x))`` - one fused HIP pass pair when ``x`` is a CUDA f32 channels-last [B, C, H, W] tensor whose group
    size is a multiple of 4 channels, the eager ops otherwise (``torch.nn.GroupNorm`` returns NCHW memory)."""
    C = x.shape[1] if x.dim() == 4 else 0
    ok = (x.dim() == 4 and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
          and _bn_channels_ok(C) and C % gn.num_groups == 0
          and (C // gn.num_groups) % 4 == 0 and gn.affine and x.shape[2] * x.shape[3] >= 1)
    if not ok:
        y = gn(x)
        return torch.relu(y) if relu else y
    y, amax = _GNAct.apply(x, gn.weight, gn.bias, int(gn.num_groups), float(gn.eps), bool(relu))
    if amax.numel():
        from . import dense_conv
        dense_conv.set_amax(y, amax)
    return y


def bn_relu_cat(xs, bns):
    """``torch.cat([relu(bn(x)) for x, bn in zip(xs, bns)], dim=1)`` without the concat copy (and
    without the split copies in backward) when every branch qualifies for the fused BatchNorm
    kernel; the plain composition otherwise."""
    def fusable(x, bn):
        rc = _rows_channels(x) if (x.is_cuda and x.dtype == torch.float32) else None
        C = x.shape[1]
        return (rc is not None and _bn_channels_ok(C) and _bn_module_ok(bn)
                and (bn.training or not torch.is_grad_enabled()))
    same = all(x.shape[0] == xs[0].shape[0] and x.shape[2:] == xs[0].shape[2:] for x in xs)
    if len(xs) < 2 or not same or not all(fusable(x, bn) for x, bn in zip(xs, bns)):
        return torch.cat([bn_act(x, bn, relu=True) for x, bn in zip(xs, bns)], dim=1) if len(xs) > 1 \
            else bn_act(xs[0], bns[0], relu=True)
    for bn in bns:
        if bn.training:
            count_batch(bn)
    n = len(xs)
    cfg = tuple((float(bn.eps), float(bn.momentum), bool(bn.training), True) for bn in bns)
    # the producers' per-channel sums (dense_conv / strided_conv / sparse convolutions), where they left them
    out, amax, *saved = _BNActBlocks.apply(n, cfg, *xs, *[None] * n, *[bn.weight for bn in bns], *[bn.bias for bn in bns],
                                           *[bn.running_mean for bn in bns], *[bn.running_var for bn in bns],
                                           *[bn_partials_of(x) for x in xs])
    from . import dense_conv
    if amax.numel():
        dense_conv.set_amax(out, amax)
    if out.requires_grad and all(bn.training for bn in bns):
        parts, off = [], 0
        for x, bn, sv in zip(xs, bns, saved):
            parts.append((off, int(x.shape[1]), x.detach(), bn.weight.detach(), bn.bias.detach(), sv))
            off += int(x.shape[1])
        out._gga_bn_src = dense_conv.BnSource(out, parts)
    return out


# ----------------------------------------------------------------------------- head output convs
class _HeadConv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        B, C, H, W = x.shape
        cout = weight.shape[0]
        w = weight.contiguous()                       # logical [cout, 64, 3, 3], NCHW-contiguous
        y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
        check(_lib.lib().gga_head_conv3x3_fwd(_p(x), C, None, _p(w), _p(bias), B, H, W, C, cout, _p(y), _stream()),
              'gga_head_conv3x3_fwd')
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        B, C, H, W = x.shape
        cout = w.shape[0]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # the input gradient writes the full [B,64,H,W] tensor: already bandwidth-bound in MIOpen
            gx = torch.ops.aten.convolution_backward(gy, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                     [True, False, False])[0]
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw = torch.empty_like(w)
            gb = torch.empty(cout, dtype=torch.float32, device=x.device) if ctx.has_bias else None
            L = _lib.lib()
            ws = _workspace('headconv', L.gga_head_conv3x3_workspace_bytes(cout), x.device)
            check(L.gga_head_conv3x3_wgrad(_p(x), C, None, _p(gy), B, H, W, C, cout, _p(gw), _p(gb), _p(ws), ws.numel(),
                                           _stream()), 'gga_head_conv3x3_wgrad')
        return gx, gw, gb


def _head_out_conv_ok(conv):
    """An output conv of a head branch that the gga_head_conv3x3_* kernels take (the caller checks its 64 input channels)."""
    return (conv.out_channels <= 4 and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros')


def _head_tail_fwd(x_ptr, x_stride, stats, ws, bn, eps, momentum, training, saved, ss, w, bias, geom, y, tile_map=None):
    """The tail of one head branch on the current stream: the BatchNorm statistics (gga_bn_stats: ``saved`` = mean / invstd,
    ``ss`` = scale / shift), then the output conv, which normalises while it loads, into ``y``. ``x_ptr``, ``x_stride``: the
    BatchNorm input, its C channels every ``x_stride`` floats. ``stats``: (partial sums, their row width, this BatchNorm's
    first column) left by the producer of x, or None - a reduce pass over x (dense) with the workspace ``ws``.
    ``tile_map``: compute the map's active tiles only (gga_head_conv3x3_fwd_tiles)."""
    L = _lib.lib()
    gamma, beta, running_mean, running_var = bn
    B, H, W, C = geom
    pt, width, col = stats if stats is not None else (None, 0, 0)
    check(L.gga_bn_stats(x_ptr if pt is None else None, _p(gamma), _p(beta), _p(running_mean), _p(running_var), B * H * W, C, eps,
                         momentum, int(training), _p(saved), _p(ss), _p(pt), int(pt.shape[0]) if pt is not None else 0, width, col,
                         _p(ws), ws.numel() if ws is not None else 0, _stream()), 'gga_bn_stats')
    if tile_map is not None:
        check(L.gga_head_conv3x3_fwd_tiles(x_ptr, x_stride, _p(ss), _p(w), _p(bias), B, H, W, C, w.shape[0], _p(tile_map), _p(y),
                                           _stream()), 'gga_head_conv3x3_fwd_tiles')
    else:
        check(L.gga_head_conv3x3_fwd(x_ptr, x_stride, _p(ss), _p(w), _p(bias), B, H, W, C, w.shape[0], _p(y), _stream()),
              'gga_head_conv3x3_fwd')


def _head_tail_bwd(gy, x_ptr, x_stride, ss, gamma, saved, w, geom, gw, gb, gx_ptr, gx_stride, gg, gbeta, amax, sparse_grad):
    """Backward of ``_head_tail_fwd`` on the current stream (gga_head_branch_bwd): the output conv's weight / bias gradient
    ``gw`` / ``gb`` and the BatchNorm + ReLU backward ``gg`` / ``gbeta`` and, at ``gx_ptr`` with ``gx_stride`` floats between
    pixels, the gradient of the BatchNorm input; ``amax``: the absmax slot of that gradient, or None."""
    L = _lib.lib()
    B, H, W, C = geom
    cout = w.shape[0]
    ws = _workspace('headbranch', L.gga_head_branch_bwd_workspace_bytes(B, H, W, cout), gy.device)       # (scratch buffers are per stream)
    check(L.gga_head_branch_bwd(_p(gy), x_ptr, x_stride, _p(ss), _p(gamma), _p(saved), _p(w), B, H, W, C, cout, _p(gw), _p(gb),
                                gx_ptr, gx_stride, _p(gg), _p(gbeta), _p(amax), int(sparse_grad), _p(ws), ws.numel(), _stream()),
          'gga_head_branch_bwd')


class _BnReluHeadConv3x3(torch.autograd.Function):
    """``conv(relu(bn(x)))`` for the tail of a head branch without materialising the normalised
    activation: batch statistics (gga_bn_stats), then the output conv applies scale/shift + ReLU
    while it loads x; backward = the weight gradient from x with the same on-load affine, and the
    BatchNorm backward with the ReLU mask recomputed from x and the conv's input gradient rebuilt from
    grad_y in registers (gga_head_tail_bwd: no backward-data tensor)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, weight, bias, eps, momentum, training, partials=None,
                sparse_grad=True):
        L = _lib.lib()
        B, C, H, W = x.shape
        rows, cout = B * H * W, weight.shape[0]
        dev = x.device
        w = weight.contiguous()
        saved = torch.empty(2 * C, dtype=torch.float32, device=dev)
        ss = torch.empty(2 * C, dtype=torch.float32, device=dev)
        # sums left by the convolution that produced x, or a reduce pass over x
        ws = _workspace('bn', L.gga_bn_relu_workspace_bytes(rows, C), dev) if partials is None else None
        y = torch.empty((B, cout, H, W), dtype=torch.float32, device=dev)
        _head_tail_fwd(x.data_ptr(), C, (partials, C, 0) if partials is not None else None, ws,
                       (gamma, beta, running_mean, running_var), eps, momentum, training, saved, ss, w, bias, (B, H, W, C), y)
        ctx.save_for_backward(x, gamma, saved, ss, w)
        ctx.has_bias, ctx.sparse_grad = bias is not None, bool(sparse_grad)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, saved, ss, w = ctx.saved_tensors
        gy = gy.contiguous()
        B, C, H, W = x.shape
        cout = w.shape[0]
        dev = x.device
        gw = torch.empty_like(w)
        gb = torch.empty(cout, dtype=torch.float32, device=dev) if ctx.has_bias else None
        # the weight gradient, then BatchNorm + ReLU backward with the conv's input gradient rebuilt from gy on the fly (never
        # stored); both on the tiles of gy that hold anything
        gx = torch.empty_like(x)
        gg = torch.empty(C, dtype=torch.float32, device=dev)
        gbeta = torch.empty(C, dtype=torch.float32, device=dev)
        from . import dense_conv
        amax = dense_conv.new_amax(dev)
        _head_tail_bwd(gy, x.data_ptr(), C, ss, gamma, saved, w, (B, H, W, C), gw, gb, gx.data_ptr(), C, gg, gbeta, amax,
                       ctx.sparse_grad)
        dense_conv.set_amax(gx, amax)
        return gx, gg, gbeta, None, None, gw, gb, None, None, None, None, None


def bn_relu_head_conv3x3(x, bn, conv, sparse_grad=True):
    """``conv(relu(bn(x)))`` (tail of a SeparateHead branch: the ConvModule's norm + activation
    and the output conv), fused when both halves qualify for their HIP kernels in training mode.
    ``sparse_grad``: a hint for the backward, never a change of its result - False when the output's gradient is
    known to be dense (a heat-map), see ``gga_head_branch_bwd``."""
    rc = _rows_channels(x) if (x.is_cuda and x.dtype == torch.float32) else None
    ok = (rc is not None and x.dim() == 4 and x.shape[1] == 64 and _bn_module_ok(bn) and bn.training and torch.is_grad_enabled()
          and _head_out_conv_ok(conv))
    if not ok:
        return head_conv3x3(bn_act(x, bn, relu=True), conv)
    count_batch(bn)
    partials = bn_partials_of(x)
    return _BnReluHeadConv3x3.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, conv.weight, conv.bias,
                                    float(bn.eps), float(bn.momentum), True, partials, sparse_grad)


_BRANCH_STREAMS = {}
HEAD_STREAMS = int(os.environ.get('GGA_HEAD_STREAMS', '2'))      # streams the branch launches are dealt to (1: none but the caller's)


def _branch_streams(device, n):
    """Streams for the per-branch launches of a head (see _HeadBranches), the caller's first: every one of those launches is a
    persistent grid whose last round leaves most of the chip idle (2240 tiles on 512 workgroup slots: 4.4 rounds), and the
    branches are independent - dealt to two streams, one branch's tail runs beside the next branch's start."""
    k = max(1, min(HEAD_STREAMS, n))
    pool = _BRANCH_STREAMS.setdefault(device, [])
    while len(pool) < k - 1:
        pool.append(torch.cuda.Stream(device=device))
    return [torch.cuda.current_stream(device)] + pool[:k - 1]


def head_cell_tiles(inds, H, W):
    """Per task, the byte map of the 13 x 32 forward tiles of its ``B`` maps that hold a gathered cell (``gga_head_cell_tiles``:
    the tile of ``ind[b, k]`` for every slot, dead ones included - ``gather_pred`` reads those too). ``inds``: the per-task
    ``[B, K]`` int64 index tensors of ``CenterHead_GGA.get_targets``; when they are the consecutive slices of one ``[T, B, K]``
    tensor, as ``get_targets`` uploads them, one launch serves all tasks. -> list of uint8 ``[B * tiles]`` views of one buffer."""
    _need_cuda(*inds)
    L = _lib.lib()
    T = len(inds)
    B, K = inds[0].shape
    for ind in inds:
        if ind.dtype != torch.int64 or tuple(ind.shape) != (B, K) or not ind.is_contiguous():
            raise ValueError(f'head_cell_tiles: every ind must be a contiguous int64 [B, K] tensor (got {ind.dtype} {tuple(ind.shape)})')
    per = int(L.gga_head_cell_tiles_count(B, H, W))
    maps = torch.zeros((T, per), dtype=torch.uint8, device=inds[0].device)
    one = all(inds[t].data_ptr() == inds[0].data_ptr() + 8 * B * K * t for t in range(T))
    for t in range(1 if one else T):
        check(L.gga_head_cell_tiles(_p(inds[t]), (T if one else 1) * B, K, H, W, _p(maps[t]), _stream()), 'gga_head_cell_tiles')
    return list(maps.unbind(0))


class _HeadBranches(torch.autograd.Function):
    """All branches ``conv3x3(64 -> c_i)(relu(bn_i(conv3x3(64 -> 64)_i(x))))`` of a CenterHead (every task's
    SeparateHead, centerpoint_head.py:46-79) on the one shared feature map, as one autograd node.

    Forward: per branch the bf16x6 convolution writes its 64 channels (and their BatchNorm sums) into a column
    block of ONE [B, 64n, H, W] channels-last buffer, the statistics are folded, and the output conv normalises
    while it loads. ``maps`` (None, or per branch None / a tile map of ``head_cell_tiles``): a branch with a map gets its
    output from ``gga_head_conv3x3_fwd_tiles`` - the dense launch's values on the active tiles, +0.0 everywhere else (those
    outputs are views of one zero-filled buffer) - for a map the loss reads at a few cells only.
    Backward: per branch ``gga_head_branch_bwd`` - the output conv's weight gradient and the tail's
    BatchNorm backward, both on the tiles of the branch's output gradient that hold anything (the regression branches
    receive one at a few object cells only) - which writes the gradient w.r.t. the branch's column block of a second
    [B, 64n, H, W] buffer; then ONE
    backward-data convolution 64n -> 64 and ONE weight-gradient call over all branches - where one node per
    branch left autograd n - 1 full-size additions of the shared map's gradient."""

    @staticmethod
    def forward(ctx, x, n, cfg, maps, *t):
        from . import dense_conv
        w1, gam, bet, rm, rv, w2, b2 = (t[i * n:(i + 1) * n] for i in range(7))
        maps = [None] * n if maps is None else list(maps)
        B, C, H, W = x.shape
        dev, tot = x.device, C * n
        Y = torch.empty((B, tot, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        outs, saved_all, ss_all = [], [], []
        x_amax = dense_conv.tensor_amax(x) if dense_conv.PLANES == 2 else None     # from x's producer, for all n convolutions
        # the first convolutions two branches at a time (64 -> 128 channels into adjacent column blocks of Y): the
        # 128-channel form of the kernel stages and splits the shared input once for both
        pair_stats = {}
        for i in range(0, n - 1, 2):          # (the pair's operand is assembled from the two parameters by the weight bank: no cat)
            _, st = dense_conv._run(x, [w1[i].detach(), w1[i + 1].detach()], False, True, x_amax, None, Y, C * i)
            pair_stats[i], pair_stats[i + 1] = (st, 0), (st, C)          # columns of the pair's [tiles, 2, 2C] rows: no copies
        all_stats = []
        for i in range(n):
            if i in pair_stats:
                all_stats.append(pair_stats[i])
            else:
                all_stats.append((dense_conv._run(x, w1[i].detach(), False, True, x_amax, None, Y, C * i)[1], 0))
        # everything the branch launches write is allocated here, on this stream; odd branches are LAUNCHED on a second one
        w2c = [w.contiguous() for w in w2]
        sizes = [B * w2[i].shape[0] * H * W if maps[i] is not None else 0 for i in range(n)]
        tiled = torch.zeros(sum(sizes), dtype=torch.float32, device=dev) if any(sizes) else None      # one fill for all of them
        for i in range(n):
            if maps[i] is not None:
                o = sum(sizes[:i])
                outs.append(tiled[o:o + sizes[i]].view(B, w2[i].shape[0], H, W))
            else:
                outs.append(torch.empty((B, w2[i].shape[0], H, W), dtype=torch.float32, device=dev))
            saved_all.append(torch.empty(2 * C, dtype=torch.float32, device=dev))
            ss_all.append(torch.empty(2 * C, dtype=torch.float32, device=dev))
        streams = _branch_streams(dev, n)
        for st_ in streams[1:]:
            st_.wait_stream(streams[0])
        for i in range(n):
            eps, momentum = cfg[i][:2]
            stats, col = all_stats[i]
            with torch.cuda.stream(streams[i % len(streams)]):
                _head_tail_fwd(Y.data_ptr() + 4 * C * i, tot, (stats, int(stats.shape[2]), col), None,
                               (gam[i], bet[i], rm[i], rv[i]), eps, momentum, True, saved_all[i], ss_all[i], w2c[i], b2[i],
                               (B, H, W, C), outs[i], maps[i])
        for st_ in streams[1:]:
            streams[0].wait_stream(st_)
        ctx.save_for_backward(x, Y, *w1, *gam, *w2, *saved_all, *ss_all)
        ctx.n, ctx.has_bias, ctx.x_amax = n, [b is not None for b in b2], x_amax
        ctx.sparse_grad = [int(c[2]) for c in cfg]
        ctx.bn_src = dense_conv.bn_source(x, C) if dense_conv.BN_BWD_FUSED else None     # x = relu(bn(shared conv))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gys):
        from . import dense_conv
        n = ctx.n
        t = ctx.saved_tensors
        x, Y = t[0], t[1]
        w1, gam, w2, saved_all, ss_all = (t[2 + i * n:2 + (i + 1) * n] for i in range(5))
        B, C, H, W = x.shape
        dev, tot = x.device, C * n
        G = torch.empty_like(Y)
        # the tail kernels leave max |G_i| of their column block: the weight gradient scales every branch's block by its own
        # maximum (a regression branch's gradient lives on a few object cells, orders of magnitude below a heat-map branch's:
        # under ONE scale for the 960 channels its two fp16 planes keep only a few bits - measured 3e-3 .. 7e-3 on those
        # branches' weight gradients where fp32 is at 1e-5); the backward-data convolution, whose result sums over the branches,
        # takes the largest of them
        g_blocks = dense_conv.new_amax(dev, n)
        gw2, gb2, ggam, gbet = [], [], [], []
        gyc = [g.contiguous() for g in gys]
        w2c = [w.contiguous() for w in w2]
        for i in range(n):                      # outputs of the branch launches: allocated on this stream (see forward)
            gw2.append(torch.empty_like(w2c[i]))
            gb2.append(torch.empty(w2[i].shape[0], dtype=torch.float32, device=dev) if ctx.has_bias[i] else None)
            ggam.append(torch.empty(C, dtype=torch.float32, device=dev))
            gbet.append(torch.empty(C, dtype=torch.float32, device=dev))
        streams = _branch_streams(dev, n)
        for st_ in streams[1:]:
            st_.wait_stream(streams[0])
        for i in range(n):
            with torch.cuda.stream(streams[i % len(streams)]):
                _head_tail_bwd(gyc[i], Y.data_ptr() + 4 * C * i, tot, ss_all[i], gam[i], saved_all[i], w2c[i], (B, H, W, C),
                               gw2[i], gb2[i], G.data_ptr() + 4 * C * i, tot, ggam[i], gbet[i],
                               g_blocks[i:i + 1] if g_blocks is not None else None, ctx.sparse_grad[i])
        for st_ in streams[1:]:
            streams[0].wait_stream(st_)
        wcat = [w.detach() for w in w1]            # stands for the [64n, 64, 3, 3] concatenation (weight bank: never made)
        g_amax = g_blocks.max().reshape(1) if g_blocks is not None else None       # (bits of non-negative floats order like ints)
        gx = dense_conv.run_bn_bwd(G, wcat, g_amax, None, ctx.bn_src) if ctx.needs_input_grad[0] else None
        gwcat = dense_conv._wgrad(x, G, wcat, ctx.x_amax if dense_conv.PLANES == 2 else None, g_blocks, g_per_block=True)
        gw1 = list(gwcat.split(C, dim=0))
        none = [None] * n
        return (gx, None, None, None, *gw1, *ggam, *gbet, *none, *none, *gw2, *gb2)


def head_branches(x, branches, sparse_grad=None, tile_maps=None):
    """Outputs of the head branches ``[(conv1, bn, conv2), ...]`` that all read ``x`` (see _HeadBranches), or
    None when a branch does not qualify for the fused kernels (the caller then runs them one by one).
    ``sparse_grad``: per branch, False where the output's gradient is known to be dense (a heat-map) - a hint for
    ``gga_head_branch_bwd``, never a change of the result; default: every branch may be sparse.
    ``tile_maps``: per branch None, or a map of ``head_cell_tiles`` - that branch's output is then computed on the map's
    active tiles only and is +0.0 elsewhere (for an output that is read at the gathered cells alone); default: all dense."""
    from . import dense_conv
    rc = _rows_channels(x) if (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4) else None
    if rc is None or x.shape[1] != 64 or not torch.is_grad_enabled() or not dense_conv.ENABLED or not dense_conv.WGRAD:
        return None
    for conv1, bn, conv2 in branches:
        ok = (dense_conv.eligible(conv1, x) and conv1.bias is None and conv1.out_channels == 64 and _bn_module_ok(bn)
              and bn.training and type(conv2) is torch.nn.Conv2d and conv2.in_channels == 64 and _head_out_conv_ok(conv2))
        if not ok:
            return None
    for _, bn, _ in branches:
        count_batch(bn)
    n = len(branches)
    sparse = [True] * n if sparse_grad is None else [bool(s) for s in sparse_grad]
    assert len(sparse) == n
    cfg = tuple((float(bn.eps), float(bn.momentum), s) for (_, bn, _), s in zip(branches, sparse))
    cols = ([c1.weight for c1, _, _ in branches], [bn.weight for _, bn, _ in branches], [bn.bias for _, bn, _ in branches],
            [bn.running_mean for _, bn, _ in branches], [bn.running_var for _, bn, _ in branches],
            [c2.weight for _, _, c2 in branches], [c2.bias for _, _, c2 in branches])
    if tile_maps is not None:
        B, _, H, W = x.shape
        per = int(_lib.lib().gga_head_cell_tiles_count(B, H, W))
        assert len(tile_maps) == n
        for m in tile_maps:
            if m is not None and not (m.dtype == torch.uint8 and m.device == x.device and m.is_contiguous() and m.numel() == per):
                raise ValueError(f'head_branches: a tile map must be a contiguous uint8 tensor of {per} tiles on {x.device}')
        tile_maps = tuple(tile_maps) if any(m is not None for m in tile_maps) else None
    return _HeadBranches.apply(x, n, cfg, tile_maps, *[t for col in cols for t in col])


def head_conv3x3(x, conv):
    """``conv(x)`` for the output convs of the head branches (64 -> 1..4 channels, 3x3, pad 1): the
    HBM-bound HIP kernels when ``x`` is a CUDA f32 channels-last activation, MIOpen otherwise."""
    ok = (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 64
          and x.is_contiguous(memory_format=torch.channels_last) and _head_out_conv_ok(conv))
    if not ok:
        return conv(x)
    return _HeadConv3x3.apply(x, conv.weight, conv.bias)


def centerpoint_detect(boxes, scores, labels, coder_range, coder_score_threshold, score_threshold, limit_range, nms_threshold,
                       pre_max_size, post_max_size, num_classes):
    """``gga_centerpoint_detect``: boxes [T, B, K, D] / scores / labels [T, B, K] of all tasks' decoded top-k cells -> the
    detections of every frame (masks, rotated BEV NMS, range filter, task merge, bottom-centre z, global labels) in one launch.
    -> (out_boxes [B, T*K, D], out_scores [B, T*K], out_labels int32 [B, T*K], count int32 [B])."""
    _need_cuda(boxes, scores, labels)
    T, B, K, D = boxes.shape
    dev = boxes.device
    boxes, scores, labels = boxes.float().contiguous(), scores.float().contiguous(), labels.float().contiguous()
    out_boxes = torch.empty((B, T * K, D), dtype=torch.float32, device=dev)
    out_scores = torch.empty((B, T * K), dtype=torch.float32, device=dev)
    out_labels = torch.empty((B, T * K), dtype=torch.int32, device=dev)
    count = torch.zeros((B,), dtype=torch.int32, device=dev)
    offs, flag = [], 0
    for n in num_classes:
        offs.append(flag)
        flag += int(n)
    cr = const_tensor([float(v) for v in coder_range], dev)
    lr = const_tensor([float(v) for v in limit_range], dev) if limit_range is not None and len(limit_range) > 0 else None
    co = const_tensor(offs, dev, torch.int32)
    sc = const_tensor([int(int(n) == 1) for n in num_classes], dev, torch.int32)
    ws = _workspace('cp_detect', _lib.lib().gga_centerpoint_detect_workspace_bytes(T, B), dev)
    check(_lib.lib().gga_centerpoint_detect(_p(boxes), _p(scores), _p(labels), T, B, K, D, _p(cr),
                                            float(coder_score_threshold) if coder_score_threshold is not None else 0.0,
                                            int(coder_score_threshold is not None), float(score_threshold), _p(lr), float(nms_threshold),
                                            int(pre_max_size or 0), int(post_max_size or 0), _p(co), _p(sc), _p(out_boxes), _p(out_scores),
                                            _p(out_labels), _p(count), _p(ws), ws.numel(), _stream()), 'gga_centerpoint_detect')
    return out_boxes, out_scores, out_labels, count


def multiclass_nms3d(boxes, scores, scene, n_scenes, score_thr, iou_thr):
    """``gga_multiclass_nms3d``: per-class greedy BEV NMS of every scene of a batch in a fixed number of launches.
    boxes [n, 7] (x, y, z, dx, dy, dz, heading; heading 0 for axis-aligned boxes), scores [n, C], scene [n] int64 (rows in any
    order) -> (rows int32 [n * C], classes int32 [n * C], count int32 [n_scenes]), all on the device: the kept detections
    packed scene by scene, class-ascending, by descending score within a class; only the first ``count.sum()`` entries are
    written. Nothing is read back here: the caller downloads ``count`` once."""
    _need_cuda(boxes, scores, scene)
    if boxes.dim() != 2 or boxes.shape[1] != 7 or scores.dim() != 2 or scores.shape[0] != boxes.shape[0] or \
            scene.shape != (boxes.shape[0],):
        raise ValueError(f'multiclass_nms3d: boxes [n, 7], scores [n, C], scene [n] expected, got {tuple(boxes.shape)}, '
                         f'{tuple(scores.shape)}, {tuple(scene.shape)}')
    n, nc = scores.shape
    if not 1 <= nc <= _lib.MULTICLASS_NMS_MAX_CLASSES:
        raise ValueError(f'multiclass_nms3d: {nc} classes, the kernel takes 1..{_lib.MULTICLASS_NMS_MAX_CLASSES}')
    dev = boxes.device
    boxes, scores, scene = boxes.float().contiguous(), scores.float().contiguous(), scene.long().contiguous()
    rows = torch.empty(n * nc, dtype=torch.int32, device=dev)
    classes = torch.empty(n * nc, dtype=torch.int32, device=dev)
    count = torch.empty(int(n_scenes), dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = _workspace('mc_nms', L.gga_multiclass_nms3d_workspace_bytes(n, nc, int(n_scenes)), dev)
    check(L.gga_multiclass_nms3d(_p(boxes), _p(scores), _p(scene), n, nc, int(n_scenes), float(score_thr), float(iou_thr),
                                 _p(rows), _p(classes), _p(count), _p(ws), ws.numel(), _stream()), 'gga_multiclass_nms3d')
    return rows, classes, count


TTA_KINDS = {'reg': _lib.TTA_REG, 'rot': _lib.TTA_ROT, 'vel': _lib.TTA_VEL}       # every other key is only mirrored


def tta_merge_maps(outs, group, hflip, vflip, n_frames):
    """``gga_tta_merge_maps``: the head's eval output ``[[{key: [V * F, C, H, W]}], ...]`` (one entry per task, view-major
    batch) -> the same structure with batch ``S * F``: per scale group ``group[v]`` in ``0..S-1`` the mean, in view order, of
    the views' maps with their flips (``hflip[v]``, ``vflip[v]``) undone - all tasks, keys, groups and frames in one launch,
    with the bits of the reference's per-view flip / add / divide sequence (centerpoint_gga.py:123-182)."""
    V, F_ = len(group), int(n_frames)
    if not (len(hflip) == V and len(vflip) == V):
        raise ValueError('tta_merge_maps: group, hflip and vflip must have one entry per view')
    if not 1 <= V <= _lib.TTA_MAX_VIEWS:
        raise ValueError(f'tta_merge_maps: {V} views, the kernel takes 1..{_lib.TTA_MAX_VIEWS}')
    S = max(int(g) for g in group) + 1
    tb = _lib.TtaTable()
    tb.n_views, tb.n_groups = V, S
    for v in range(V):
        tb.group[v], tb.hflip[v], tb.vflip[v] = int(group[v]), int(bool(hflip[v])), int(bool(vflip[v]))
    merged, keep, n, shape = [], [], 0, None
    for task in outs:
        if len(task) != 1:
            raise ValueError(f'tta_merge_maps: {len(task)} feature levels in a task, the head returns one')
        new = {}
        for key, src in task[0].items():
            _need_cuda(src)
            if src.dtype != torch.float32 or src.dim() != 4 or src.shape[0] != V * F_:
                raise ValueError(f'tta_merge_maps: {key} must be float32 [{V * F_}, C, H, W], got {src.dtype} {tuple(src.shape)}')
            if shape is None:
                shape = tuple(src.shape[2:])
            elif tuple(src.shape[2:]) != shape:
                raise ValueError(f'tta_merge_maps: {key} is {tuple(src.shape[2:])}, the other maps are {shape}')
            if n == _lib.TTA_MAX_MAPS:
                raise ValueError(f'tta_merge_maps: more than {_lib.TTA_MAX_MAPS} maps')
            src = src.contiguous()
            dst = torch.empty((S * F_,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
            e = tb.map[n]
            e.src, e.dst, e.channels, e.kind = _p(src), _p(dst), src.shape[1], TTA_KINDS.get(key, _lib.TTA_PLAIN)
            keep.append(src)
            new[key] = dst
            n += 1
        merged.append([new])
    if shape is None:
        raise ValueError('tta_merge_maps: no maps')
    tb.n_maps = n
    check(_lib.lib().gga_tta_merge_maps(C.byref(tb), F_, shape[0], shape[1], _stream()), 'gga_tta_merge_maps')
    return merged


def mono3d_tta_merge(outs, n_frames):
    """``gga_mono3d_tta_merge``: the mono3d head's output for a view-major two-view batch - the tuple ``(cls_scores, bbox_preds,
    dir_cls_preds, depth_cls_preds, weights, attr_preds, centernesses)`` of per-level ``[2 F, C, H, W]`` maps, view 0 the
    unflipped images, view 1 their horizontal mirrors - merged into ``[F, C, H, W]`` maps in one launch, with the bits of the
    reference's flip / ``1 - x`` / mean sequence (single_stage_mono3d.py:141-181). The direction classifier keeps view 0 (a
    slice); a group of ``None`` entries stays as it is."""
    F_ = int(n_frames)
    tb = _lib.Mono3dTtaTable()
    tb.n_frames = F_
    merged, keep, n = [], [], 0
    for g, group in enumerate(outs):
        if group[0] is None:
            merged.append(list(group))
            continue
        new = []
        for src in group:
            _need_cuda(src)
            if src.dtype != torch.float32 or src.dim() != 4 or src.shape[0] != 2 * F_:
                raise ValueError(f'mono3d_tta_merge: group {g} must hold float32 [{2 * F_}, C, H, W] maps, got {src.dtype} {tuple(src.shape)}')
            if g == 2:                            # dir_cls keeps the original
                new.append(src[:F_])
                continue
            if g == 1 and src.shape[1] < 7:
                raise ValueError(f'mono3d_tta_merge: a regression map of {src.shape[1]} channels (at least 7 expected)')
            if n == _lib.MONO3D_TTA_MAX_MAPS:
                raise ValueError(f'mono3d_tta_merge: more than {_lib.MONO3D_TTA_MAX_MAPS} maps')
            src = src.contiguous()
            dst = torch.empty((F_,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
            e = tb.map[n]
            e.src, e.dst, e.channels, e.H, e.W = _p(src), _p(dst), src.shape[1], src.shape[2], src.shape[3]
            e.kind = _lib.MONO3D_TTA_REG if g == 1 else _lib.MONO3D_TTA_MEAN
            keep.append(src)
            new.append(dst)
            n += 1
        merged.append(new)
    if n:
        tb.n_maps = n
        check(_lib.lib().gga_mono3d_tta_merge(C.byref(tb), _stream()), 'gga_mono3d_tta_merge')
    return tuple(merged)


def mono3d_collect(rows, classes, count, scores, boxes, dir_scores, attr_scores, boxes2d, max_per_img):
    """``gga_mono3d_collect``: the packed output of ``multiclass_nms3d`` (scene = image) -> one byte buffer on the device that
    holds, for ``B = len(count)`` images, ``max_per_img`` slots of boxes [code], score, label, direction, attribute and 2D box
    (when ``boxes2d`` is given) and the per-image counts; an image with more kept detections than ``max_per_img`` keeps its
    highest scores in descending order. -> ``(buffer, views)``: ``views(host_buffer)`` cuts a (downloaded) copy of the buffer
    into ``dict(boxes, scores, labels, dir, attr, boxes2d, count)``. Nothing is read back here."""
    _need_cuda(rows, classes, count, scores, boxes)
    B, (n, nc), code, M = int(count.shape[0]), scores.shape, int(boxes.shape[1]), int(max_per_img)
    if boxes.shape[0] != n or rows.numel() < n * nc or classes.numel() < n * nc:
        raise ValueError(f'mono3d_collect: scores {tuple(scores.shape)}, boxes {tuple(boxes.shape)}, lists of {rows.numel()} / {classes.numel()}')
    dev = boxes.device
    scores, boxes = scores.float().contiguous(), boxes.float().contiguous()
    opt = lambda t, dt: None if t is None else t.to(dt).contiguous()
    dir_scores, attr_scores, boxes2d = opt(dir_scores, torch.int64), opt(attr_scores, torch.int64), opt(boxes2d, torch.float32)
    fields = [('boxes', torch.float32, (B, M, code)), ('scores', torch.float32, (B, M)), ('labels', torch.int32, (B, M)),
              ('dir', torch.int32, (B, M)), ('attr', torch.int32, (B, M)), ('boxes2d', torch.float32, (B, M, 4)),
              ('count', torch.int32, (B,))]
    if boxes2d is None:
        fields = [f for f in fields if f[0] != 'boxes2d']
    where, at = {}, 0
    for name, dt, shape in fields:
        where[name] = (at, dt, shape)
        at += -(-int(np.prod(shape)) * 4 // 16) * 16

    def views(buf):
        return {name: buf[o:o + int(np.prod(shape)) * 4].view(dt).reshape(shape) for name, (o, dt, shape) in where.items()}

    out = torch.empty(at, dtype=torch.uint8, device=dev)
    v = views(out)
    L = _lib.lib()
    ws = _workspace('mono3d_collect', L.gga_mono3d_collect_workspace_bytes(n, nc, B), dev)
    check(L.gga_mono3d_collect(_p(rows), _p(classes), _p(count), B, n, nc, _p(scores), nc, _p(boxes), code,
                               _p(dir_scores), _p(attr_scores), _p(boxes2d), M, _p(v['boxes']), _p(v['scores']), _p(v['labels']),
                               _p(v['dir']), _p(v['attr']), _p(v.get('boxes2d')), _p(v['count']), _p(ws), ws.numel(), _stream()),
          'gga_mono3d_collect')
    return out, views
