"""Sparse tensors and sparse 3D convolution layers on the HIP kernels of
gga_amd/csrc/sparse_conv.hip — the subset of the mmcv / spconv API the reference's
SparseEncoder uses (mmdet3d/ops/sparse_block.py:9-20,167-184; mmdet3d/models/
middle_encoders/sparse_encoder.py:120-138): ``SparseConvTensor(features, indices,
spatial_shape, batch_size)`` with ``.features`` / ``.indices`` / ``.dense()`` /
``replace_feature``, ``SparseModule``, ``SparseSequential`` and the conv layers
``SubMConv3d`` / ``SparseConv3d`` registered in ``CONV_LAYERS`` so
``build_conv_layer(dict(type='SubMConv3d', indice_key=...), Cin, Cout, k, stride=, padding=,
bias=False)`` works unchanged. Weights use the mmcv layout ``[kz, ky, kx, Cin, Cout]``.
"""
import ctypes as C
import math
import os

import torch
from torch import nn

from . import _lib
from . import functional as F
from . import gather_gemm as G
from ._lib import check
# (the tilings and orders are reached as sparse._Halo / mask_order / morton_order by bench.py's sparse roofline and the tests)
from .gather_gemm import Rulebook, _Halo, mask_order, morton_order         # noqa: F401
from .registry import CONV_LAYERS


def _triple(v):
    return tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v),) * 3


def _i3(v):
    return (C.c_int32 * 3)(*v)


class _Level:
    """One resolution level: coordinates + hash index + cached rule books."""

    def __init__(self, coors, spatial_shape, batch_size, index=None, index_n=None):
        self.coors = coors.contiguous()
        self.n = int(coors.shape[0])
        self.shape = tuple(int(s) for s in spatial_shape)
        self.batch_size = int(batch_size)
        self.index, self.index_n = index, index_n
        self._subm = {}

    def ensure_index(self):
        if self.index is None:
            L = _lib.lib()
            self.index_n = self.n
            self.index = torch.empty(L.gga_sparse_index_bytes(self.n), dtype=torch.uint8, device=self.coors.device)
            D, H, W = self.shape
            check(L.gga_sparse_build_index(F._p(self.coors), self.n, self.batch_size, D, H, W, F._p(self.index),
                                           self.index.numel(), F._stream()), 'gga_sparse_build_index')
        return self.index

    def subm_rulebook(self, kernel):
        nbr = self._subm.get(kernel)
        if nbr is None:
            self.ensure_index()
            kvol = kernel[0] * kernel[1] * kernel[2]
            nbr = torch.empty((kvol, self.n), dtype=torch.int32, device=self.coors.device)
            pad = tuple(k // 2 for k in kernel)
            check(_lib.lib().gga_sparse_rulebook(F._p(self.coors), self.n, F._p(self.coors), self.n, self.batch_size,
                                                 _i3(self.shape), _i3(self.shape), _i3(kernel), _i3((1, 1, 1)), _i3(pad),
                                                 F._p(self.index), self.index_n, None, 0, F._p(nbr), None,
                                                 F._stream()), 'gga_sparse_rulebook')
            cells = self.batch_size * self.shape[0] * self.shape[1] * self.shape[2]
            nbr = Rulebook(nbr, self.coors, self.n / max(cells, 1), (self.batch_size, max(self.shape)))
            self._subm[kernel] = nbr
        return nbr

    def strided(self, kernel, stride, padding):
        """-> (output level, nbr [kvol,n_out], nbr_t [kvol,n_in])"""
        L = _lib.lib()
        dev = self.coors.device
        self.ensure_index()
        kvol = kernel[0] * kernel[1] * kernel[2]
        cap = self.n * min(kvol, 8)       # a site reaches at most ceil(k/s)^3 <= 8 outputs for k=3, s>=2
        for a in range(3):
            cap = cap if stride[a] >= 2 or kernel[a] == 1 else self.n * kvol
        out_coors = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        n_out_d = torch.zeros(1, dtype=torch.int32, device=dev)
        out_index = torch.empty(L.gga_sparse_out_index_bytes(self.n, kvol), dtype=torch.uint8, device=dev)
        ws = F._workspace('sp_sites', L.gga_sparse_out_sites_workspace_bytes(self.n, kvol), dev)
        out_dhw = (C.c_int32 * 3)()
        check(L.gga_sparse_conv_out_sites(F._p(self.coors), self.n, self.batch_size, _i3(self.shape), _i3(kernel),
                                          _i3(stride), _i3(padding), out_dhw, F._p(out_coors), cap, F._p(n_out_d),
                                          F._p(out_index), out_index.numel(), F._p(ws), ws.numel(), F._stream()),
              'gga_sparse_conv_out_sites')
        n_out = int(n_out_d.item())        # data-dependent size: one 4-byte read back, as spconv does
        if not 0 <= n_out <= cap:
            raise RuntimeError(f'sparse conv output sites: count {n_out} outside [0, {cap}]')
        if n_out == 0:                     # e.g. a (3,1,1)/(2,1,1) conv over sites that all sit in an odd, unpadded top slice
            return _empty_level(tuple(out_dhw), self.batch_size, dev), None, None
        out = _Level(out_coors[:n_out], tuple(out_dhw), self.batch_size, index=out_index, index_n=self.n * kvol)
        nbr = torch.empty((kvol, n_out), dtype=torch.int32, device=dev)
        nbr_t = torch.empty((kvol, self.n), dtype=torch.int32, device=dev)
        check(L.gga_sparse_rulebook(F._p(out.coors), n_out, F._p(self.coors), self.n, self.batch_size, _i3(self.shape),
                                    _i3(out.shape), _i3(kernel), _i3(stride), _i3(padding), F._p(self.index),
                                    self.index_n, F._p(out_index), out.index_n, F._p(nbr), F._p(nbr_t), F._stream()),
              'gga_sparse_rulebook')
        return out, Rulebook(nbr), Rulebook(nbr_t)


def _empty_level(shape, batch_size, device):
    return _Level(torch.zeros((0, 4), dtype=torch.int32, device=device), shape, batch_size)


def conv_out_shape(shape, kernel, stride, padding):
    return tuple((shape[i] + 2 * padding[i] - kernel[i]) // stride[i] + 1 for i in range(3))


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size, grid=None, _level=None):
        F._need_cuda(features, indices)
        self.features = features
        self.indices = indices if indices.dtype == torch.int32 else indices.int()
        self.spatial_shape = list(spatial_shape)
        self.batch_size = batch_size
        self.indice_dict = {}
        self._level = _level or _Level(self.indices, spatial_shape, batch_size)

    def replace_feature(self, new_features):
        out = SparseConvTensor(new_features, self.indices, self.spatial_shape, self.batch_size, _level=self._level)
        out.indice_dict = self.indice_dict
        return out

    @property
    def spatial_size(self):
        return int(torch.tensor(self.spatial_shape).prod())

    def dense(self, channels_first=True):
        """[N,C] features -> dense [B, C, D, H, W] (zeros elsewhere): the pillar-scatter canvas kernel
        with (z,y) folded into the row index."""
        D, H, W = self._level.shape
        c = self.indices
        if c.shape[0] == 0:
            out = self.features.new_zeros((self.batch_size, self.features.shape[1], D, H, W)) + 0 * self.features.sum()
            return out if channels_first else out.permute(0, 2, 3, 4, 1).contiguous()
        folded = torch.stack([c[:, 0], torch.zeros_like(c[:, 0]), c[:, 1] * H + c[:, 2], c[:, 3]], 1).contiguous()
        out = F.pillar_scatter(self.features, folded, self.batch_size, D * H, W, unique=True)
        out = out.view(self.batch_size, self.features.shape[1], D, H, W)
        return out if channels_first else out.permute(0, 2, 3, 4, 1).contiguous()


class IndexPlan:
    """Index structures of one batch for a stack of sparse convolutions (levels, rule books), built
    ahead of the features by ``build_index_plan`` - e.g. on a side stream while the previous
    step's backward is still running, so that the host reads of the site counts do not drain the
    main stream's launch queue."""

    def __init__(self, level0, indice_dict):
        self.level0, self.indice_dict = level0, indice_dict

    def tensors(self):
        """Every device tensor the plan holds (for ``Tensor.record_stream`` when it was built on
        another stream than the one that consumes it)."""
        levels, books = [self.level0], []
        for lvl, out_lvl, rb, rb_t in self.indice_dict.values():
            levels.append(out_lvl)
            books += [rb, rb_t]
        for lvl in levels:
            books += list(lvl._subm.values())
            for t in (lvl.coors, lvl.index):
                if t is not None:
                    yield t
        for rb in books:
            if rb is not None:
                for t in (rb.nbr, rb.mask, rb.perm):
                    if t is not None:
                        yield t


def build_index_plan(module, coors, spatial_shape, batch_size):
    """Walk the ``SparseConvolution`` layers of ``module`` in execution order (= registration order
    for the sequential encoders of the reference) and build every level / rule book they will ask for."""
    coors = coors if coors.dtype == torch.int32 else coors.int()
    lvl = level0 = _Level(coors, spatial_shape, batch_size)
    indice_dict = {}
    for m in module.modules():
        if not isinstance(m, SparseConvolution):
            continue
        if m.subm:
            if lvl.n:
                lvl.subm_rulebook(m.kernel_size)
        else:
            cached = indice_dict.get(m.indice_key) if m.indice_key else None
            if cached is None or cached[0] is not lvl:
                if lvl.n == 0:
                    cached = (lvl, _empty_level(conv_out_shape(lvl.shape, m.kernel_size, m.stride, m.padding),
                                                lvl.batch_size, coors.device), None, None)
                else:
                    cached = (lvl,) + lvl.strided(m.kernel_size, m.stride, m.padding)
                if m.indice_key:
                    indice_dict[m.indice_key] = cached
            lvl = cached[1]
    return IndexPlan(level0, indice_dict)


class SparseModule(nn.Module):
    """Marker base: modules that take and return a SparseConvTensor."""


class SparseSequential(SparseModule):
    def __init__(self, *args, **kwargs):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], dict):
            for k, m in args[0].items():
                self.add_module(k, m)
        else:
            for i, m in enumerate(args):
                self.add_module(str(i), m)
        for k, m in kwargs.items():
            self.add_module(k, m)

    def __getitem__(self, idx):
        return list(self._modules.values())[idx]

    def __len__(self):
        return len(self._modules)

    def add(self, module, name=None):
        self.add_module(name or str(len(self._modules)), module)

    def forward(self, x):
        mods = list(self._modules.values())
        i = 0
        while i < len(mods):
            m = mods[i]
            i += 1
            if isinstance(m, SparseModule):
                x = m(x)
            elif isinstance(x, SparseConvTensor):
                if x.features.shape[0] == 0:
                    continue
                if isinstance(m, nn.modules.batchnorm._BatchNorm) and i < len(mods) and isinstance(mods[i], nn.ReLU):
                    x = x.replace_feature(F.bn_act(x.features, m, relu=True))     # fused BN + ReLU on [N, C]
                    i += 1
                else:
                    x = x.replace_feature(m(x.features))
            else:
                x = m(x)
        return x


# Halo form of the submanifold gather-GEMM (csrc/sparse_conv.hip::sp_conv_halo_kernel; two fp16 planes) for the output widths in
# HALO_COLUMNS: 128. (The entry point also takes 64 columns - tests/test_sparse_gpu.py keeps that covered - but the product does
# not send them there: half the matrix work per gathered byte, no difference in the step, profiles/r05_sp_halo2.txt.) It walks
# all kvol offsets of every row block where the default kernel skips the offsets none of a block's 32 mask-sorted rows uses, and
# is 7 % faster than the default kernel on the 128-channel level of the shipped config (0.36 occupancy, 14.5 of 27 offsets per row).
# Round 6: OFF by default (GGA_SP_HALO=1 turns it on). The default kernel now sums every offset's products as a chain of its own
# (sp_conv_x9_kernel, `offset_sums`) and is as close to float64 as a per-offset fp32 sgemm (RMS 0.7-1.2 x, tests/test_precision_gpu.py);
# the halo form walks chunk-outer with ONE accumulator chain of cin / 32 x 27 x 6 roundings per element (4.9 x that sgemm at 128
# channels), its 128 accumulators per wave leave no registers for a second set, and ending a chain through the accumulator file
# costs ~5 vector instructions per element (measured: the compiler spills 1 000 registers; by hand 640 instructions per chain end):
# 0.8 ms of the 52 ms step bought the last rows of the precision table (profiles/r06_sparse_chain_ab.txt).
# gather_gemm.apply reads these; any rule book that carries its level's coordinates can take the form (subm_rulebook below).
HALO = int(os.environ.get('GGA_SP_HALO', '0'))
HALO_COLUMNS = (128,)
HALO_MIN_ROWS = int(os.environ.get('GGA_SP_HALO_MIN_ROWS', '65536'))
HALO_MIN_OCCUPANCY = float(os.environ.get('GGA_SP_HALO_MIN_OCCUPANCY', '0.25'))


class _SparseConvFn(torch.autograd.Function):
    """features [n_in,Cin] x weight [kvol,Cin,Cout] -> [n_out,Cout] through rule book ``rb``
    (``rb_t`` = transposed rule book for the backward-data pass, None for submanifold convs)."""

    @staticmethod
    def forward(ctx, feats, weight, rb, rb_t, n_out):
        feats, w = feats.contiguous(), weight.contiguous()
        kvol = rb.nbr.shape[0]
        cin, cout = w.shape[-2], w.shape[-1]
        planes = G.planes()
        x_amax = G.amax(feats)
        banked = cout <= 128 and w.data_ptr() == weight.data_ptr()      # the parameter itself: its operands live in the weight bank
        w_amax = None if banked else G.amax(w.detach())
        # the per-channel sums of y for the BatchNorm that follows (widths the fused BatchNorm takes)
        want_stats = cout % 4 == 0 and cout <= 128 and n_out >= 1
        res = G.apply(feats, rb, w.detach().reshape(kvol, cin, cout), n_out, planes=planes, x_amax=x_amax, w_amax=w_amax,
                      want_stats=want_stats, bank=banked)
        y, stats = res if want_stats else (res, torch.empty(0, dtype=torch.float64, device=feats.device))
        ctx.save_for_backward(feats, w)
        ctx.rb, ctx.rb_t, ctx.planes, ctx.amax, ctx.banked = rb, rb_t, planes, (x_amax, w_amax), banked
        # feats = relu(bn(.)) with this convolution as its consumer: the backward-data pass then does that BatchNorm's reduce
        from . import dense_conv
        ctx.bn_src = dense_conv.bn_source(feats, cin) if cin % 4 == 0 else None
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)     # no zero tensors (one fill launch each) for the gradients of the non-differentiable outputs
        return y, stats

    @staticmethod
    def backward(ctx, gy, _gstats=None):
        feats, w = ctx.saved_tensors
        rb, rb_t, planes = ctx.rb, ctx.rb_t, ctx.planes
        gy = gy.contiguous()
        kvol, n_out = rb.nbr.shape
        n_in = feats.shape[0]
        cin, cout = w.shape[-2], w.shape[-1]
        gx = gw = None
        x_amax, w_amax = ctx.amax
        g_amax = G.amax(gy) if planes == 2 else None        # one pass for both consumers of gy
        if ctx.needs_input_grad[0]:
            # W[k]^T: the transposed view of the parameter (from the weight bank) or of its contiguous copy (packed in place)
            wt = w.detach().reshape(kvol, cin, cout).transpose(1, 2)
            tb, flip = (rb_t, 0) if rb_t is not None else (rb, 1)     # SubM: transposed map = reversed offsets
            src = ctx.bn_src
            bn = src.part(0, cin) if src is not None else None
            gx = G.apply(gy, tb, wt, n_in, planes=planes, x_amax=g_amax, w_amax=w_amax, flip=flip, want_stats=bn is not None,
                         bank=ctx.banked, bn=bn, guard=False)
            if bn is not None:
                from . import dense_conv
                gx, st = gx
                gx._gga_bn_bwd = dense_conv.BnPartials(gx, [(0, cin, st)], tuple(p[5].data_ptr() for p in src.parts))
        if ctx.needs_input_grad[1]:
            gw = G.wgrad(feats, gy, rb.nbr, n_out, planes=planes, x_amax=x_amax, g_amax=g_amax, out=torch.empty_like(w))
        return gx, gw, None, None, None


class SparseConvolution(SparseModule):
    def __init__(self, ndim, in_channels, out_channels, kernel_size=3, stride=1, padding=0, dilation=1, groups=1,
                 bias=True, subm=False, indice_key=None, **kw):
        super().__init__()
        assert ndim == 3 and groups == 1 and _triple(dilation) == (1, 1, 1), 'only plain 3D sparse convs are on the GGA path'
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = _triple(kernel_size), _triple(stride), _triple(padding)
        self.subm, self.indice_key = subm, indice_key
        self.weight = nn.Parameter(torch.empty(*self.kernel_size, in_channels, out_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        # mmcv SparseConvolution.reset_parameters: kaiming_uniform_(a=sqrt(5)) on the 5-D weight
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in, _ = nn.init._calculate_fan_in_and_fan_out(self.weight)
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    # Checkpoint layouts (mmdet3d/ops/spconv/overwrite_spconv/write_spconv2.py:42-101): mmcv's sparse
    # convs - and this module - keep the kernel as [kz, ky, kx, Cin, Cout]; spconv 2.x modules keep
    # [Cout, kz, ky, kx, Cin] and stamp their state_dict entries with version 2. The reference
    # permutes mmcv checkpoints on their way INTO spconv 2 modules; here the opposite direction is
    # needed: a checkpoint written by a reference run on spconv 2 loads into this module.
    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        key = prefix + 'weight'
        w = state_dict.get(key)
        if w is not None and w.dim() == 5:
            mine = tuple(self.weight.shape)
            spconv2 = (mine[4],) + mine[:4]
            if (local_metadata.get('version', None) == 2 and tuple(w.shape) == spconv2) or \
                    (tuple(w.shape) == spconv2 and tuple(w.shape) != mine):
                state_dict = dict(state_dict)
                state_dict[key] = w.permute(1, 2, 3, 4, 0).contiguous()
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def spconv2_weight(self):
        """The kernel in spconv 2.x layout [Cout, kz, ky, kx, Cin] (for exporting a checkpoint to a
        reference installation that runs on spconv 2)."""
        return self.weight.detach().permute(4, 0, 1, 2, 3).contiguous()

    def _run(self, feats, w, rb, rb_t, n_out):
        y, stats = _SparseConvFn.apply(feats, w, rb, rb_t, n_out)
        if stats.numel() and self.bias is None:
            F.attach_bn_partials(y, stats)       # per-channel sums of y for the BatchNorm that follows (functional.bn_act)
        return y

    def forward(self, x):
        assert isinstance(x, SparseConvTensor)
        lvl = x._level
        w = self.weight.view(-1, self.in_channels, self.out_channels)
        empty = lambda n: x.features.new_zeros((n, self.out_channels)) + 0 * w.sum()      # keeps the graph connected
        if self.subm:
            if lvl.n == 0:
                y = empty(0)
            else:
                y = self._run(x.features, w, lvl.subm_rulebook(self.kernel_size), None, lvl.n)
            out = x.replace_feature(y)
        else:
            cached = x.indice_dict.get(self.indice_key) if self.indice_key else None
            if cached is None or cached[0] is not lvl:
                if lvl.n == 0:       # no input site (an all-empty batch): an empty level of the right shape
                    cached = (lvl, _empty_level(conv_out_shape(lvl.shape, self.kernel_size, self.stride, self.padding),
                                                lvl.batch_size, x.features.device), None, None)
                else:
                    cached = (lvl,) + lvl.strided(self.kernel_size, self.stride, self.padding)
                if self.indice_key:
                    x.indice_dict[self.indice_key] = cached
            _, out_lvl, nbr, nbr_t = cached
            y = empty(0) if out_lvl.n == 0 else self._run(x.features, w, nbr, nbr_t, out_lvl.n)
            out = SparseConvTensor(y, out_lvl.coors, out_lvl.shape, x.batch_size, _level=out_lvl)
            out.indice_dict = x.indice_dict
        if self.bias is not None:
            out = out.replace_feature(out.features + self.bias)
        return out


@CONV_LAYERS.register_module()
class SubMConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, True,
                         indice_key=indice_key)


@CONV_LAYERS.register_module()
class SparseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias,
                         indice_key=indice_key)
