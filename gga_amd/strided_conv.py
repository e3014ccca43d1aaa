"""The stride-2 3x3 convolutions that open a ``SECOND`` stage (mmdet3d/models/backbones/second.py:49-57) and the
kernel = stride transposed convolutions of ``SECONDFPN`` (necks/second_fpn.py:52-69; stride 1 = a 1x1 product) on
the repo's own matrix kernels: forward, backward-data and weight gradient.

Over the pixel rows of a channels-last image all of them are gather-GEMMs ``y[row] = sum_k x[map[k][row]] W[k]``
with an ARITHMETIC rule book - exactly what the sparse-convolution kernels compute from a hashed one
(``gather_gemm.apply`` / ``gather_gemm.wgrad``: fp32 carried by operand planes,
deterministic weight gradient). The rule books depend on the shape only and are built once per
(batch, map size, kernel, stride, padding); rows are visited grouped by their set of valid taps, so a transposed
convolution's output rows run the one tap of their phase and border rows skip the padding taps.
Channel widths above 128 run as 128-wide column blocks (``gather_gemm``).
"""
import ctypes as C
import os

import torch
from torch import nn

from . import _lib
from . import functional as F
from . import gather_gemm as G
from ._lib import check

ENABLED = True
# The kernel = stride transposed convolutions as streaming GEMMs (csrc/deconv_stream.hip) instead of gather-GEMMs over an
# arithmetic rule book. GGA_DECONV_STREAM=0: the gather launches for all of them; STREAM_OFF: the (stride, 'fwd' | 'bwd')
# forms that stay on the gather-GEMM because their streaming launch is not faster (EXPERIMENTS.md 6s).
STREAM = os.environ.get('GGA_DECONV_STREAM', '1') != '0'
STREAM_OFF = set()
_BOOKS = {}


class _Book:
    """Rule books of a k x k / stride s / padding p convolution [B, H, W] -> [B, Ho, Wo]:
    ``fwd.nbr`` [k*k, n_out]: input pixel of (tap, output pixel) or -1; ``bwd.nbr`` [k*k, n_in]: output pixel that
    reaches the input pixel through that tap or -1. Each side is built when it is first asked for (a transposed convolution
    on the streaming kernels needs ``fwd`` alone, for its weight gradient)."""

    def __init__(self, B, H, W, k, s, p, device):
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        self.Ho, self.Wo, self.kvol = Ho, Wo, k * k
        self.n_in, self.n_out = B * H * W, B * Ho * Wo
        self._geom = (B, H, W, k, s, p, device)

    def __getattr__(self, side):
        if side not in ('fwd', 'bwd'):
            raise AttributeError(side)
        with torch.no_grad():
            # cached per shape: where every row has the same taps (kernel = stride) the natural row order is kept
            self.__dict__[side] = G.Rulebook(self._map(side), uniform_check=True)
        return self.__dict__[side]

    def _map(self, side):
        B, H, W, k, s, p, device = self._geom
        Ho, Wo = self.Ho, self.Wo
        b = torch.arange(B, device=device).view(B, 1, 1)
        oy, ox = torch.arange(Ho, device=device).view(1, Ho, 1), torch.arange(Wo, device=device).view(1, 1, Wo)
        iy_, ix_ = torch.arange(H, device=device).view(1, H, 1), torch.arange(W, device=device).view(1, 1, W)
        rows = []
        for ky in range(k):
            for kx in range(k):
                if side == 'fwd':
                    iy, ix = oy * s + ky - p, ox * s + kx - p
                    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
                    rows.append(torch.where(ok, b * (H * W) + iy * W + ix, -1).reshape(-1))
                else:
                    ny, nx = iy_ + p - ky, ix_ + p - kx
                    ok = (ny >= 0) & (nx >= 0) & (ny % s == 0) & (nx % s == 0) & (ny // s < Ho) & (nx // s < Wo)
                    rows.append(torch.where(ok, b * (Ho * Wo) + (ny // s) * Wo + nx // s, -1).reshape(-1))
        return torch.stack(rows).int().contiguous()


def book(B, H, W, k, s, p, device):
    key = (B, H, W, k, s, p, str(device))
    if key not in _BOOKS:
        with torch.no_grad():
            _BOOKS[key] = _Book(B, H, W, k, s, p, device)
    return _BOOKS[key]


def _rows(t):
    """[B, C, H, W] channels-last tensor as its [B*H*W, C] row matrix (no copy)."""
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, C)


class _StridedConv(torch.autograd.Function):
    """Conv2d(k, stride s, padding p), weight [cout, cin, k, k]."""

    @staticmethod
    def forward(ctx, x, weight, k, s, p):
        B, cin, H, W = x.shape
        bk = book(B, H, W, k, s, p, x.device)
        w = weight.detach()
        x_amax = G.amax(x)
        y, stats = G.apply(_rows(x), bk.fwd, w.permute(2, 3, 1, 0), bk.n_out, planes=G.planes(), x_amax=x_amax, want_stats=True, bank=True)
        ctx.save_for_backward(x, weight)
        ctx.geom, ctx.amax = (k, s, p), (x_amax, None)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)     # no zero tensors (one fill launch each) for the gradients of the non-differentiable outputs
        return y.view(B, bk.Ho, bk.Wo, -1).permute(0, 3, 1, 2), stats

    @staticmethod
    def backward(ctx, gy, _gstats=None):
        x, weight = ctx.saved_tensors
        k, s, p = ctx.geom
        B, cin, H, W = x.shape
        cout = weight.shape[0]
        bk = book(B, H, W, k, s, p, x.device)
        gy = gy.contiguous(memory_format=torch.channels_last)
        g_rows = _rows(gy)
        gx = gw = None
        x_amax, w_amax = ctx.amax if G.planes() == 2 else (None, None)
        g_amax = G.amax(gy)
        if ctx.needs_input_grad[0]:
            w = weight.detach()
            gx = G.apply(g_rows, bk.bwd, w.permute(2, 3, 0, 1), bk.n_in, planes=G.planes(), x_amax=g_amax, bank=True)
            gx = gx.view(B, H, W, cin).permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            gw = G.wgrad(_rows(x), g_rows, bk.fwd.nbr, bk.n_out, planes=G.planes(), x_amax=x_amax, g_amax=g_amax).view(k, k, cin, cout).permute(3, 2, 0, 1)
        return gx, gw, None, None, None


def _stream_form(cin, cout, s, backward):
    """The streaming kernels (csrc/deconv_stream.hip) take this transposed convolution: two-plane arithmetic, cout in
    128-column blocks, cin 64 / 128 / 256 (backward-data keeps a [64, cout] gradient tile in LDS: cout a power of two)."""
    if not STREAM or G.planes() != 2 or cin not in (64, 128, 256) or cout % 128 or not 1 <= s <= 4:
        return False
    form = (s, 'bwd' if backward else 'fwd')
    return form not in STREAM_OFF and (not backward or cout in (128, 256, 512))


def _block_pointers(ops):
    return (C.c_void_p * len(ops))(*[op.data_ptr() for op in ops])


def _stream_fwd(x, weight, s, x_amax, want_stats=True):
    """y [B, s*H, s*W, cout] (channels-last memory) and its BatchNorm partial sums from x [B, cin, H, W] channels-last and
    the ConvTranspose2d weight [cin, cout, s, s]: ``gga_deconv_stream_fwd``."""
    from . import dense_conv, weight_bank
    L = _lib.lib()
    B, cin, H, W = x.shape
    cout = weight.shape[1]
    w_kio = weight.detach().permute(2, 3, 0, 1)
    if dense_conv.RANGE_GUARD.armed:
        dense_conv.RANGE_GUARD.record(w_kio)
    ops = [weight_bank.gather_operand(w_kio, 2, c0, c0 + 128) for c0 in range(0, cout, 128)]
    x_amax = G.amax(x) if x_amax is None else x_amax
    y = torch.empty((B, H * s, W * s, cout), dtype=torch.float32, device=x.device)
    tiles = int(L.gga_deconv_stream_tiles(B * H * W, cin, s))
    stats = torch.empty((tiles, 2, cout), dtype=torch.float64, device=x.device) if want_stats else None
    check(L.gga_deconv_stream_fwd(F._p(_rows(x)), _block_pointers([op for op, _ in ops]), F._p(x_amax), F._p(ops[0][1]), B, H, W,
                                  cin, cout, s, F._p(y), F._p(stats), F._stream()), 'gga_deconv_stream_fwd')
    return y, stats


def _stream_bwd(gy, weight, s, g_amax):
    """gx [B, H, W, cin] (channels-last memory) from gy [B, cout, s*H, s*W] channels-last: ``gga_deconv_stream_bwd``."""
    from . import dense_conv, weight_bank
    L = _lib.lib()
    B, cout, Hs, Ws = gy.shape
    H, W = Hs // s, Ws // s
    cin = weight.shape[0]
    w_koi = weight.detach().permute(2, 3, 1, 0)
    if dense_conv.RANGE_GUARD.armed:
        dense_conv.RANGE_GUARD.record(w_koi)
    ops = [weight_bank.gather_operand(w_koi, 2, c0, min(c0 + 128, cin)) for c0 in range(0, cin, 128)]
    g_amax = G.amax(gy) if g_amax is None else g_amax
    gx = torch.empty((B, H, W, cin), dtype=torch.float32, device=gy.device)
    check(L.gga_deconv_stream_bwd(F._p(_rows(gy)), _block_pointers([op for op, _ in ops]), F._p(g_amax), F._p(ops[0][1]), B, H, W,
                                  cin, cout, s, F._p(gx), F._stream()), 'gga_deconv_stream_bwd')
    return gx


class _Deconv(torch.autograd.Function):
    """ConvTranspose2d(kernel = stride = s, no padding), weight [cin, cout, s, s]: a streaming GEMM over the coarse pixels
    (``_stream_form``), or the gather-GEMM whose rule books are those of the s x s / stride s convolution from the fine map
    to the coarse one, with the roles swapped. The weight gradient is the gather form's either way."""

    @staticmethod
    def forward(ctx, x, weight, s):
        B, cin, H, W = x.shape
        w = weight.detach()
        x_amax = G.amax(x)
        if _stream_form(cin, weight.shape[1], s, False):
            y, stats = _stream_fwd(x, weight, s, x_amax)
            ctx.save_for_backward(x, weight)
            ctx.s, ctx.amax = s, (x_amax, None)
            ctx.mark_non_differentiable(stats)
            ctx.set_materialize_grads(False)
            return y.permute(0, 3, 1, 2), stats
        bk = book(B, H * s, W * s, s, s, 0, x.device)          # fwd [s*s, n_coarse] fine pixel; bwd [s*s, n_fine] coarse pixel
        y, stats = G.apply(_rows(x), bk.bwd, w.permute(2, 3, 0, 1), bk.n_in, planes=G.planes(), x_amax=x_amax, want_stats=True, bank=True)
        ctx.save_for_backward(x, weight)
        ctx.s, ctx.amax = s, (x_amax, None)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)     # no zero tensors (one fill launch each) for the gradients of the non-differentiable outputs
        return y.view(B, H * s, W * s, -1).permute(0, 3, 1, 2), stats

    @staticmethod
    def backward(ctx, gy, _gstats=None):
        x, weight = ctx.saved_tensors
        s = ctx.s
        B, cin, H, W = x.shape
        cout = weight.shape[1]
        gy = gy.contiguous(memory_format=torch.channels_last)
        g_rows = _rows(gy)
        gx = gw = None
        x_amax, w_amax = ctx.amax if G.planes() == 2 else (None, None)
        g_amax = G.amax(gy)
        stream = _stream_form(cin, cout, s, True)
        if not stream or ctx.needs_input_grad[1]:
            bk = book(B, H * s, W * s, s, s, 0, x.device)
        if ctx.needs_input_grad[0]:
            if stream:
                gx = _stream_bwd(gy, weight, s, g_amax).permute(0, 3, 1, 2)
            else:
                w = weight.detach()
                gx = G.apply(g_rows, bk.fwd, w.permute(2, 3, 1, 0), bk.n_out, planes=G.planes(), x_amax=g_amax, bank=True)
                gx = gx.view(B, H, W, cin).permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:      # [k][cout][cin] = sum over coarse rows of gy[fine(k, row)]^T x[row]
            gw = G.wgrad(g_rows, _rows(x), bk.fwd.nbr, bk.n_out, planes=G.planes(), x_amax=g_amax, g_amax=x_amax).view(s, s, cout, cin).permute(3, 2, 0, 1)
        return gx, gw, None


def _common(m, x):
    # widths above 256 would run as many 128 x 128 blocks that each re-read their operands (measured on ResNet-101's
    # 1x1 convolutions: 1282 weight-gradient launches, 153 ms per step against MIOpen's 7): those stay with the framework
    return (ENABLED and max(m.in_channels, m.out_channels) <= 256 and m.bias is None and m.groups == 1 and m.dilation == (1, 1) and x.is_cuda and x.dtype == torch.float32
            and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and m.in_channels % 4 == 0
            and m.out_channels % 4 == 0 and x.shape[0] * x.shape[2] * x.shape[3] * max(m.stride) ** 2 < 2 ** 31)


def eligible(m, x):
    if type(m) is nn.Conv2d:
        k, s, p = m.kernel_size, m.stride, m.padding
        return (_common(m, x) and m.padding_mode == 'zeros' and k[0] == k[1] and s[0] == s[1] and p[0] == p[1] and k[0] <= 5
                and (s[0] > 1 or k[0] == 1) and isinstance(p[0], int))
    if type(m) is nn.ConvTranspose2d:
        k, s = m.kernel_size, m.stride
        return (_common(m, x) and k == s and k[0] == k[1] and k[0] <= 5 and m.padding == (0, 0) and m.output_padding == (0, 0))
    return False


def conv(x, m):
    """``m(x)`` for an eligible Conv2d / ConvTranspose2d module; the result carries the per-channel sums of its values
    (``y.bn_partials``) that ``functional.bn_act`` uses instead of a reduce pass of its own."""
    if type(m) is nn.Conv2d:
        y, stats = _StridedConv.apply(x, m.weight, m.kernel_size[0], m.stride[0], m.padding[0])
    else:
        y, stats = _Deconv.apply(x, m.weight, m.stride[0])
    F.attach_bn_partials(y, stats)
    return y
