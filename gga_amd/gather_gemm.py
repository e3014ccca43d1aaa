"""Host driver of the split-plane gather-GEMM kernels (csrc/sparse_conv.hip): rule book, packed weight, apply and weight
gradient - the one place that calls them.

``y[row] = sum_k x[nbr[k][row]] W[k]`` with fp32 operands carried by 16-bit planes (``planes``: 2 = two fp16 planes of the
scaled operands, which need the operands' absmax bits; 3 = three bf16 planes) and its deterministic weight gradient. The front
ends differ only in where the rule book comes from: a hash index (``sparse.py``, ``mink.py``), the pillar coordinates
(``pillar_conv.py``) or arithmetic on the pixel rows of an image (``strided_conv.py``, ``dcn.py``). Matrices wider than 128
columns run as 128-wide column blocks (the row strides of the entry points).
"""
import torch

from . import _lib
from . import dense_conv
from . import functional as F
from ._lib import check

_NO_BN = (None, 0, None, None, None, None)


def planes():
    """Arithmetic of the split-plane kernels: 2 = two fp16 planes of the scaled operands / three partial products,
    3 = three bf16 planes / six (dense_conv.PLANES, one switch for all matrix kernels)."""
    return dense_conv.PLANES


def amax(t):
    """Absmax bits of ``t`` (left by its producer when possible, else one pass), None on the three-bf16-plane path."""
    return dense_conv.tensor_amax(t) if dense_conv.PLANES == 2 else None


def mask_order(mask, kvol):
    """Rows in ascending order of their offset mask, ties in row order: what ``torch.sort(mask, stable=True)[1].int()`` returns,
    from an LSD radix sort over the ``kvol`` mask bits (gga_sparse_mask_order, include/gga_hip.h) - the framework's stable
    sort of int32 keys is a 22-launch merge sort per rule book on this stack."""
    L = _lib.lib()
    n = int(mask.shape[0])
    order = torch.empty(n, dtype=torch.int32, device=mask.device)
    nbytes = int(L.gga_sparse_mask_order_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mask.device)
    check(L.gga_sparse_mask_order(F._p(mask), n, int(kvol), F._p(order), F._p(ws), nbytes, F._stream()), 'gga_sparse_mask_order')
    return order


class Rulebook:
    """Gather map ``nbr`` [kvol, n_rows] (-1: no input) + per-row offset bit mask + mask-sorted processing order (both None for
    kvol > 32: the mask has 32 bits)."""

    def __init__(self, nbr, coors=None, occupancy=0.0, extent=None, uniform_check=False):
        self.nbr = nbr
        kvol, n = nbr.shape
        self.mask = self.perm = None
        # submanifold rule books: the level's coordinates and the share of its grid cells that are active (halo form)
        self.coors, self.occupancy, self._halo = coors, occupancy, None
        self.extent = extent                    # (batch size, largest grid extent) of the level, for the Z-order tiling
        if kvol <= 32:
            self.mask = torch.empty(n, dtype=torch.int32, device=nbr.device)
            check(_lib.lib().gga_sparse_rowmask(F._p(nbr), n, kvol, F._p(self.mask), F._stream()), 'gga_sparse_rowmask')
            # ``uniform_check`` reads one value back to the host: for books cached per shape only, never for a per-step one
            if uniform_check and bool((self.mask == self.mask[0]).all()):
                return                          # every row has the same taps: the natural order is the best one
            # index preprocessing (once per level, shared by every conv on it): rows with the same
            # neighbour pattern become adjacent, so a 128-row tile skips the offsets none of them uses
            self.perm = mask_order(self.mask, kvol)

    def halo(self):
        if self._halo is None:
            self._halo = _Halo(self.coors, self)
        return self._halo


def _spread3(v):
    """Bits of v (< 2^16, int64) moved to every third position."""
    v = v & 0xFFFF
    v = (v | (v << 32)) & 0x1F00000000FFFF
    v = (v | (v << 16)) & 0x1F0000FF0000FF
    v = (v | (v << 8)) & 0x100F00F00F00F00F
    v = (v | (v << 4)) & 0x10C30C30C30C30C3
    v = (v | (v << 2)) & 0x1249249249249249
    return v


def morton_order(coors, batch_size=None, max_extent=None):
    """Rows of ``coors`` [n,4] (batch, z, y, x) along a Z-order curve per sample: consecutive rows are close in space.
    With the level's ``batch_size`` and largest grid extent on a device tensor: gga_sparse_morton_order (one key kernel + a radix
    sort over the bits the extent can set; int32 order) - the expression below is 17 elementwise launches and a merge sort."""
    if batch_size is not None and max_extent is not None and coors.is_cuda and coors.dtype == torch.int32 and coors.shape[0]:
        L = _lib.lib()
        c = coors.contiguous()
        n = int(c.shape[0])
        order = torch.empty(n, dtype=torch.int32, device=c.device)
        nbytes = int(L.gga_sparse_morton_order_workspace_bytes(n))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=c.device)
        check(L.gga_sparse_morton_order(F._p(c), n, int(batch_size), int(max_extent), F._p(order), F._p(ws), nbytes, F._stream()),
              'gga_sparse_morton_order')
        return order
    c = coors.long()
    key = (c[:, 0] << 48) | (_spread3(c[:, 1]) << 2) | (_spread3(c[:, 2]) << 1) | _spread3(c[:, 3])
    return torch.argsort(key)


class _Halo:
    """Tiling of a submanifold rule book for gga_sparse_conv_apply_halo (include/gga_hip.h): tiles of 256 rows in Z-order,
    each with the list of distinct input rows its entries name and the entries rewritten as positions in that list
    (gga_sparse_halo_build)."""

    def __init__(self, coors, rb):
        L = _lib.lib()
        TM = int(L.gga_sparse_halo_tile_rows())
        kvol, n = rb.nbr.shape
        dev = rb.nbr.device
        self.n_tiles = T = (n + TM - 1) // TM
        self.tile_rows = torch.full((T * TM,), -1, dtype=torch.int32, device=dev)
        self.tile_rows[:n] = morton_order(coors, *(rb.extent or (None, None))).int()
        self.capacity = kvol * TM
        self.halo_rows = torch.empty((T, self.capacity), dtype=torch.int32, device=dev)
        self.counts = torch.empty(T, dtype=torch.int32, device=dev)
        self.local_map = torch.empty((T, kvol, TM), dtype=torch.int16, device=dev)
        check(L.gga_sparse_halo_build(F._p(rb.nbr), F._p(self.tile_rows), n, T, kvol, self.capacity, F._p(self.halo_rows),
                                      F._p(self.counts), F._p(self.local_map), F._stream()), 'gga_sparse_halo_build')


def _pack(w_kio, c0, c1, planes, w_amax):
    """Columns [c0, c1) of ``w_kio`` [kvol, cin, cout] in the kernel's operand order (gga_sparse_pack_weight_planes). The
    transposed view of a contiguous [kvol, cout, cin] weight - W[k]^T for a backward-data pass - is read where it lies when it
    is one block; every other view is copied first."""
    L = _lib.lib()
    kvol, cin, cout = w_kio.shape
    wp = torch.empty(L.gga_sparse_split_weight_bytes(kvol, cin, c1 - c0) // 2, dtype=torch.int16, device=w_kio.device)
    if c1 - c0 == cout and not w_kio.is_contiguous() and w_kio.transpose(1, 2).is_contiguous():
        src, transpose = w_kio.transpose(1, 2), 1
    else:
        src, transpose = (w_kio if c1 - c0 == cout else w_kio[:, :, c0:c1]).contiguous(), 0
    check(L.gga_sparse_pack_weight_planes(F._p(src), kvol, cin, c1 - c0, transpose, planes, F._p(w_amax), F._p(wp), F._stream()),
          'gga_sparse_pack_weight_planes')
    return wp


def apply(x_rows, rb, w_kio, n_rows, *, planes, x_amax=None, w_amax=None, flip=0, want_stats=False, bank=False, bn=None, out=None,
          guard=True):
    """y [n_rows, cout] = sum_k x_rows[rb.nbr[kk]] @ w_kio[k], kk = kvol - 1 - k with ``flip`` (a submanifold book read as its
    own transpose), else k. ``w_kio``: [kvol, cin, cout]. Returns y, or (y, stats) with ``want_stats``.

    ``x_amax`` / ``w_amax``: absmax bits of the operands for ``planes`` == 2, computed here when missing (ignored on three planes).
    ``want_stats``: the f64 [workgroups, 2, cout] per-channel sums of y and y^2 for the BatchNorm that follows.
    ``bank``: ``w_kio`` is a VIEW ([kvol, cin, cout] or [k, k, cin, cout], any strides) of a parameter that lives across steps -
    its operand and absmax come from the weight bank (refreshed with all others once per optimizer step) instead of a pack +
    absmax launch per call, and the armed range guard records it here (``tensor_amax`` records the operands it measures).
    ``guard`` = False: not this launch - the sparse trunk's backward-data pass, whose forward recorded the same weight.
    ``bn`` (backward-data launches, with ``want_stats``, one column block): ``BnSource.part`` pointers of the BatchNorm + ReLU
    whose output gradient y is - y is stored masked by the ReLU and the stats are that BatchNorm's backward sums.
    ``out``: the [n_rows, cout] result buffer."""
    L = _lib.lib()
    kvol, cin, cout = (w_kio.shape[0] * w_kio.shape[1], w_kio.shape[2], w_kio.shape[3]) if w_kio.dim() == 4 else w_kio.shape
    assert bank or w_kio.dim() == 3
    assert bn is None or (want_stats and cout <= 128)
    if planes == 2:
        x_amax = dense_conv.tensor_amax(x_rows) if x_amax is None else x_amax
        if not bank:
            w_amax = dense_conv.tensor_amax(w_kio) if w_amax is None else w_amax
        elif guard and dense_conv.RANGE_GUARD.armed:
            dense_conv.RANGE_GUARD.record(w_kio.detach())
    else:
        x_amax = w_amax = None
    y = torch.empty((n_rows, cout), dtype=torch.float32, device=x_rows.device) if out is None else out
    tiles = int(L.gga_sparse_conv_apply_tiles(n_rows)) if want_stats else 0
    halo = False
    if rb.coors is not None and planes == 2:        # a submanifold book: the halo form where the sparse trunk's switch asks for it
        from . import sparse
        halo = (sparse.HALO and cin % 32 == 0 and 9 <= kvol <= 27 and cout in sparse.HALO_COLUMNS
                and n_rows >= sparse.HALO_MIN_ROWS and rb.occupancy >= sparse.HALO_MIN_OCCUPANCY)
    parts = []
    for c0 in range(0, cout, 128):
        c1 = min(c0 + 128, cout)
        if bank:
            from . import weight_bank
            wp, w_amax = weight_bank.gather_operand(w_kio, planes, *((c0, c1) if cout > 128 else ()))     # whole, or its block
        else:
            wp = _pack(w_kio, c0, c1, planes, w_amax)
        st = torch.empty((tiles, 2, c1 - c0), dtype=torch.float64, device=y.device) if want_stats else None
        if halo:
            hl = rb.halo()
            check(L.gga_sparse_conv_apply_halo(F._p(x_rows), F._p(wp), F._p(hl.tile_rows), F._p(hl.counts), hl.capacity,
                                               F._p(hl.halo_rows), F._p(hl.local_map), n_rows, hl.n_tiles, kvol, cin, cout, flip,
                                               F._p(y), cout, 2, F._p(x_amax), F._p(w_amax), F._p(st), *(bn or _NO_BN), F._stream()),
                  'gga_sparse_conv_apply_halo')
        else:
            check(L.gga_sparse_conv_apply_bn_bwd(F._p(x_rows), F._p(rb.nbr), F._p(wp), F._p(rb.perm), F._p(rb.mask), n_rows, kvol,
                                                 cin, c1 - c0, flip, y.data_ptr() + 4 * c0, cout, planes, F._p(x_amax), F._p(w_amax),
                                                 F._p(st), *(bn or _NO_BN), F._stream()), 'gga_sparse_conv_apply_bn_bwd')
        parts.append(st)
    if want_stats:
        return y, (parts[0] if len(parts) == 1 else torch.cat(parts, dim=2))
    return y


def wgrad(x_rows, g_rows, nbr, n_rows, *, planes, x_amax=None, g_amax=None, out=None):
    """gw [kvol, cin, cout] = sum over rows of x_rows[nbr[k][row]]^T g_rows[row]: the deterministic split-plane kernel in
    128 x 128 blocks. ``x_amax`` / ``g_amax``: absmax bits of the operands for ``planes`` == 2, computed here when missing."""
    if planes == 2:
        x_amax = dense_conv.tensor_amax(x_rows) if x_amax is None else x_amax
        g_amax = dense_conv.tensor_amax(g_rows) if g_amax is None else g_amax
    else:
        x_amax = g_amax = None
    L = _lib.lib()
    kvol, cin, cout = nbr.shape[0], x_rows.shape[1], g_rows.shape[1]
    gw = torch.empty((kvol, cin, cout), dtype=torch.float32, device=x_rows.device) if out is None else out
    for i0 in range(0, cin, 128):
        i1 = min(i0 + 128, cin)
        for o0 in range(0, cout, 128):
            o1 = min(o0 + 128, cout)
            whole = i1 - i0 == cin and o1 - o0 == cout
            part = gw if whole else torch.empty((kvol, i1 - i0, o1 - o0), dtype=torch.float32, device=gw.device)
            ws = F._workspace('sp_wgrad', L.gga_sparse_conv_wgrad_workspace_bytes(n_rows, kvol, i1 - i0, o1 - o0), gw.device)
            check(L.gga_sparse_conv_wgrad_planes(x_rows.data_ptr() + 4 * i0, cin, g_rows.data_ptr() + 4 * o0, cout, F._p(nbr),
                                                 n_rows, kvol, i1 - i0, o1 - o0, F._p(part), planes, F._p(x_amax), F._p(g_amax),
                                                 F._p(ws), ws.numel(), F._stream()), 'gga_sparse_conv_wgrad_planes')
            if not whole:
                gw[:, i0:i1, o0:o1] = part
    return gw
