"""The host driver of the gather-GEMM kernels (gga_amd/gather_gemm.py: ``Rulebook``, ``apply``, ``wgrad``) called directly on
random rule books with ~30 % of the entries at -1, against float64 torch (``index_add`` of ``x[idx] @ W[k]``) - at the smallest
shapes where each branch of the driver can go wrong: one full 128-row tile plus a 2-row tail and a single row, column blocks
of 128 + 4 (the second block at a non-zero column offset of a 132-wide row), a single block, 8 offsets (mask and permutation)
and 33 (neither), both arithmetics, reversed offsets, the weight bank, the no-permutation shortcut of uniform books.

Tolerances are those of tests/test_kernels_gpu.py::test_strided_and_transposed_convs_vs_torch: values within
max(3e-6, 2 x the error of the same product in fp32 torch) of the largest reference magnitude; column sums rtol 1e-6, atol 1e-3."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_IN = 97


def _nbr(kvol, n_out, n_in, g, absent=0.3):
    nbr = torch.randint(0, n_in, (kvol, n_out), generator=g, dtype=torch.int32)
    nbr[torch.rand((kvol, n_out), generator=g) < absent] = -1
    return nbr


def _product(x, nbr, w, flip=0):
    """y[r] = sum_k x[nbr[kk][r]] @ w[k], kk = kvol - 1 - k with ``flip``, in the dtype of ``x``."""
    kvol = nbr.shape[0]
    y = x.new_zeros((nbr.shape[1], w.shape[2]))
    for k in range(kvol):
        idx = nbr[kvol - 1 - k if flip else k].long()
        ok = (idx >= 0).nonzero().squeeze(1)
        y.index_add_(0, ok, x[idx[ok]] @ w[k])
    return y


def _wgrad(x, g, nbr):
    """gw[k] = sum over rows r of x[nbr[k][r]]^T g[r], in the dtype of ``x``."""
    out = []
    for k in range(nbr.shape[0]):
        idx = nbr[k].long()
        ok = (idx >= 0).nonzero().squeeze(1)
        out.append(x[idx[ok]].t() @ g[ok])
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def _case(rows, kvol, cin, cout):
    """Operands and references of one shape, shared by both arithmetics (never written)."""
    g = torch.Generator().manual_seed(1000 * rows + 10 * kvol + cin + cout)
    nbr = _nbr(kvol, rows, N_IN, g).to(DEV)
    x = torch.randn(N_IN, cin, generator=g).to(DEV)
    w = (torch.randn(kvol, cin, cout, generator=g) * 0.1).to(DEV)
    gy = torch.randn(rows, cout, generator=g).to(DEV)
    ref = {f: (_product(x.double(), nbr, w.double(), f), _product(x, nbr, w, f)) for f in (0, 1)}
    return nbr, x, w, gy, ref, (_wgrad(x.double(), gy.double(), nbr), _wgrad(x, gy, nbr))


def _close(name, mine, ref64, ref32):
    assert mine.shape == ref64.shape and mine.dtype == torch.float32, name
    scale = float(ref64.abs().max())
    e, e32 = float((mine.double() - ref64).abs().max()) / scale, float((ref32.double() - ref64).abs().max()) / scale
    print(f'{name}: error {e:.3e}, fp32 torch {e32:.3e}')
    assert e <= max(3e-6, 2 * e32), (name, e, e32)


def _sums_match(stats, y):
    yd = y.double()
    assert stats.dtype == torch.float64 and stats.shape[1:] == (2, y.shape[1])
    torch.testing.assert_close(stats[:, 0].sum(0), yd.sum(0), rtol=1e-6, atol=1e-3)
    torch.testing.assert_close(stats[:, 1].sum(0), (yd * yd).sum(0), rtol=1e-6, atol=1e-3)


@pytest.mark.parametrize('planes', [2, 3])
@pytest.mark.parametrize('cin,cout', [(64, 64), (64, 132)])
@pytest.mark.parametrize('kvol', [8, 33])
@pytest.mark.parametrize('rows', [130, 1])
def test_apply_against_float64(rows, kvol, cin, cout, planes):
    from gga_amd import gather_gemm as G
    nbr, x, w, _, ref, _ = _case(rows, kvol, cin, cout)
    rb = G.Rulebook(nbr)
    assert (rb.mask is None) == (rb.perm is None) == (kvol > 32)
    for flip in (0, 1):
        y, stats = G.apply(x, rb, w, rows, planes=planes, flip=flip, want_stats=True)
        _close(f'y flip {flip}', y, *ref[flip])
        _sums_match(stats, y)
        # run-to-run identical (no atomics), with and without the statistics, into a buffer of the caller's
        buf = torch.full((rows, cout), float('nan'), device=DEV)
        y2 = G.apply(x, rb, w, rows, planes=planes, flip=flip, out=buf)
        assert y2 is buf and torch.equal(y2, y)
        y3, stats3 = G.apply(x, rb, w, rows, planes=planes, flip=flip, want_stats=True)
        assert torch.equal(y3, y) and torch.equal(stats3, stats)


@pytest.mark.parametrize('planes', [2, 3])
@pytest.mark.parametrize('cin,cout', [(64, 64), (132, 132)])
@pytest.mark.parametrize('kvol', [8, 33])
@pytest.mark.parametrize('rows', [130, 1])
def test_wgrad_against_float64(rows, kvol, cin, cout, planes):
    from gga_amd import gather_gemm as G
    nbr, x, _, gy, _, ref = _case(rows, kvol, cin, cout)
    gw = G.wgrad(x, gy, nbr, rows, planes=planes)
    _close('gw', gw, *ref)
    buf = torch.full((kvol, cin, cout), float('nan'), device=DEV)
    gw2 = G.wgrad(x, gy, nbr, rows, planes=planes, out=buf)
    assert gw2 is buf and torch.equal(gw2, gw)


@pytest.mark.parametrize('planes', [2, 3])
def test_uniform_book_with_and_without_the_natural_order(planes):
    """A book in which every row has the same offsets: with ``uniform_check`` it keeps the natural row order (no permutation),
    without it the rows are sorted (a stable sort of equal keys: the identity) - the same y bit for bit."""
    from gga_amd import gather_gemm as G
    rows, kvol, cin, cout = 130, 8, 64, 132
    g = torch.Generator().manual_seed(3)
    nbr = _nbr(kvol, rows, N_IN, g, absent=0.0)
    nbr[[1, 4, 6]] = -1
    nbr = nbr.to(DEV)
    x, w = torch.randn(N_IN, cin, generator=g).to(DEV), (torch.randn(kvol, cin, cout, generator=g) * 0.1).to(DEV)
    sorted_rb, natural_rb = G.Rulebook(nbr), G.Rulebook(nbr, uniform_check=True)
    assert sorted_rb.perm is not None and natural_rb.perm is None and torch.equal(sorted_rb.mask, natural_rb.mask)
    assert G.Rulebook(_case(rows, kvol, cin, cout)[0], uniform_check=True).perm is not None         # not uniform: sorted
    ya, sa = G.apply(x, sorted_rb, w, rows, planes=planes, want_stats=True)
    yb, sb = G.apply(x, natural_rb, w, rows, planes=planes, want_stats=True)
    _close('y', ya, _product(x.double(), nbr, w.double()), _product(x, nbr, w))
    assert torch.equal(ya, yb)
    _sums_match(sa, ya), _sums_match(sb, yb)


@pytest.mark.parametrize('planes', [2, 3])
@pytest.mark.parametrize('transposed', [False, True])
@pytest.mark.parametrize('cin,cout', [(64, 64), (64, 132)])
def test_banked_operand_equals_the_packed_one(cin, cout, transposed, planes):
    """``bank=True`` on a view of a parameter (the weight bank's operand and absmax) against ``bank=False`` on the same view (one
    absmax pass and one pack launch; the transposed view of one block is read in place): the same y bit for bit."""
    from gga_amd import gather_gemm as G
    rows, kvol = 130, 8
    nbr, x, w, _, ref, _ = _case(rows, kvol, cin, cout)
    param = torch.nn.Parameter(w.transpose(1, 2).contiguous() if transposed else w.clone())
    view = param.detach().transpose(1, 2) if transposed else param.detach()
    assert view.shape == w.shape and view.is_contiguous() != transposed
    rb = G.Rulebook(nbr)
    banked = G.apply(x, rb, view, rows, planes=planes, bank=True)
    packed = G.apply(x, rb, view, rows, planes=planes)
    _close('y', packed, *ref[0])
    assert torch.equal(banked, packed)
    assert torch.equal(G.apply(x, rb, view, rows, planes=planes, bank=True), banked)
