"""The streaming kernels of the kernel = stride transposed convolutions (gga_amd/csrc/deconv_stream.hip) against the
gather-GEMM they replace (``strided_conv.STREAM`` off): y and gx bit for bit, the BatchNorm partial sums up to summation
order, every output element written exactly once, run-to-run identical; and one whole PointPillars step with the switch on
and off."""
import copy
import os

import pytest
import torch

from conftest import REPO
from gga_amd import _lib
from gga_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (s, cin, cout, B, H, W): the three SECONDFPN forms at odd sizes (pixel tiles that end inside a row / an image / the batch),
# two 128-column blocks on both sides, one pixel (a tile that is almost all padding), a tile that straddles row and image ends
SHAPES = [(1, 64, 128, 2, 37, 45), (2, 128, 128, 2, 19, 23), (4, 256, 128, 2, 9, 11), (2, 256, 256, 1, 8, 8),
          (4, 256, 128, 1, 1, 1), (2, 128, 128, 3, 5, 33)]
_CASES = {}


def _inputs(s, cin, cout, B, H, W):
    """Seeded weight and the three inputs of a shape: plain, with zeros (a ReLU output), scaled by 2^-20; one output gradient."""
    g = torch.Generator(device='cpu').manual_seed(1000 * s + cin + cout + B * H * W)
    w = (torch.randn(cin, cout, s, s, generator=g) * (cin * s * s) ** -0.5).to(DEV)
    x = torch.randn(B, cin, H, W, generator=g)
    xs = [x, torch.relu(x), x * 2.0 ** -20]
    xs = [t.to(DEV).contiguous(memory_format=torch.channels_last) for t in xs]
    gy = torch.randn(B, cout, H * s, W * s, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    return w, xs, gy


def _run(x, w, s, gy, stream, monkeypatch):
    from gga_amd import dense_conv, strided_conv
    monkeypatch.setattr(dense_conv, 'PLANES', 2)
    monkeypatch.setattr(strided_conv, 'STREAM', stream)
    monkeypatch.setattr(strided_conv, 'STREAM_OFF', set())
    x = x.detach().requires_grad_(True)
    w = w.detach().requires_grad_(True)
    y, stats = strided_conv._Deconv.apply(x, w, s)
    y.backward(gy)
    return y.detach(), stats, x.grad, w.grad


def _case(shape, monkeypatch):
    """Gather and streaming results of every input of a shape, computed once and shared by the tests below."""
    if shape not in _CASES:
        s = shape[0]
        w, xs, gy = _inputs(*shape)
        _CASES[shape] = (w, xs, gy, [_run(x, w, s, gy, False, monkeypatch) for x in xs], [_run(x, w, s, gy, True, monkeypatch) for x in xs])
    return _CASES[shape]


@pytest.mark.parametrize('shape', SHAPES)
def test_y_and_gx_are_the_gather_path_bit_for_bit(shape, monkeypatch):
    s, cin, cout, B, H, W = shape
    w, xs, gy, gather, stream = _case(shape, monkeypatch)
    for i, ((y0, _, gx0, gw0), (y1, _, gx1, gw1)) in enumerate(zip(gather, stream)):
        assert y1.shape == (B, cout, H * s, W * s) and gx1.shape == (B, cin, H, W)
        assert y1.is_contiguous(memory_format=torch.channels_last) and gx1.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(y1, y0), (i, float((y1 - y0).abs().max()))
        assert torch.equal(gx1, gx0), (i, float((gx1 - gx0).abs().max()))
        assert torch.equal(gw1, gw0), i                   # (the weight gradient is the gather form's on both sides)
        assert bool(y1.abs().max() > 0) and bool(gx1.abs().max() > 0)
    # against float64: the two paths are equal, and they are a convolution
    ref = torch.nn.functional.conv_transpose2d(xs[0].double(), w.double(), stride=s)
    assert float((stream[0][0].double() - ref).abs().max() / ref.abs().max()) < 3e-6


@pytest.mark.parametrize('shape', SHAPES)
def test_partial_sums_total_within_summation_order_bound(shape, monkeypatch):
    """|sum stream - sum gather| <= n * 2^-52 * sum|terms| per channel, for the sums of y and of y^2 (n rows each): the
    bound any order of a float64 summation meets. Both kernels round inside a 32-row block in fp32; the streaming path
    forms the same blocks (in its kernel, or from the finished image where the blocks do not line up with its tiles)."""
    s, cin, cout, B, H, W = shape
    w, xs, gy, gather, stream = _case(shape, monkeypatch)
    n = B * H * W * s * s
    for i, ((y0, st0, _, _), (y1, st1, _, _)) in enumerate(zip(gather, stream)):
        assert st1.dtype == torch.float64 and st1.shape[1:] == (2, cout)
        assert st1.shape[0] == _lib.lib().gga_deconv_stream_tiles(B * H * W, cin, s)
        yd = y1.double()
        terms = torch.stack((yd.abs().sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))))
        diff = (st1.sum(0) - st0.sum(0)).abs()
        bound = n * 2.0 ** -52 * terms
        print(f'PARTIAL_SUMS {shape} input {i}: worst |stream - gather| / bound {float((diff / bound.clamp_min(1e-300)).max()):.3g}')
        assert bool((diff <= bound).all()), (i, float((diff / bound.clamp_min(1e-300)).max()))
        # and they are the sums
        torch.testing.assert_close(st1[:, 0].sum(0), yd.sum((0, 2, 3)), rtol=1e-6, atol=1e-3)


@pytest.mark.parametrize('shape', SHAPES)
def test_run_to_run_identical(shape, monkeypatch):
    s = shape[0]
    w, xs, gy, gather, stream = _case(shape, monkeypatch)
    for x, (y1, st1, gx1, _) in zip(xs, stream):
        y2, st2, gx2, _ = _run(x, w, s, gy, True, monkeypatch)
        assert torch.equal(y2, y1) and torch.equal(st2, st1) and torch.equal(gx2, gx1)


@pytest.mark.parametrize('shape', SHAPES)
def test_every_output_element_is_written_once(shape, monkeypatch):
    """The entry points on NaN-filled outputs (guard rows behind them stay NaN): no NaN is left inside, and the values are
    those of the autograd path."""
    from gga_amd import dense_conv, strided_conv, weight_bank
    s, cin, cout, B, H, W = shape
    w, xs, gy, gather, stream = _case(shape, monkeypatch)
    L = _lib.lib()
    x = xs[0]
    n_y, n_gx, guard = B * H * W * s * s * cout, B * H * W * cin, 4096
    ybuf = torch.full((n_y + guard,), float('nan'), device=DEV)
    gxbuf = torch.full((n_gx + guard,), float('nan'), device=DEV)
    fwd = [weight_bank.gather_operand(w.detach().permute(2, 3, 0, 1), 2, c0, c0 + 128) for c0 in range(0, cout, 128)]
    bwd = [weight_bank.gather_operand(w.detach().permute(2, 3, 1, 0), 2, c0, min(c0 + 128, cin)) for c0 in range(0, cin, 128)]
    x_amax, g_amax = dense_conv.tensor_amax(x), dense_conv.tensor_amax(gy)
    stats = torch.full((int(L.gga_deconv_stream_tiles(B * H * W, cin, s)), 2, cout), float('nan'), dtype=torch.float64, device=DEV)
    _lib.check(L.gga_deconv_stream_fwd(F._p(strided_conv._rows(x)), strided_conv._block_pointers([op for op, _ in fwd]), F._p(x_amax),
                                       F._p(fwd[0][1]), B, H, W, cin, cout, s, F._p(ybuf), F._p(stats), F._stream()), 'gga_deconv_stream_fwd')
    _lib.check(L.gga_deconv_stream_bwd(F._p(strided_conv._rows(gy)), strided_conv._block_pointers([op for op, _ in bwd]), F._p(g_amax),
                                       F._p(bwd[0][1]), B, H, W, cin, cout, s, F._p(gxbuf), F._stream()), 'gga_deconv_stream_bwd')
    assert not bool(torch.isnan(ybuf[:n_y]).any()) and bool(torch.isnan(ybuf[n_y:]).all())
    assert not bool(torch.isnan(gxbuf[:n_gx]).any()) and bool(torch.isnan(gxbuf[n_gx:]).all())
    assert not bool(torch.isnan(stats).any())
    y1, st1, gx1, _ = stream[0]
    assert torch.equal(ybuf[:n_y].view(B, H * s, W * s, cout), y1.permute(0, 2, 3, 1))
    assert torch.equal(gxbuf[:n_gx].view(B, H, W, cin), gx1.permute(0, 2, 3, 1))
    assert torch.equal(stats, st1)


def test_switch_and_forms(monkeypatch):
    """GGA_DECONV_STREAM / strided_conv.STREAM and the per-form list decide which kernels a layer runs; other widths and the
    three-plane arithmetic stay on the gather-GEMM."""
    from gga_amd import dense_conv, strided_conv
    monkeypatch.setattr(dense_conv, 'PLANES', 2)
    monkeypatch.setattr(strided_conv, 'STREAM', True)
    monkeypatch.setattr(strided_conv, 'STREAM_OFF', {(2, 'bwd')})
    assert strided_conv._stream_form(128, 128, 2, False) and not strided_conv._stream_form(128, 128, 2, True)
    assert strided_conv._stream_form(256, 128, 4, True) and strided_conv._stream_form(64, 128, 1, False)
    assert not strided_conv._stream_form(96, 128, 2, False) and not strided_conv._stream_form(128, 64, 2, False)
    assert not strided_conv._stream_form(128, 128, 5, False)
    monkeypatch.setattr(strided_conv, 'STREAM', False)
    assert not strided_conv._stream_form(128, 128, 2, False)
    monkeypatch.setattr(strided_conv, 'STREAM', True)
    monkeypatch.setattr(dense_conv, 'PLANES', 3)
    assert not strided_conv._stream_form(128, 128, 2, False)


def _pp_step(model, data, srl):
    model.zero_grad(set_to_none=True)
    feats = model.extract_feat(data['points'], None, data['img_metas'])[1]
    outs = model.pts_bbox_head(feats)
    losses = model.pts_bbox_head.loss(data['gt_bboxes_3d'], data['gt_labels_3d'], outs, data['GGA_boxes_img'], data['GGA_lidar2img'],
                                      data['GGA_init_pseudo_labels'], data['GGA_bdry_masks'], data['GGA_in_box_points'],
                                      data['img_metas'], srl=srl)
    total, _ = model._parse_losses(losses)
    total.backward()
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in losses.items()}, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None},
            {n: b.detach().clone() for n, b in model.named_buffers()})


def test_pointpillars_step_is_the_same_with_the_switch_on_and_off(monkeypatch):
    """The PointPillars step of tests/test_model_gpu.py (2 frames x 5000 points, channels-last trunk, two planes): the 18
    losses, every gradient and every buffer are equal with the streaming kernels and with the gather-GEMM. (D3's 2 x 62 x 54
    pixels are no multiple of 32: its sums come from the finished image in the gather kernel's order.)"""
    from gga_amd import Config, build_model, dense_conv, strided_conv, synthetic
    from gga_amd.cnn import to_channels_last
    monkeypatch.setattr(dense_conv, 'PLANES', 2)
    monkeypatch.setattr(strided_conv, 'STREAM_OFF', set())
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_kitti_pointpillars_config.py'))
    torch.manual_seed(1)
    base = build_model(cfg.model)
    base.train()
    with torch.no_grad():
        for th in base.pts_bbox_head.task_heads:
            for name in ('reg', 'height', 'dim', 'rot'):
                getattr(th, name)[-1].weight.mul_(0.05)
    batch = synthetic.make_batch(2, start=50, n_points=5000, pc_range=synthetic.RANGE_PP, n_obj_range=(4, 8), n_ibp_range=(10, 200))
    srl = base.pts_bbox_head.draw_srl(2)
    base.pts_middle_encoder.channels_last = True
    results = []
    for stream in (False, True):
        monkeypatch.setattr(strided_conv, 'STREAM', stream)
        model = to_channels_last(copy.deepcopy(base).to(DEV))
        data = dict(batch, points=[p.to(DEV) for p in batch['points']])
        results.append(_pp_step(model, data, srl))
    (l0, g0, b0), (l1, g1, b1) = results
    assert len(l0) == 18 and set(l0) == set(l1) and set(g0) == set(g1) and set(b0) == set(b1) and len(g0) > 100
    differing = [k for k in l0 if not torch.equal(l0[k], l1[k])] + [n for n in g0 if not torch.equal(g0[n], g1[n])] + \
        [n for n in b0 if not torch.equal(b0[n], b1[n])]
    assert not differing, differing[:10]
