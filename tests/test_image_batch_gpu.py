"""``gga_image_batch`` (gga_amd/csrc/image_batch.hip) against the host path (``image_pipelines.DeferredImage.materialize``:
``resize_bilinear``, the flip, the channel reversal, the [3, 256] table, zero padding): integers and one lookup on both sides,
so every comparison is for equal bits. Shapes are the smallest at which the kernel can go wrong: widths that are no multiple of
the four floats a lane stores, three sizes in a batch (a real batch-max pad), a one-row image wider than one block's 1024
floats, flips on some images only, the 1:1 read and both resize directions, both storage orders. The output is pre-filled with
NaN: the kernel must write the padding too."""
import ctypes as C

import numpy as np
import pytest
import torch

from gga_amd import _lib
from gga_amd import functional as F
from gga_amd.image_pipelines import DeferredImage, PackedImages, image_batch, normalize_table

MEAN, STD = [103.530, 116.280, 123.675], [57.375, 1.0, 0.017]          # a non-trivial std, one of them far from 1


def _deferred(rng, src_hw, scale, flip, to_rgb, divisor=32, std=STD):
    img = DeferredImage(rng.integers(0, 256, (src_hw[0], src_hw[1], 3), dtype=np.uint8))
    img.dst_h, img.dst_w = max(int(src_hw[0] * scale + 0.5), 1), max(int(src_hw[1] * scale + 0.5), 1)
    img.flip, img.table, img.reverse = flip, normalize_table(MEAN, std), to_rgb
    img.pad_h, img.pad_w = -(-img.dst_h // divisor) * divisor, -(-img.dst_w // divisor) * divisor
    return img


def _launch_on_nan(images, channels_last):
    """``image_batch`` with the output pre-filled with NaN (the product hands the kernel ``torch.empty``)."""
    packed = PackedImages(images)
    n, hp, wp = len(packed), max(r[6] for r in packed.records), max(r[7] for r in packed.records)
    descs = (_lib.ImageDesc * n)()
    for k, (at, sh, sw, dh, dw, flip, _, _) in enumerate(packed.records):
        descs[k].src_offset, descs[k].src_h, descs[k].src_w, descs[k].dst_h, descs[k].dst_w, descs[k].flip = at, sh, sw, dh, dw, flip
    src = packed.buffer.to('cuda:0')
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    out = torch.full((n, 3, hp, wp), float('nan'), device='cuda:0').contiguous(memory_format=fmt)
    _lib.check(_lib.lib().gga_image_batch(src.data_ptr(), src.numel(), descs, n, src.data_ptr(), int(packed.reverse), hp, wp,
                                          F.LAYOUT_NHWC if channels_last else F.LAYOUT_NCHW, out.data_ptr(), F._stream()), 'gga_image_batch')
    torch.cuda.synchronize()
    return out


def _host(images):
    hp, wp = max(i.pad_h for i in images), max(i.pad_w for i in images)
    return torch.from_numpy(np.stack([i.materialize(hp, wp) for i in images]))


def _same_bits(got, want):
    got = got.cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32
    assert not torch.isnan(got).any(), 'part of the output was not written'
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


SIZES = [(37, 53), (40, 64), (33, 50)]


@pytest.mark.gpu
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('to_rgb', [False, True])
@pytest.mark.parametrize('scale', [1.0, 1.013, 0.8])
def test_batches_equal_the_host_path(scale, to_rgb, channels_last):
    rng = np.random.default_rng(int(scale * 1000) + 2 * to_rgb + channels_last)
    batch3 = [_deferred(rng, hw, scale, flip, to_rgb) for hw, flip in zip(SIZES, (False, True, False))]
    for images in ([batch3[1]], batch3):          # B = 1 and B = 3 (three source sizes, the middle one flipped)
        want = _host(images)
        _same_bits(_launch_on_nan(images, channels_last), want)
        got = image_batch(PackedImages(images), 'cuda:0', channels_last)          # the product's call: torch.empty output
        assert got.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        _same_bits(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize('channels_last', [False, True])
def test_batch_max_pad_and_partial_flips(channels_last):
    """Different padded sizes in one batch (divisor 4): every image is padded to the batch's largest, with zeros."""
    rng = np.random.default_rng(5)
    images = [_deferred(rng, hw, s, f, False, divisor=4) for hw, s, f in zip(SIZES, (1.0, 0.8, 1.013), (True, False, True))]
    assert len({(i.pad_h, i.pad_w) for i in images}) == 3
    want = _host(images)
    got = _launch_on_nan(images, channels_last).cpu().contiguous()
    _same_bits(got, want)
    for k, i in enumerate(images):
        assert (got[k, :, i.dst_h:, :] == 0).all() and (got[k, :, :, i.dst_w:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('width', [700, 1100])
@pytest.mark.parametrize('scale,flip', [(1.0, False), (1.0, True), (1.013, True), (0.8, False)])
def test_one_row_spanning_several_workgroups(scale, flip, width, channels_last):
    """A block covers 1024 floats of a row: 1 x 700 is 2100 floats in channels-last memory, 1 x 1100 is more than one block in
    either order."""
    rng = np.random.default_rng(11)
    img = _deferred(rng, (1, width), 1.0, flip, True, divisor=4)
    img.dst_w = int(width * scale + 0.5)
    img.pad_h, img.pad_w = 1, -(-img.dst_w // 4) * 4
    if scale == 1.0:
        assert img.pad_w * (3 if channels_last else 1) > 1024 or width == 700
    _same_bits(_launch_on_nan([img], channels_last), _host([img]))


@pytest.mark.gpu
def test_identity_table_returns_the_source_pixels():
    """With table[c][v] = v and dst == src the output is the source image itself, channel by channel."""
    rng = np.random.default_rng(3)
    img = _deferred(rng, (33, 50), 1.0, False, False, divisor=4)
    img.table = np.tile(np.arange(256, dtype=np.float32), (3, 1))
    got = _launch_on_nan([img], False).cpu().numpy()[0]
    assert np.array_equal(got[:, :33, :50], img.src.transpose(2, 0, 1).astype(np.float32))


@pytest.mark.gpu
def test_empty_batch_is_a_no_op():
    out = torch.full((4, 4), 7.0, device='cuda:0')
    rc = _lib.lib().gga_image_batch(None, 0, C.cast(None, C.POINTER(_lib.ImageDesc)), 0, None, 0, 32, 32, F.LAYOUT_NCHW, out.data_ptr(), F._stream())
    torch.cuda.synchronize()
    assert rc == 0 and (out == 7.0).all()
