"""CPU-side checks of the streaming transposed-convolution entry points (include/gga_hip.h, gga_amd/csrc/deconv_stream.hip):
bad arguments are refused before any HIP call, under the entry point's own name, and the sizing function says how many
rows of partial sums a launch writes."""
import ctypes as C

import pytest

from gga_amd import _lib

P = C.c_void_p(4096)          # a non-null stand-in for a device pointer: nothing here dereferences it


def _blocks(n=2):
    return (C.c_void_p * n)(*([4096] * n))         # host array of (stand-in) device pointers


def _fwd(x=P, blocks=None, ax=P, aw=P, B=2, h=9, w=11, cin=256, cout=128, s=4, y=P, stats=P):
    L = _lib.lib()
    rc = L.gga_deconv_stream_fwd(x, _blocks() if blocks is None else blocks, ax, aw, B, h, w, cin, cout, s, y, stats, None)
    return rc, L.gga_last_error().decode()


def _bwd(gy=P, blocks=None, ag=P, aw=P, B=2, h=9, w=11, cin=256, cout=128, s=4, gx=P):
    L = _lib.lib()
    rc = L.gga_deconv_stream_bwd(gy, _blocks() if blocks is None else blocks, ag, aw, B, h, w, cin, cout, s, gx, None)
    return rc, L.gga_last_error().decode()


@pytest.mark.parametrize('call,name,out', [(_fwd, 'gga_deconv_stream_fwd', 'y'), (_bwd, 'gga_deconv_stream_bwd', 'gx')])
def test_entry_points_refuse_bad_arguments_by_name(call, name, out):
    def refused(**kw):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(name + ':'), (kw, rc, msg)
        return msg

    first = 'x' if call is _fwd else 'gy'
    for arg in (first, 'aw', out, 'ax' if call is _fwd else 'ag'):
        assert 'null pointer' in refused(**{arg: None})
    assert 'null pointer' in refused(blocks=C.cast(None, C.c_void_p))
    assert 'null pointer' in refused(blocks=(C.c_void_p * 2)(4096, None), **({'cout': 256} if call is _fwd else {}))
    for cout in (0, 64, 96, 192, 130):
        assert 'multiple of 128' in refused(cout=cout)
    for s in (0, 5, -1):
        assert 'outside 1..4' in refused(s=s)
    for cin in (0, 32, 96, 512):
        assert 'cin' in refused(cin=cin)
    assert 'bad sizes' in refused(B=0)
    # 2^31 output rows and more: B * h * w * s * s
    assert '2^31' in refused(B=2 ** 15, h=2 ** 8, w=2 ** 8, s=1)
    assert '2^31' in refused(B=2 ** 11, h=2 ** 8, w=2 ** 8, s=4)
    assert '2^31' in refused(B=2 ** 15, h=2 ** 15, w=2 ** 15, s=4)
    if call is _bwd:
        assert '128, 256 or 512' in refused(cout=384)


def test_tile_count_of_known_shapes():
    L = _lib.lib()
    tiles = L.gga_deconv_stream_tiles
    # the three SECONDFPN layers at 16 frames: (tap, pixel tile) rows, 128 pixels per tile up to cin 128, 64 at cin 256
    assert tiles(16 * 248 * 216, 64, 1) == 16 * 248 * 216 // 128 == 6696
    assert tiles(16 * 124 * 108, 128, 2) == 4 * (16 * 124 * 108 // 128) == 4 * 1674
    assert tiles(16 * 62 * 54, 256, 4) == 16 * (16 * 62 * 54 // 64) == 16 * 837
    # a last tile that is partly padding; stride 1 never needs the pixel count to be a multiple of 32
    assert tiles(2 * 37 * 45, 64, 1) == (2 * 37 * 45 + 127) // 128 == 27
    assert tiles(64, 256, 2) == 4
    # pixel counts that are no multiple of 32 at s > 1: the sums are taken in the gather kernel's tiling, 128 fine rows each
    assert tiles(2 * 19 * 23, 128, 2) == (4 * 2 * 19 * 23 + 127) // 128 == int(L.gga_sparse_conv_apply_tiles(4 * 2 * 19 * 23))
    assert tiles(1, 256, 4) == 1
    # arguments no launch accepts
    assert tiles(0, 64, 1) == 0 and tiles(100, 96, 1) == 0 and tiles(100, 64, 5) == 0
