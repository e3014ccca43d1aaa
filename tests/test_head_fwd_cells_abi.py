"""CPU-side checks of the entry points behind the head's forward on gathered tiles: arguments are refused before any HIP
call, with a message that names the entry point and what is wrong (no GPU needed)."""
from gga_amd import _lib


def _err(L):
    return L.gga_last_error().decode()


def test_cell_tiles_count():
    L = _lib.lib()
    assert L.gga_head_cell_tiles_count(2, 27, 72) == 2 * 3 * 3
    assert L.gga_head_cell_tiles_count(2, 13, 32) == 2 and L.gga_head_cell_tiles_count(2, 14, 33) == 2 * 2 * 2
    assert L.gga_head_cell_tiles_count(16, 248, 216) == 16 * 20 * 7
    assert L.gga_head_cell_tiles_count(0, 27, 72) == 0 and L.gga_head_cell_tiles_count(2, -1, 72) == 0


def test_cell_tiles_validates_its_arguments_without_gpu():
    L = _lib.lib()
    ptr = 0x1000                                   # never dereferenced: every call below is refused before a launch
    for sizes in ((0, 4, 27, 72), (2, 0, 27, 72), (2, 4, 0, 72), (2, 4, 27, -3)):
        assert L.gga_head_cell_tiles(ptr, *sizes, ptr, None) == -1
        assert _err(L).startswith('gga_head_cell_tiles: bad sizes'), sizes
    assert L.gga_head_cell_tiles(None, 2, 4, 27, 72, ptr, None) == -1
    assert _err(L).startswith('gga_head_cell_tiles: null index pointer')
    assert L.gga_head_cell_tiles(ptr, 2, 4, 27, 72, None, None) == -1
    assert _err(L).startswith('gga_head_cell_tiles: null tile map')


def test_fwd_tiles_validates_its_arguments_without_gpu():
    L = _lib.lib()
    p = 0x1000

    def call(x=p, xs=64, w=p, B=2, H=27, W=72, cin=64, cout=2, tiles=p, y=p):
        return L.gga_head_conv3x3_fwd_tiles(x, xs, None, w, None, B, H, W, cin, cout, tiles, y, None)

    assert call(tiles=None) == -1 and _err(L).startswith('gga_head_conv3x3_fwd_tiles: null tile map')
    for kw in (dict(x=None), dict(w=None), dict(y=None)):
        assert call(**kw) == -1 and _err(L).startswith('gga_head_conv3x3_fwd_tiles: null pointer'), kw
    assert call(B=0) == -1 and _err(L).startswith('gga_head_conv3x3_fwd_tiles: bad sizes')
    assert call(cin=32) == -1 and _err(L).startswith('gga_head_conv3x3_fwd_tiles: specialised for 64 input channels')
    assert call(cout=5) == -1 and _err(L).startswith('gga_head_conv3x3_fwd_tiles: specialised for 64 input channels')
    assert call(xs=62) == -1 and _err(L).startswith('gga_head_conv3x3_fwd_tiles: pixel stride 62')
    assert call(x=0x1004) == -1 and _err(L).startswith('gga_head_conv3x3_fwd_tiles: pixel stride')
    assert call(W=16384) == -1 and _err(L).startswith('gga_head_conv3x3_fwd_tiles: height and width must be below 16384')
    # the dense entry point keeps its messages
    assert L.gga_head_conv3x3_fwd(None, 64, None, p, None, 2, 27, 72, 64, 2, p, None) == -1
    assert _err(L).startswith('gga_head_conv3x3_fwd: null pointer')
