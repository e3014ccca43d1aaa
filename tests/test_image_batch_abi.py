"""CPU-side checks of the two entry points of the image branch (include/gga_hip.h: ``gga_image_batch`` in
gga_amd/csrc/image_batch.hip, ``gga_kitti_format_dets_cam`` in gga_amd/csrc/kitti_format.hip): bad arguments are refused before
any HIP call, under the entry point's own name; an empty batch / run is a no-op."""
import ctypes as C

from gga_amd import _lib

P = C.c_void_p(4096)          # a non-null, 16-byte aligned stand-in for a device pointer: nothing here dereferences it
NCHW, NHWC = 0, 1


def _descs(*records):
    """(src_offset, src_h, src_w, dst_h, dst_w, flip) per image -> host array of gga_image_desc."""
    arr = (_lib.ImageDesc * max(len(records), 1))()
    for d, r in zip(arr, records):
        d.src_offset, d.src_h, d.src_w, d.dst_h, d.dst_w, d.flip = r
    return arr


def _batch(src=P, src_bytes=3072 + 40 * 64 * 3, descs=None, n=1, table=P, reverse=0, out_h=64, out_w=64, layout=NCHW, out=P):
    L = _lib.lib()
    descs = _descs((3072, 40, 64, 40, 64, 0)) if descs is None else descs
    rc = L.gga_image_batch(src, src_bytes, descs, n, table, reverse, out_h, out_w, layout, out, None)
    return rc, L.gga_last_error().decode()


def test_image_batch_refuses_bad_arguments_by_name():
    def refused(**kw):
        rc, msg = _batch(**kw)
        assert rc == -1 and msg.startswith('gga_image_batch:'), (kw, rc, msg)
        return msg

    for arg in ('src', 'table', 'out'):
        assert 'null pointer' in refused(**{arg: None})
    assert 'null pointer' in refused(descs=C.cast(None, C.POINTER(_lib.ImageDesc)))
    assert 'negative size' in refused(n=-1)
    assert 'GGA_IMAGE_BATCH_MAX' in refused(n=_lib.IMAGE_BATCH_MAX + 1)
    for layout in (-1, 2, 7):
        assert 'unknown layout' in refused(layout=layout)
    assert '16-byte aligned' in refused(out=C.c_void_p(4100))
    assert 'multiple of 4' in refused(out_w=66)
    assert 'bad sizes' in refused(out_h=0) and 'bad sizes' in refused(src_bytes=-1)
    # dst larger than out, in either direction
    assert 'larger than out' in refused(descs=_descs((3072, 40, 64, 65, 64, 0)))
    assert 'larger than out' in refused(descs=_descs((3072, 40, 64, 40, 68, 0)), out_w=64)
    # sizes below one
    for bad in ((3072, 0, 64, 40, 64, 0), (3072, 40, 0, 40, 64, 0), (3072, 40, 64, 0, 64, 0), (3072, 40, 64, 40, 0, 0)):
        assert 'bad sizes' in refused(descs=_descs(bad))
    # an offset or an extent that leaves the source buffer (the last image ends one byte past it)
    assert 'leaves the source buffer' in refused(descs=_descs((-1, 40, 64, 40, 64, 0)))
    assert 'leaves the source buffer' in refused(descs=_descs((3073, 40, 64, 40, 64, 0)))
    assert 'leaves the source buffer' in refused(descs=_descs((1 << 40, 40, 64, 40, 64, 0)))
    assert 'image 1' in refused(descs=_descs((3072, 20, 64, 20, 64, 0), (3072 + 20 * 64 * 3, 21, 64, 21, 64, 1)), n=2)


def test_image_batch_empty_batch_is_a_no_op():
    assert _batch(n=0, src=None, table=None, out=None, descs=C.cast(None, C.POINTER(_lib.ImageDesc)))[0] == 0
    assert _batch(n=0)[0] == 0
    assert _batch(n=0, layout=5)[0] == -1            # (an unknown layout is refused whatever the count)


def _cam(boxes=P, scores=P, labels=P, n_dets=10, offsets=P, n_frames=2, p2=P, hw=P, cols=P, out_labels=P, counts=P):
    L = _lib.lib()
    rc = L.gga_kitti_format_dets_cam(boxes, scores, labels, n_dets, offsets, n_frames, p2, hw, cols, out_labels, counts, None)
    return rc, L.gga_last_error().decode()


def test_kitti_format_cam_refuses_bad_arguments_by_name():
    def refused(**kw):
        rc, msg = _cam(**kw)
        assert rc == -1 and msg.startswith('gga_kitti_format_dets_cam:'), (kw, rc, msg)
        return msg

    assert 'negative size' in refused(n_dets=-1) and 'negative size' in refused(n_frames=-1)
    for arg in ('offsets', 'p2', 'hw', 'counts'):
        assert 'per-frame arrays' in refused(**{arg: None})
    for arg in ('boxes', 'scores', 'labels', 'cols', 'out_labels'):
        assert 'per-detection arrays' in refused(**{arg: None})
    assert _cam(n_frames=0, offsets=None, p2=None, hw=None, counts=None)[0] == 0          # no frames: nothing to do
