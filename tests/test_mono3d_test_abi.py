"""CPU-side checks of the two entry points of the mono3d test run (include/gga_hip.h: ``gga_mono3d_tta_merge`` and
``gga_mono3d_collect`` in gga_amd/csrc/mono3d_test.hip): every invalid argument is refused before any HIP call, under the entry
point's own name."""
import ctypes as C

from gga_amd import _lib

P = 4096          # a non-null, 16-byte aligned stand-in for a device pointer: nothing here dereferences it


def _table(n_maps=2, n_frames=2, **entry):
    tb = _lib.Mono3dTtaTable()
    tb.n_maps, tb.n_frames = n_maps, n_frames
    for m in range(min(max(n_maps, 0), _lib.MONO3D_TTA_MAX_MAPS)):
        e = tb.map[m]
        e.src, e.dst, e.channels, e.H, e.W, e.kind = P, P, 27, 6, 10, _lib.MONO3D_TTA_REG if m == 0 else _lib.MONO3D_TTA_MEAN
    for k, v in entry.items():          # the bad value goes into the LAST entry: every entry is checked
        setattr(tb.map[n_maps - 1], k, v)
    return tb


def test_tta_merge_refuses_bad_arguments_by_name():
    L = _lib.lib()

    def refused(tb):
        rc = L.gga_mono3d_tta_merge(None if tb is None else C.byref(tb), None)
        msg = L.gga_last_error().decode()
        assert rc == -1 and msg.startswith('gga_mono3d_tta_merge:'), (rc, msg)
        return msg

    assert 'null table' in refused(None)
    for n in (0, -1, _lib.MONO3D_TTA_MAX_MAPS + 1):
        assert 'n_maps' in refused(_table(n_maps=n))
    for n in (0, -3):
        assert 'n_frames' in refused(_table(n_frames=n))
    assert 'null pointer in map 1' in refused(_table(src=None)) and 'null pointer in map 1' in refused(_table(dst=None))
    for field in ('H', 'W', 'channels'):
        for bad in (0, -2):
            assert 'must be positive' in refused(_table(**{field: bad}))
    for kind in (-1, 2, 9):
        assert 'unknown kind' in refused(_table(kind=kind))
    assert 'fewer than 7' in refused(_table(kind=_lib.MONO3D_TTA_REG, channels=6))
    assert 'fewer than 7' in refused(_table(n_maps=1, channels=2))            # (entry 0 is the REG one)
    assert _lib.MONO3D_TTA_MAX_MAPS >= 6 * 5                                    # six merged groups on five FPN levels


def _collect(rows=P, classes=P, counts=P, n_images=2, n_rows=40, n_classes=3, scores=P, stride=3, boxes=P, code=7, dir_=P, attr=P,
             boxes2d=P, max_per_img=5, out_boxes=P, out_scores=P, out_labels=P, out_dir=P, out_attr=P, out_boxes2d=P, out_count=P,
             ws=P, ws_bytes=1 << 20):
    L = _lib.lib()
    rc = L.gga_mono3d_collect(rows, classes, counts, n_images, n_rows, n_classes, scores, stride, boxes, code, dir_, attr, boxes2d,
                              max_per_img, out_boxes, out_scores, out_labels, out_dir, out_attr, out_boxes2d, out_count, ws, ws_bytes,
                              None)
    return rc, L.gga_last_error().decode()


def test_collect_refuses_bad_arguments_by_name():
    L = _lib.lib()

    def refused(**kw):
        rc, msg = _collect(**kw)
        assert rc == -1 and msg.startswith('gga_mono3d_collect:'), (kw, rc, msg)
        return msg

    for kw in (dict(n_rows=-1), dict(n_classes=0), dict(n_classes=_lib.MULTICLASS_NMS_MAX_CLASSES + 1), dict(n_images=0),
               dict(n_images=_lib.MONO3D_COLLECT_MAX_IMAGES + 1), dict(n_rows=1 << 30, n_classes=2)):
        assert 'bad sizes' in refused(**kw)
    assert 'code size' in refused(code=0) and 'code size' in refused(code=65)
    assert 'max_per_img' in refused(max_per_img=0) and 'max_per_img' in refused(max_per_img=1 << 24)
    assert 'score_stride' in refused(stride=2)
    for arg in ('counts', 'out_count', 'out_boxes', 'out_scores', 'out_labels', 'out_dir', 'out_attr'):
        assert 'null output or count pointer' in refused(**{arg: None})
    assert 'both be given' in refused(boxes2d=None) and 'both be given' in refused(out_boxes2d=None)
    for arg in ('rows', 'classes', 'scores', 'boxes', 'ws'):
        assert 'null pointer argument' in refused(**{arg: None})
    need = L.gga_mono3d_collect_workspace_bytes(40, 3, 2)
    assert need >= 40 * 3 * 4 and 'workspace' in refused(ws_bytes=need - 1)
    assert L.gga_mono3d_collect_workspace_bytes(-1, 3, 2) == 0 and L.gga_mono3d_collect_workspace_bytes(40, 0, 2) == 0
    assert L.gga_mono3d_collect_workspace_bytes(40, 3, 0) == 0
    assert L.gga_mono3d_collect_workspace_bytes(80, 3, 2) > L.gga_mono3d_collect_workspace_bytes(8, 3, 2) > 0
