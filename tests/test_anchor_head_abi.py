"""The anchor-head entry points refuse bad arguments before any HIP call and under their own names (no GPU here)."""
import ctypes as C

import numpy as np

from gga_amd import _lib

P = 4096        # a non-null, 16 B aligned stand-in for a device pointer; nothing here dereferences it


def refused(L, name, word=None):
    msg = L.gga_last_error().decode()
    return msg.startswith(name + ':') and (word is None or word in msg)


def params(n_groups=3, n_rot=2, num_classes=3):
    prm = _lib.AnchorParams()
    prm.n_groups, prm.n_rot, prm.num_classes, prm.assign_per_class = n_groups, n_rot, num_classes, 1
    return prm


def test_anchor_targets_validates_without_gpu():
    L = _lib.lib()
    name = 'gga_anchor_targets'
    offs = np.array([0, 2, 2, 5], np.int32)

    def call(prm=None, A=864, N=5, B=3, host=offs, anchors=P, out=P, ws=P, ws_bytes=1 << 20):
        prm = params() if prm is None else prm
        return L.gga_anchor_targets(anchors, A, C.byref(prm) if prm is not False else None, P, P, N, P,
                                    C.c_void_p(host.ctypes.data) if host is not None else None, B, out, P, P, P, P, P, P, ws,
                                    ws_bytes, None)

    assert call(prm=False) == -1 and refused(L, name, 'null params')
    for B in (0, -1, 65536):
        assert call(B=B) == -1 and refused(L, name, 'B ')
    for g in (0, _lib.ANCHOR_MAX_GROUPS + 1):
        assert call(prm=params(n_groups=g)) == -1 and refused(L, name, 'n_groups')
    assert call(prm=params(n_rot=0)) == -1 and refused(L, name, 'n_rot')
    assert call(prm=params(num_classes=0)) == -1 and refused(L, name, 'num_classes')
    assert call(A=0) == -1 and refused(L, name, 'A ')
    assert call(A=865) == -1 and refused(L, name, 'not a multiple')
    assert call(N=-1) == -1 and refused(L, name, 'N ')
    assert call(host=None) == -1 and refused(L, name, 'frame_offsets_host')
    assert call(host=np.array([0, 3, 2, 5], np.int32)) == -1 and refused(L, name, 'not monotone')
    assert call(host=np.array([-1, 2, 2, 5], np.int32)) == -1 and refused(L, name, 'frame_offsets[0]')
    assert call(N=4) == -1 and refused(L, name, 'past the 4 boxes')
    assert call(anchors=None) == -1 and refused(L, name, 'null pointer')
    assert call(out=None) == -1 and refused(L, name, 'null pointer')
    assert call(ws=None) == -1 and refused(L, name, 'null pointer')
    assert call(ws_bytes=8) == -1 and refused(L, name, 'workspace')
    assert L.gga_anchor_targets_workspace_bytes(5, 3) >= 5 * 3 * 4
    assert L.gga_anchor_targets_workspace_bytes(-1, 3) == 0 and L.gga_anchor_targets_workspace_bytes(5, 0) == 0


def loss_params(B=3, HW=144, n_anchors=6, num_classes=3, stride=(1, 1, 1), beta=1.0 / 9.0):
    prm = _lib.AnchorLossParams()
    prm.B, prm.HW, prm.n_anchors, prm.num_classes, prm.diff_rad_by_sin = B, HW, n_anchors, num_classes, 1
    for field in ('cls_stride', 'reg_stride', 'dir_stride'):
        getattr(prm, field)[:] = list(stride)
    prm.gamma, prm.alpha, prm.beta = 2.0, 0.25, beta
    return prm


def test_anchor_losses_validate_without_gpu():
    L = _lib.lib()
    ws_bytes = _lib.ANCHOR_LOSS_WORKSPACE_BYTES

    def fwd(prm, cls=P, dirp=P, out=P, ws=P, nbytes=ws_bytes):
        return L.gga_anchor_loss_fwd(C.byref(prm) if prm is not None else None, cls, P, dirp, P, P, P, P, P, P, P, out, ws, nbytes, None)

    def bwd(prm, cls=P, dirp=P, grad=P, **_):
        return L.gga_anchor_loss_bwd(C.byref(prm) if prm is not None else None, cls, P, dirp, P, P, P, P, P, P, P, P, grad, P, P, None)

    for name, call in (('gga_anchor_loss_fwd', fwd), ('gga_anchor_loss_bwd', bwd)):
        assert call(None) == -1 and refused(L, name, 'null params')
        for B in (0, 65536):
            assert call(loss_params(B=B)) == -1 and refused(L, name, 'B ')
        assert call(loss_params(HW=0)) == -1 and refused(L, name, 'HW')
        assert call(loss_params(n_anchors=0)) == -1 and refused(L, name, 'n_anchors')
        assert call(loss_params(num_classes=0)) == -1 and refused(L, name, 'num_classes')
        assert call(loss_params(beta=0.0)) == -1 and refused(L, name, 'beta')
        for k in range(3):
            s = [1, 1, 1]
            s[k] = 0
            assert call(loss_params(stride=s)) == -1 and refused(L, name, 'stride')
        assert call(loss_params(), cls=None) == -1 and refused(L, name, 'null pointer')
    assert fwd(loss_params(), out=None) == -1 and refused(L, 'gga_anchor_loss_fwd', 'null pointer')
    assert fwd(loss_params(), nbytes=ws_bytes - 1) == -1 and refused(L, 'gga_anchor_loss_fwd', 'workspace')
    assert bwd(loss_params(), grad=None) == -1 and refused(L, 'gga_anchor_loss_bwd', 'null pointer')


def test_anchor_decode_validates_without_gpu():
    L = _lib.lib()
    name = 'gga_anchor_decode'
    ones = (C.c_int64 * 3)(1, 1, 1)

    def call(inds=P, B=3, K=20, A=864, n_anchors=6, nc=3, reg_stride=ones, dirp=P, dir_stride=ones, out=P):
        return L.gga_anchor_decode(inds, B, K, P, A, n_anchors, nc, P, P, reg_stride, dirp, dir_stride, out, P, P, None)

    for B in (0, 65536):
        assert call(B=B) == -1 and refused(L, name, 'B ')
    assert call(K=0) == -1 and refused(L, name, 'K ')
    assert call(n_anchors=0) == -1 and refused(L, name, 'n_anchors')
    assert call(A=865) == -1 and refused(L, name, 'multiple')
    assert call(nc=0) == -1 and refused(L, name, 'num_classes')
    assert call(inds=None) == -1 and refused(L, name, 'null pointer')
    assert call(out=None) == -1 and refused(L, name, 'null pointer')
    assert call(reg_stride=None) == -1 and refused(L, name, 'null pointer')
    assert call(dir_stride=None) == -1 and refused(L, name, 'strides')
    assert call(reg_stride=(C.c_int64 * 3)(1, 0, 1)) == -1 and refused(L, name, 'stride')
    assert call(dir_stride=(C.c_int64 * 3)(0, 1, 1)) == -1 and refused(L, name, 'stride')
