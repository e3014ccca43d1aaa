"""CPU-side checks of the point-operator entry points (include/gga_hip.h "Point operators"): every one refuses null pointers
and impossible sizes before any HIP call, with a message under its own name (which also shows that the ctypes signatures line
up with the C ones up to the point of validation)."""
import pytest

from gga_amd import _lib

P = 4096            # a non-null stand-in for a device pointer; nothing here dereferences it


def _refused(rc, name, *words):
    msg = _lib.lib().gga_last_error().decode()
    assert rc == -1 and msg.startswith(name + ':'), (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_furthest_point_sample_validates():
    L, name = _lib.lib(), 'gga_furthest_point_sample'
    _refused(L.gga_furthest_point_sample(None, 2, 100, 10, 0, None, P, None), name, 'null pointer')
    _refused(L.gga_furthest_point_sample(P, 2, 100, 10, 0, None, None, None), name, 'null pointer')
    _refused(L.gga_furthest_point_sample(P, 2, 100, 101, 0, None, P, None), name, 'num_points 101 > N 100')
    _refused(L.gga_furthest_point_sample(P, 2, 100, 0, 0, None, P, None), name, 'bad sizes')
    _refused(L.gga_furthest_point_sample(P, -1, 100, 10, 0, None, P, None), name, 'bad sizes')
    _refused(L.gga_furthest_point_sample(P, 2, -5, -6, 0, None, P, None), name, 'bad sizes')
    # the any-N path keeps its running minima in `temp`
    _refused(L.gga_furthest_point_sample(P, 2, _lib.FPS_REGISTER_MAX_N + 1, 10, 0, None, P, None), name, 'temp')
    _refused(L.gga_furthest_point_sample(P, 2, 100, 10, 1, None, P, None), name, 'temp')


def test_ball_query_validates():
    L, name = _lib.lib(), 'gga_ball_query'
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        _refused(L.gga_ball_query(args[0], args[1], 2, 100, 10, 0.0, 0.3, 16, args[2], None), name, 'null pointer')
    _refused(L.gga_ball_query(P, P, 2, 100, 10, 0.0, 0.3, 0, P, None), name, 'sample_num 0 < 1')
    _refused(L.gga_ball_query(P, P, 2, -100, 10, 0.0, 0.3, 16, P, None), name, 'bad sizes')
    _refused(L.gga_ball_query(P, P, 2, 100, -10, 0.0, 0.3, 16, P, None), name, 'bad sizes')
    _refused(L.gga_ball_query(P, P, 0, 100, 10, 0.0, 0.3, 16, P, None), name, 'bad sizes')
    _refused(L.gga_ball_query(P, P, 2, 100, 10, -0.1, 0.3, 16, P, None), name, 'negative radius')
    assert L.gga_ball_query(None, None, 2, 100, 0, 0.0, 0.3, 16, None, None) == 0          # no centres: nothing to do


@pytest.mark.parametrize('name', ['gga_group_points_fwd', 'gga_group_points_bwd'])
def test_group_points_validates(name):
    fn = getattr(_lib.lib(), name)
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        _refused(fn(args[0], args[1], 2, 4, 100, 30, args[2], None), name, 'null pointer')
    _refused(fn(P, P, 2, 4, -100, 30, P, None), name, 'bad sizes')
    _refused(fn(P, P, 2, -4, 100, 30, P, None), name, 'bad sizes')
    _refused(fn(P, P, 2, 4, 100, -30, P, None), name, 'bad sizes')
    _refused(fn(P, P, 0, 4, 100, 30, P, None), name, 'bad sizes')


def test_three_nn_validates():
    L, name = _lib.lib(), 'gga_three_nn'
    for args in ((None, P, P, P), (P, None, P, P), (P, P, None, P), (P, P, P, None)):
        _refused(L.gga_three_nn(args[0], args[1], 2, 10, 5, args[2], args[3], None), name, 'null pointer')
    _refused(L.gga_three_nn(P, P, 2, 10, 2, P, P, None), name, 'm 2 < 3')
    _refused(L.gga_three_nn(P, P, 2, -10, 5, P, P, None), name, 'bad sizes')
    _refused(L.gga_three_nn(P, P, 2, 10, -5, P, P, None), name, 'bad sizes')


@pytest.mark.parametrize('name', ['gga_three_interpolate_fwd', 'gga_three_interpolate_bwd'])
def test_three_interpolate_validates(name):
    fn = getattr(_lib.lib(), name)
    for args in ((None, P, P, P), (P, None, P, P), (P, P, None, P), (P, P, P, None)):
        _refused(fn(args[0], args[1], args[2], 2, 4, 5, 10, args[3], None), name, 'null pointer')
    _refused(fn(P, P, P, 2, 4, 0, 10, P, None), name, 'bad sizes')
    _refused(fn(P, P, P, 2, 4, 5, -10, P, None), name, 'bad sizes')
    _refused(fn(P, P, P, 2, -4, 5, 10, P, None), name, 'bad sizes')


def test_query_and_group_validates():
    L, name = _lib.lib(), 'gga_query_and_group'

    def call(xyz=P, centre=P, feat=P, B=2, N=100, M=10, C=4, rmin=0.0, rmax=0.3, K=16, use_xyz=1, norm=1, idx=P, out=P):
        return L.gga_query_and_group(xyz, centre, feat, B, N, M, C, rmin, rmax, K, use_xyz, norm, 1, idx, out, None)

    for kw in (dict(xyz=None), dict(centre=None), dict(feat=None), dict(idx=None), dict(out=None)):
        _refused(call(**kw), name, 'null pointer')
    _refused(call(K=0), name, 'sample_num 0 not in 1..')
    _refused(call(K=_lib.GROUP_MAX_SAMPLES + 1), name, 'sample_num')
    _refused(call(N=-1), name, 'bad sizes')
    _refused(call(M=-1), name, 'bad sizes')
    _refused(call(C=-1), name, 'bad sizes')
    _refused(call(C=0, feat=None, use_xyz=0), name, 'neither coordinates nor features')
    _refused(call(rmax=0.0), name, 'normalize_xyz needs max_radius > 0')
    _refused(call(rmin=-1.0), name, 'negative radius')


def test_query_and_group_bwd_validates():
    L, name = _lib.lib(), 'gga_query_and_group_bwd'

    def call(gout=P, idx=P, B=2, N=100, M=10, C=4, rmax=0.3, K=16, use_xyz=1, norm=1, gx=P, gc=P, gf=P):
        return L.gga_query_and_group_bwd(gout, idx, B, N, M, C, rmax, K, use_xyz, norm, gx, gc, gf, None)

    _refused(call(gout=None), name, 'null pointer')
    _refused(call(idx=None), name, 'null pointer')
    _refused(call(gx=None, gc=None, gf=None), name, 'no gradient asked for')
    _refused(call(K=0), name, 'sample_num 0 < 1')
    _refused(call(N=-1), name, 'bad sizes')
    _refused(call(use_xyz=0, norm=0), name, 'coordinate gradients without use_xyz')
    _refused(call(C=0), name, 'feature gradient with C = 0')


def test_product_refuses_cpu_tensors():
    import torch
    from gga_amd import pointnet2
    with pytest.raises(RuntimeError, match='GPU only'):
        pointnet2.furthest_point_sample(torch.zeros(1, 8, 3), 4)
    with pytest.raises(RuntimeError, match='GPU only'):
        pointnet2.ball_query(0, 0.3, 4, torch.zeros(1, 8, 3), torch.zeros(1, 2, 3))
    with pytest.raises(NotImplementedError, match='FS'):
        pointnet2.PointsSampler([8], ['FS'], [-1])
