"""CPU-side checks of the group max pool's entry points (include/gga_hip.h "Point operators"), of the set abstraction / feature
propagation modules' construction (gga_amd/pointnet_modules.py, PointNet2SASSG in gga_amd/backbones.py), and of the
conditioning of the case that tests/test_pointnet_modules_gpu.py compares against float64."""
import pytest
import torch

import _pointnet_modules_ref as R
from gga_amd import _lib
from gga_amd.pointnet_modules import SA_MODULES, PointFPModule, PointSAModule, PointSAModuleMSG, build_sa_module
from gga_amd.registry import BACKBONES, build_backbone

P = 4096            # a non-null stand-in for a device pointer; nothing here dereferences it


def _refused(rc, name, *words):
    msg = _lib.lib().gga_last_error().decode()
    assert rc == -1 and msg.startswith(name + ':'), (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_group_max_fwd_validates():
    L, name = _lib.lib(), 'gga_group_max_fwd'

    def call(x=P, B=2, C=4, M=10, K=16, strides=(640, 160, 16, 1), y=P, arg=P):
        return L.gga_group_max_fwd(x, B, C, M, K, *strides, y, arg, None)

    for kw in (dict(x=None), dict(y=None), dict(arg=None)):
        _refused(call(**kw), name, 'null pointer')
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(C=-3), dict(M=0), dict(M=-7)):
        _refused(call(**kw), name, 'bad sizes')
    _refused(call(K=0), name, 'K 0 not in 1..256')
    _refused(call(K=_lib.GROUP_MAX_SAMPLES + 1), name, 'K 257 not in 1..256')
    for i in range(4):
        strides = [640, 160, 16, 1]
        strides[i] = -strides[i]
        _refused(call(strides=strides), name, 'negative stride')


def test_group_max_bwd_validates():
    L, name = _lib.lib(), 'gga_group_max_bwd'

    def call(gy=P, arg=P, B=2, C=4, M=10, K=16, strides=(640, 1, 64, 4), gx=P):
        return L.gga_group_max_bwd(gy, arg, B, C, M, K, *strides, gx, None)

    for kw in (dict(gy=None), dict(arg=None), dict(gx=None)):
        _refused(call(**kw), name, 'null pointer')
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(C=-3), dict(M=0), dict(M=-7)):
        _refused(call(**kw), name, 'bad sizes')
    _refused(call(K=0), name, 'K 0 not in 1..256')
    _refused(call(K=_lib.GROUP_MAX_SAMPLES + 1), name, 'K 257 not in 1..256')
    for i in range(4):
        strides = [640, 1, 64, 4]
        strides[i] = -strides[i]
        _refused(call(strides=strides), name, 'negative stride')


def _votenet_keys():
    # the reference's module structure: four set abstraction modules with one shared MLP (mlps.0) of three layers, two feature
    # propagation modules with an MLP of two layers; a layer is a bias-free conv and a BatchNorm2d
    layer = ['conv.weight', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var', 'bn.num_batches_tracked']
    keys = [f'SA_modules.{m}.mlps.0.layer{i}.{k}' for m in range(4) for i in range(3) for k in layer]
    return keys + [f'FP_modules.{m}.mlps.layer{i}.{k}' for m in range(2) for i in range(2) for k in layer]


def test_votenet_backbone_builds_with_the_reference_names():
    assert BACKBONES.get('PointNet2SASSG') is not None
    model = build_backbone(R.VOTENET)
    sd = model.state_dict()
    assert list(sd) == _votenet_keys()
    assert len(sd) == (4 * 3 + 2 * 2) * 6
    # widths: xyz (3) + features in front of every set abstraction MLP; interpolated + skip features in front of a propagation
    assert tuple(sd['SA_modules.0.mlps.0.layer0.conv.weight'].shape) == (64, 4, 1, 1)
    assert tuple(sd['SA_modules.1.mlps.0.layer0.conv.weight'].shape) == (128, 131, 1, 1)
    assert tuple(sd['SA_modules.3.mlps.0.layer2.conv.weight'].shape) == (256, 128, 1, 1)
    assert tuple(sd['FP_modules.0.mlps.layer0.conv.weight'].shape) == (256, 512, 1, 1)
    assert tuple(sd['FP_modules.1.mlps.layer0.conv.weight'].shape) == (256, 512, 1, 1)
    sa = model.SA_modules[1]
    assert isinstance(sa, PointSAModule) and sa.num_point == [1024]
    g = sa.groupers[0]
    assert (g.max_radius, g.min_radius, g.sample_num, g.use_xyz, g.normalize_xyz) == (0.4, 0, 32, True, True)


def test_split_point_feats():
    from gga_amd.backbones import PointNet2SASSG
    pts = torch.arange(2 * 5 * 4, dtype=torch.float32).reshape(2, 5, 4)
    xyz, feats = PointNet2SASSG._split_point_feats(pts)
    assert xyz.is_contiguous() and feats.is_contiguous()
    assert torch.equal(xyz, pts[..., :3]) and torch.equal(feats, pts[..., 3:].transpose(1, 2))
    assert PointNet2SASSG._split_point_feats(pts[..., :3])[1] is None


def test_sa_module_registry_and_refusals():
    assert SA_MODULES.get('PointSAModule') is PointSAModule and SA_MODULES.get('PointSAModuleMSG') is PointSAModuleMSG
    assert isinstance(build_sa_module(None, mlp_channels=[4, 8], num_point=4, radius=0.2, num_sample=4), PointSAModule)
    with pytest.raises(NotImplementedError, match='F-FPS'):
        PointSAModule(mlp_channels=[4, 8], num_point=4, radius=0.2, num_sample=4, fps_mod=['F-FPS'])
    with pytest.raises(NotImplementedError, match='FS'):
        PointSAModule(mlp_channels=[4, 8], num_point=4, radius=0.2, num_sample=4, fps_mod=['FS'])
    with pytest.raises(NotImplementedError, match='PAConv'):
        build_sa_module(dict(type='PAConvSAModule'), mlp_channels=[4, 8], num_point=4, radius=0.2, num_sample=4)
    with pytest.raises(KeyError):
        build_sa_module(dict(type='NoSuchModule'), mlp_channels=[4, 8])


def test_msg_module_structure():
    m = PointSAModuleMSG(num_point=8, radii=[0.2, 0.4], sample_nums=[4, 8], mlp_channels=[[1, 8], [1, 8, 16]], dilated_group=True)
    assert [(g.min_radius, g.max_radius, g.sample_num) for g in m.groupers] == [(0, 0.2, 4), (0.2, 0.4, 8)]
    assert [k for k in m.state_dict() if k.endswith('conv.weight')] == ['mlps.0.layer0.conv.weight', 'mlps.1.layer0.conv.weight',
                                                                         'mlps.1.layer1.conv.weight']
    assert tuple(m.mlps[0].layer0.conv.weight.shape) == (8, 4, 1, 1)        # use_xyz adds the three coordinate channels
    fp = PointFPModule(mlp_channels=[24, 16, 8])
    assert [k for k in fp.state_dict() if k.endswith('conv.weight')] == ['mlps.layer0.conv.weight', 'mlps.layer1.conv.weight']
    # num_point=None: no sampler, every point in one group
    whole = PointSAModule(mlp_channels=[1, 8], num_point=None)
    assert whole.points_sampler is None and type(whole.groupers[0]).__name__ == 'GroupAll'


def test_pool_restatement_follows_the_scan():
    import numpy as np
    nan, inf = np.nan, np.inf
    x = np.array([[1, 3, 3, 2], [0.0, -0.0, 0, -1], [-0.0, 0.0, -1, -1], [-inf, -inf, -inf, -inf], [1, nan, 5, nan],
                  [nan, 7, 7, 7], [2, 2, 2, 2]], np.float32)
    y, arg = R.group_max(x)
    assert arg.tolist() == [1, 0, 0, 0, 1, 0, 0] and arg.dtype == np.uint8
    assert np.array_equal(y, np.array([3, 0, -0.0, -inf, nan, nan, 2], np.float32), equal_nan=True)
    assert np.signbit(y[2]) and not np.signbit(y[1])
    gx = R.group_max_grad(np.arange(1, 8, dtype=np.float32), arg, 4)
    assert gx[0].tolist() == [0, 1, 0, 0] and gx[4].tolist() == [0, 5, 0, 0] and (gx != 0).sum() == 7


def test_group_max_pool_takes_the_eager_path_on_the_cpu():
    from gga_amd import ops, pointnet2
    assert ops.group_max_pool is pointnet2.group_max_pool
    x = torch.randn(2, 3, 5, 7, requires_grad=True)
    y = pointnet2.group_max_pool(x)
    assert y.shape == (2, 3, 5) and y.is_contiguous() and torch.equal(y, x.max(dim=3).values)
    y.sum().backward()
    assert torch.equal(x.grad.sum(dim=3), torch.ones(2, 3, 5))


def test_small_case_is_well_conditioned():
    # the two conditions under which a float32 run can be compared with the float64 restatement tensor by tensor: the float32
    # and the float64 restatement pick the same pool position wherever the pooled value is positive (where it is zero every
    # sample was cut by the ReLU and no gradient passes), and no pre-activation lies within 1e-4 of zero in units of its
    # channel's standard deviation (so no ReLU decides differently at the two precisions)
    #
    # A third condition, on the conditioning of the arithmetic itself: the plain float32 restatement stays within HALF of
    # the device comparison's bound, 0.5e-4 * max(1, max|ref|), on every compared tensor. The case has batch statistics over
    # as few as 16 values per channel, sixteen layers deep; at most seeds float32 rounding alone costs 0.5e-4 .. 5e-4 in the
    # gradients, which would leave a correct float32 device run (another summation order, the same precision) no room.
    model, points = R.small_case()
    index = R.indices_numpy(points[..., :3].numpy())
    out32, grads32 = R.run(model, points, index, torch.float32)
    out64, grads64 = R.run(model, points, index, torch.float64)
    assert len(out64['pre']) == 4 * 3 + 2 * 2 and len(out64['pool_pos']) == 4
    for p32, p64, v64 in zip(out32['pool_pos'], out64['pool_pos'], out64['pooled']):
        assert bool((v64 > 0).any())
        assert torch.equal(p32[v64 > 0], p64[v64 > 0])
    for i, pre in enumerate(out64['pre']):
        margin = pre.detach().abs() / pre.detach().std(dim=(0, 2, 3), keepdim=True)
        assert float(margin.min()) >= 1e-4, (i, float(margin.min()))
    assert len(grads64) == 48 + 1
    pairs = list(zip(out32['fp_features'] + out32['sa_features'], out64['fp_features'] + out64['sa_features']))
    pairs += [(grads32[k], grads64[k]) for k in grads64]
    for a, b in pairs:
        a, b = a.detach(), b.detach()
        assert float((a.double() - b).abs().max()) <= 0.5e-4 * max(1.0, float(b.abs().max()))
