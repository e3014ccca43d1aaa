"""Dynamic voxelization without a GPU: construction, configs, parameter names, the restatement of
tests/_dynamic_voxel_ref.py against the reference's recorded results (tests/golden/dynamic_voxel.npz, written by
tools_dev/make_golden.py) and the argument checks of the new entry points."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _dynamic_voxel_ref as DR
from conftest import REPO
from gga_amd import Config, _lib, build_model
from gga_amd import functional as F
from gga_amd.registry import VOXEL_ENCODERS
from gga_amd.voxel_layer import Voxelization

PP_RANGE = [0, -39.68, -3, 69.12, 39.68, 1]
DV_PP_CFG = os.path.join(REPO, 'configs', 'gga', 'gga_kitti_dv_pointpillars_config.py')
DV_SECOND_CFG = os.path.join(REPO, 'configs', 'gga', 'gga_kitti_dv_config.py')


def test_dynamic_voxel_layer_constructs():
    layer = Voxelization(voxel_size=[0.16, 0.16, 4], point_cloud_range=PP_RANGE, max_num_points=-1, max_voxels=(-1, -1))
    assert layer.dynamic and layer.grid_size.tolist() == [432, 496, 1]
    assert layer.max_num_points == -1 and layer.max_voxels == (-1, -1)
    layer = Voxelization(voxel_size=[0.05, 0.05, 0.1], point_cloud_range=[0, -40, -3, 70.4, 40, 1], max_num_points=-1,
                         max_voxels=(-1, -1))
    assert layer.dynamic and layer.grid_size.tolist() == [1408, 1600, 40]
    hard = Voxelization(voxel_size=[0.16, 0.16, 4], point_cloud_range=PP_RANGE, max_num_points=32, max_voxels=(16000, 40000))
    assert not hard.dynamic and hard.grid_size.tolist() == [432, 496, 1]


@pytest.mark.parametrize('path,encoder,hard_path', [(DV_PP_CFG, 'DynamicPillarFeatureNet', 'gga_kitti_pointpillars_config.py'),
                                                    (DV_SECOND_CFG, 'DynamicSimpleVFE', 'gga_kitti_config.py')])
def test_dynamic_configs_load_and_build(path, encoder, hard_path):
    cfg = Config.fromfile(path)
    assert cfg.model.pts_voxel_layer['max_num_points'] == -1 and tuple(cfg.model.pts_voxel_layer['max_voxels']) == (-1, -1)
    assert cfg.model.pts_voxel_encoder['type'] == encoder
    model = build_model(cfg.model)
    assert model.dynamic_voxelization
    # the fused pillar front hands a device-side count on; DynamicSimpleVFE + SparseEncoder read the level sizes anyway
    assert model.front_reads_counts == (encoder == 'DynamicSimpleVFE')
    assert type(model.pts_voxel_encoder).__name__ == encoder
    # everything behind the voxel encoder is the hard config's, parameter for parameter
    hard = build_model(Config.fromfile(os.path.join(REPO, 'configs', 'gga', hard_path)).model)
    assert not hard.dynamic_voxelization
    rest = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith('pts_voxel_encoder.')}
    assert rest(model) == rest(hard)


def _build_encoders(golden):
    d = golden('dynamic_voxel')
    rng = tuple(float(v) for v in d['pc_range'])
    vs = lambda n: tuple(float(v) for v in d[f'{n}.voxel_size'])
    return d, dict(
        dpfn=VOXEL_ENCODERS.build(dict(type='DynamicPillarFeatureNet', in_channels=4, feat_channels=(64,), voxel_size=vs('dpfn'),
                                       point_cloud_range=rng)),
        vfe_max=VOXEL_ENCODERS.build(dict(type='DynamicVFE', in_channels=4, feat_channels=[32, 64], with_cluster_center=True,
                                          with_voxel_center=True, voxel_size=vs('vfe_max'), point_cloud_range=rng, mode='max')),
        vfe_avg=VOXEL_ENCODERS.build(dict(type='DynamicVFE', in_channels=4, feat_channels=[32, 64], with_cluster_center=True,
                                          with_voxel_center=True, voxel_size=vs('vfe_avg'), point_cloud_range=rng, mode='avg')),
        simple=VOXEL_ENCODERS.build(dict(type='DynamicSimpleVFE', voxel_size=vs('simple'), point_cloud_range=rng)))


def test_encoder_state_dict_keys_equal_the_reference(golden):
    d, mods = _build_encoders(golden)
    for name, m in mods.items():
        assert sorted(m.state_dict().keys()) == [str(k) for k in d[f'{name}.state_keys']], name
        for k, v in m.state_dict().items():
            assert tuple(v.shape) == d[f'{name}.init.{k}'].shape, (name, k)
    with pytest.raises(NotImplementedError):
        VOXEL_ENCODERS.build(dict(type='DynamicVFE', feat_channels=[16], fusion_layer=dict(type='PointFusion')))


def test_restatement_coors_equal_the_golden(golden):
    d = golden('dynamic_voxel')
    sizes = d['frame_sizes'].tolist()
    pts = torch.from_numpy(d['points'])
    frames = [pts[:sizes[0]], pts[sizes[0]:]]
    for name in ('dpfn', 'vfe_max', 'simple'):
        coors = DR.point_coors(frames, d[f'{name}.voxel_size'].tolist(), d['pc_range'].tolist())
        assert torch.equal(coors, torch.from_numpy(d[f'{name}.coors']))
        vm = DR.voxel_map(coors)
        assert torch.equal(vm['voxel_coors'].int(), torch.from_numpy(d[f'{name}.voxel_coors']))      # values AND order
        assert int(vm['counts'].sum()) == pts.shape[0] and int(vm['counts'].max()) > 1
        for v in (0, vm['counts'].numel() - 1):                  # order: ascending point index inside a voxel
            seg = vm['order'][vm['voxel_start'][v]:vm['voxel_start'][v + 1]]
            assert (seg[1:] > seg[:-1]).all() and (vm['point2voxel'][seg] == v).all()


@pytest.mark.parametrize('name', ['dpfn', 'vfe_max', 'vfe_avg'])
def test_restatement_reproduces_the_golden(golden, name):
    d = golden('dynamic_voxel')
    layers, stack = DR.golden_layers(d, name)
    pts, coors = torch.from_numpy(d['points']), torch.from_numpy(d[f'{name}.coors'])
    r = DR.dynamic_encoder(pts, coors, layers, d[f'{name}.voxel_size'].tolist(), d['pc_range'].tolist(), True, True,
                           mode=DR.GOLDEN_ENCODERS[name]['mode'])
    assert torch.equal(r['voxel_coors'].int(), torch.from_numpy(d[f'{name}.voxel_coors']))
    np.testing.assert_allclose(r['out'].detach().numpy(), d[f'{name}.out'], rtol=1e-4, atol=1e-4)
    r['out'].backward(torch.from_numpy(d[f'{name}.grad_out']).double())
    for i, L in enumerate(layers):
        for ours, theirs in (('weight', '0.weight'), ('gamma', '1.weight'), ('beta', '1.bias')):
            np.testing.assert_allclose(L[ours].grad.numpy(), d[f'{name}.grad.{stack}.{i}.{theirs}'], rtol=1e-4, atol=1e-4,
                                       err_msg=f'{name} layer {i} {ours}')
        np.testing.assert_allclose(r['running'][i][0].numpy(), d[f'{name}.after.{stack}.{i}.1.running_mean'], rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(r['running'][i][1].numpy(), d[f'{name}.after.{stack}.{i}.1.running_var'], rtol=1e-5)


def test_restatement_simple_vfe_and_max_backward_rule(golden):
    d = golden('dynamic_voxel')
    pts, coors = torch.from_numpy(d['points']), torch.from_numpy(d['simple.coors'])
    vm = DR.voxel_map(coors)
    out, _ = DR.scatter(pts, vm, 'avg')
    np.testing.assert_allclose(out.numpy(), d['simple.out'], rtol=1e-4, atol=1e-4)
    # a tie sends its whole gradient to the lowest point index (not split evenly, which is what index_reduce('amax') does)
    x = torch.tensor([[1.0], [3.0], [3.0], [2.0]], dtype=torch.float64, requires_grad=True)
    vm = DR.voxel_map(torch.tensor([[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 2]]))
    y, arg = DR.scatter(x, vm, 'max')
    y.sum().backward()
    assert arg.flatten().tolist() == [1, 3] and x.grad.flatten().tolist() == [0.0, 1.0, 0.0, 1.0]


def test_new_entry_points_reject_bad_arguments_without_gpu():
    L = _lib.lib()
    one = C.c_void_p(256)                # never dereferenced: the checks come before any HIP call
    offs = (C.c_int64 * 65)(*range(0, 650, 10))
    prm = F.voxel_params([0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1], 1, 1)
    assert L.gga_dynamic_voxelize(None, 4, offs, None, 2, C.byref(prm), None, None, None) == -1
    assert b'null pointer' in L.gga_last_error()
    assert L.gga_dynamic_voxelize(one, 2, offs, None, 2, C.byref(prm), one, one, None) == -1 and b'ndim' in L.gga_last_error()
    assert L.gga_dynamic_voxelize(one, 4, offs, None, 129, C.byref(prm), one, one, None) == -1 and b'batch' in L.gga_last_error()
    # 64 frames of the 41 x 1600 x 1408 grid: 5.9e9 cells do not fit the 32-bit key
    prm41 = F.voxel_params([0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1.1], 1, 1)
    assert F.voxel_grid_size(prm41) == [1408, 1600, 41]
    assert L.gga_dynamic_voxelize(one, 4, offs, None, 64, C.byref(prm41), one, one, None) == -1
    assert b'32-bit voxel key' in L.gga_last_error()
    assert L.gga_dynamic_voxel_map(one, None, 0, 10, 64, 1408, 1600, 41, one, one, one, one, one, one, 1 << 30, None) == -1
    assert b'32-bit voxel key' in L.gga_last_error()
    assert L.gga_dynamic_voxel_map(None, None, 4, 10, 1, 8, 8, 4, one, one, one, one, one, one, 1 << 30, None) == -1
    assert b'null pointer' in L.gga_last_error()
    assert L.gga_dynamic_voxel_map(None, one, 5, 10, 1, 8, 8, 4, one, one, one, one, one, one, 1 << 30, None) == -1
    assert b'3 or 4 columns' in L.gga_last_error()
    assert L.gga_dynamic_voxel_map(one, None, 0, 1 << 30, 1, 8, 8, 4, one, one, one, one, one, one, 1 << 30, None) == -1
    assert b'n_points' in L.gga_last_error()
    assert L.gga_dynamic_voxel_map_workspace_bytes(0) == 0 and L.gga_dynamic_voxel_map_workspace_bytes(1000) >= 4 * 4000
    assert L.gga_dynamic_scatter_chunk() == 256
    assert L.gga_dynamic_scatter_workspace_bytes(1000, 64) >= 2 * 4 * 2 * 64 * 4
    for ch in (0, 129):
        assert L.gga_dynamic_scatter_fwd(one, ch, 10, one, one, one, one, 10, 0, one, one, one, 1 << 20, None) == -1
        assert b'channels' in L.gga_last_error()
        assert L.gga_dynamic_scatter_bwd(one, ch, 10, one, one, one, 10, 0, one, None) == -1 and b'channels' in L.gga_last_error()
    assert L.gga_dynamic_scatter_fwd(one, 4, 10, one, one, one, one, 10, 2, one, one, one, 1 << 20, None) == -1
    assert b'mode' in L.gga_last_error()
    assert L.gga_dynamic_scatter_fwd(one, 4, 10, one, one, one, one, 11, 0, one, one, one, 1 << 20, None) == -1
    assert b'bad sizes' in L.gga_last_error()
    assert L.gga_dynamic_scatter_fwd(one, 4, 10, one, one, one, one, 10, 1, one, None, one, 1 << 20, None) == -1
    assert b'null pointer' in L.gga_last_error()
    assert L.gga_dynamic_scatter_fwd(one, 64, 1000, one, one, one, one, 10, 0, one, one, one, 16, None) == -2
    assert b'workspace' in L.gga_last_error()
    assert L.gga_dynamic_scatter_bwd(one, 4, 10, None, one, one, 10, 0, one, None) == -1 and b'null pointer' in L.gga_last_error()
    pfn = F.pfn_params((0.16, 0.16, 4), (0.08, -39.6, -1), 1e-3, 0.01, True)
    ptrs = [one] * 10
    assert L.gga_dynamic_pfn_workspace_bytes(0) == 0 and L.gga_dynamic_pfn_workspace_bytes(1000) > 0
    assert L.gga_dynamic_pfn_fwd(one, one, 100, one, one, one, one, 101, C.byref(pfn), *ptrs, 1 << 30, None) == -1
    assert b'bad sizes' in L.gga_last_error()
    assert L.gga_dynamic_pfn_fwd(None, one, 100, one, one, one, one, 100, C.byref(pfn), *ptrs, 1 << 30, None) == -1
    assert b'null pointer' in L.gga_last_error()
    assert L.gga_dynamic_pfn_fwd(one, one, 100, one, one, one, one, 100, C.byref(pfn), *ptrs, 16, None) == -2
    pfn.channels = 32
    assert L.gga_dynamic_pfn_fwd(one, one, 100, one, one, one, one, 100, C.byref(pfn), *ptrs, 1 << 30, None) == -1
    assert b'specialised' in L.gga_last_error()
    pfn.channels, pfn.training = 64, 0
    assert L.gga_dynamic_pfn_bwd(one, one, 100, one, 100, C.byref(pfn), *([one] * 11), 1 << 30, None) == -1
    assert b'training-mode' in L.gga_last_error()


def test_fused_pillar_encoder_selection(monkeypatch):
    from gga_amd import voxel_encoders as VE
    mk = lambda **kw: VOXEL_ENCODERS.build(dict(type='DynamicPillarFeatureNet', voxel_size=(0.16, 0.16, 4),
                                                point_cloud_range=tuple(PP_RANGE), **kw))
    assert mk().fusable_config()
    for kw in (dict(feat_channels=(32,)), dict(feat_channels=(64, 64)), dict(mode='avg'), dict(with_distance=True),
               dict(with_cluster_center=False), dict(in_channels=5)):
        assert not mk(**kw).fusable_config(), kw
    monkeypatch.setattr(VE, 'DYNAMIC_PFN_FUSED', False)             # GGA_DYNAMIC_PFN_FUSED=0
    assert not mk().fusable_config()
    model = build_model(Config.fromfile(DV_PP_CFG).model)
    assert model.front_reads_counts


def test_dynamic_ops_refuse_cpu_tensors():
    from gga_amd.ops import DynamicScatter
    layer = Voxelization(voxel_size=[0.5, 0.5, 0.5], point_cloud_range=[0, -2, -1, 4, 2, 1], max_num_points=-1, max_voxels=(-1, -1))
    with pytest.raises(RuntimeError, match='GPU only'):
        layer(torch.zeros(5, 4))
    with pytest.raises(RuntimeError, match='GPU only'):
        DynamicScatter([0.5, 0.5, 0.5], [0, -2, -1, 4, 2, 1], True)(torch.zeros(5, 4), torch.zeros(5, 3, dtype=torch.int32))
