"""CPU-side checks of the drop-in boundary: libgga_hip.so loads and exports every symbol
include/gga_hip.h declares (no compute calls — there is no GPU here)."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from gga_amd import _lib


def _declared_symbols():
    src = open(os.path.join(REPO, 'include', 'gga_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(gga_[a-z0-9_]+)\s*\(', src)))


def test_library_builds_and_exports_header_symbols():
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared_symbols()
    assert len(names) >= 18
    for n in names:
        assert hasattr(L, n), f'{n} declared in include/gga_hip.h but not exported'
    assert set(names) == set(_lib.SIGNATURES), 'python binding and header disagree'


def test_every_bound_entry_point_has_a_caller():
    # an entry point nothing calls is deleted, not kept as a forwarder to its successor
    import glob
    elsewhere = {
        'gga_last_error', 'gga_abi_version', 'gga_timing_begin', 'gga_timing_collect',      # called inside gga_amd/_lib.py
        'gga_dense_conv3x3_bn_bwd_pays',      # tests/test_kernels_gpu.py binds it to a local name before calling it
    }
    files = [f for pat in ('gga_amd/*.py', 'tests/*.py', 'bench.py', '__graft_entry__.py', 'tools/*.py')
             for f in glob.glob(os.path.join(REPO, pat)) if not f.endswith(os.path.join('gga_amd', '_lib.py'))]
    text = '\n'.join(open(f).read() for f in files)
    unused = [n for n in _lib.SIGNATURES if n not in elsewhere and not re.search(r'\.' + n + r'\s*[(,)]', text)]
    assert not unused, f'bound in _lib.SIGNATURES but called nowhere: {unused}'


def test_abi_version_and_grid_size():
    L = _lib.lib()
    assert L.gga_abi_version() == _lib.ABI_VERSION
    from gga_amd.functional import voxel_grid_size, voxel_params
    assert voxel_grid_size(voxel_params([0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1], 5, 16000)) == [1408, 1600, 40]
    assert voxel_grid_size(voxel_params([0.16, 0.16, 4], [0, -39.68, -3, 69.12, 39.68, 1], 32, 16000)) == [432, 496, 1]


def test_argument_validation_without_gpu():
    # invalid arguments are rejected before any HIP call, with a message
    L = _lib.lib()
    rc = L.gga_voxel_mean(None, None, 10, 5, 4, 4, None, None)
    assert rc == -1 and b'null pointer' in L.gga_last_error()
    rc = L.gga_pillar_scatter_fwd(None, None, 0, None, 1, 6, 4, 4, 0, 0, 1, 1, None)
    assert rc == -1 and b'multiple of 4' in L.gga_last_error()


def test_batchnorm_entry_points_validate_without_gpu():
    # the three BatchNorm compute entry points refuse before any HIP call, under their own names (which also shows that the
    # ctypes signatures line up with the C ones up to the point of validation)
    L = _lib.lib()
    rows, C, p = 100, 64, 4096          # p: a non-null, 16 B aligned stand-in for a device pointer; nothing here dereferences it

    def stats(x, channels, partials, n_partials, width, col):
        return L.gga_bn_stats(x, p, p, p, p, rows, channels, 1e-3, 0.01, 1, p, p, partials, n_partials, width, col, p, 1 << 30, None)

    def refused(name):
        return L.gga_last_error().decode().startswith(name + ':')

    assert stats(None, C, None, 0, 0, 0) == -1 and refused('gga_bn_stats') and 'both null' in L.gga_last_error().decode()
    assert stats(None, C, p, 0, C, 0) == -1 and refused('gga_bn_stats')                     # n_partials < 1
    assert stats(None, C, p, 8, 2 * C, C + 4) == -1 and refused('gga_bn_stats')             # partials_width < column_offset + channels
    assert 'columns' in L.gga_last_error().decode()
    assert stats(None, C, p, 8, 2 * C, -4) == -1 and refused('gga_bn_stats')                # column_offset < 0
    assert stats(p, 6, None, 0, 0, 0) == -1 and refused('gga_bn_stats') and 'channels' in L.gga_last_error().decode()
    rc = L.gga_bn_relu_fwd(p, None, p, p, p, p, rows, 6, 1e-3, 0.01, 1, 1, p, 6, p, p, None, 0, None, p, 1 << 30, None)
    assert rc == -1 and refused('gga_bn_relu_fwd')
    rc = L.gga_bn_relu_bwd(p, 6, p, p, p, p, rows, 6, 1, 1, p, None, p, p, None, p, 1 << 30, None)
    assert rc == -1 and refused('gga_bn_relu_bwd')


def test_loss_stages_validate_their_task_table_without_gpu():
    # the head-loss entry points take a gga_task_table: a null table and a task count outside 1..GGA_MAX_TASKS are rejected
    # before any HIP call, and the message names the entry point (the two workspace-size functions take no table: they are
    # plain arithmetic in n_tasks)
    import ctypes as C
    L = _lib.lib()
    prm = _lib.LossParams()
    calls = {
        'gga_focal_loss_fwd': lambda tb: L.gga_focal_loss_fwd(tb, 0.0, 4.0, 1.0, None, 0, None),
        'gga_focal_loss_bwd': lambda tb: L.gga_focal_loss_bwd(tb, 0.0, 4.0, 1.0, None),
        'gga_gather_pred_fwd': lambda tb: L.gga_gather_pred_fwd(tb, 2, 12, 20, 72, None),
        'gga_gather_pred_bwd': lambda tb: L.gga_gather_pred_bwd(tb, 2, 12, 20, 72, None),
        'gga_box_losses_fwd': lambda tb: L.gga_box_losses_fwd(tb, C.byref(prm), None, 0, None),
        'gga_box_losses_bwd': lambda tb: L.gga_box_losses_bwd(tb, 2, 12, None),
    }
    for name, call in calls.items():
        assert call(None) == -1
        assert L.gga_last_error().decode().startswith(name + ': null task table'), name
        for n in (0, _lib.MAX_TASKS + 1):
            tb = _lib.TaskTable()
            tb.n_tasks = n
            assert call(C.byref(tb)) == -1
            assert L.gga_last_error().decode().startswith(f'{name}: n_tasks {n} not in 1..{_lib.MAX_TASKS}'), (name, n)
    assert L.gga_focal_loss_workspace_bytes(4096, 3) == 3 * L.gga_focal_loss_workspace_bytes(4096, 1) > 0
    assert L.gga_box_losses_workspace_bytes(2, 12, 3) == 3 * L.gga_box_losses_workspace_bytes(2, 12, 1) == 3 * 5 * 2 * 12 * 4


def test_product_refuses_cpu_tensors():
    import torch
    from gga_amd import functional as F
    with pytest.raises(RuntimeError, match='GPU only'):
        F.voxel_mean(torch.zeros(2, 5, 4), torch.ones(2, dtype=torch.int32), 4)


def test_product_never_imports_oracle():
    # the oracle is test infrastructure; the product tree must not reference it
    for root, _, files in os.walk(os.path.join(REPO, 'gga_amd')):
        for f in files:
            if f.endswith(('.py', '.hip', '.cc', '.h')):
                txt = open(os.path.join(root, f)).read()
                assert 'import oracle' not in txt and 'from oracle' not in txt and 'gga_oracle' not in txt, f


def test_hard_voxelize_workspace_did_not_grow():
    # (batch, total points) -> bytes before the unused fourth per-point array left the workspace: one 256 B-aligned int32 per point less
    before = {(1, 0): 25856, (1, 1): 26880, (1, 65537): 7342592, (2, 40000): 3787008, (6, 87002): 7685632, (16, 320000): 30288384}
    L = _lib.lib()
    for (batch, total), old in before.items():
        new = L.gga_hard_voxelize_workspace_bytes(batch, total)
        assert new == old - (total * 4 + 255) // 256 * 256 <= old, (batch, total, new, old)
