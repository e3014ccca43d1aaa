"""bench.py's `--dump-outputs` writer (``dump_outputs``) and argument checks, on a small CPU model: every array the last
step handed its caller, in its logical layout and a float dtype; the size cap's fixed sample. CPU only."""
import os

import numpy as np
import pytest
import torch

import bench


def _stepped_run():
    """A run_workload-shaped result: a model with parameters, BatchNorm buffers and gradients in channels-last memory, and
    the step's return value (total loss and its logged terms)."""
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 32, 3), torch.nn.BatchNorm2d(32), torch.nn.Conv2d(32, 256, 1))
    model = model.to(memory_format=torch.channels_last).train()
    y = model(torch.randn(2, 3, 12, 12).to(memory_format=torch.channels_last))
    terms = dict(loss_sq=y.square().mean(), loss_abs=y.abs().mean())
    loss = terms['loss_sq'] + terms['loss_abs']
    loss.backward()
    return dict(model=model, out=dict(loss=loss, log_vars=dict(terms, loss=loss), num_samples=2))


def test_dump_writes_every_array_of_the_last_step(tmp_path):
    run = _stepped_run()
    written = bench.dump_outputs(run, str(tmp_path))
    model = run['model']
    want = {'loss', 'log_vars.loss_sq', 'log_vars.loss_abs', 'log_vars.loss'}
    want |= {'state.' + k for k in model.state_dict()} | {'grad.' + k for k, _ in model.named_parameters()}
    assert set(written) == want and sorted(os.listdir(tmp_path)) == sorted(k + '.npy' for k in want)
    for k, v in model.state_dict().items():
        a = np.load(tmp_path / f'state.{k}.npy')
        if v.is_floating_point():
            assert a.dtype == np.float32 and a.shape == tuple(v.shape) and np.array_equal(a, v.numpy())
        else:                                   # the BatchNorm counter
            assert a.dtype == np.float64 and a == float(v)
    for k, p in model.named_parameters():     # logical layout although the weights are channels-last in memory
        assert np.array_equal(np.load(tmp_path / f'grad.{k}.npy'), p.grad.contiguous().numpy())
    assert np.load(tmp_path / 'loss.npy') == np.float32(run['out']['loss'].item())
    assert np.load(tmp_path / 'log_vars.loss_abs.npy') == np.float32(run['out']['log_vars']['loss_abs'].item())


def test_dump_over_the_limit_is_a_fixed_sample(tmp_path):
    run = _stepped_run()
    full = bench.dump_outputs(run, str(tmp_path / 'full'))
    limit = 16 << 10
    a = bench.dump_outputs(run, str(tmp_path / 'a'), limit=limit)
    b = bench.dump_outputs(run, str(tmp_path / 'b'), limit=limit)
    assert a == b and set(a) == set(full)
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')) <= limit
    sampled = [k for k in full if a[k] < full[k]]
    assert sampled and all(full[k] > 4096 for k in sampled)
    for k in full:
        x, y = np.load(tmp_path / 'a' / f'{k}.npy'), np.load(tmp_path / 'b' / f'{k}.npy')
        assert np.array_equal(x, y)
        whole = np.load(tmp_path / 'full' / f'{k}.npy').reshape(-1)
        assert np.isin(x.reshape(-1), whole).all()


def test_steps_sets_the_timed_steps_and_must_be_positive():
    args = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '2', '--dump-outputs', 'out'])
    assert (args.steps, args.warmup, args.dump_outputs) == (7, 2, 'out')
    assert bench.parse_args([]).dump_outputs is None
    with pytest.raises(SystemExit):
        bench.parse_args(['--steps', '0'])


def test_full_is_off_by_default():
    assert bench.parse_args(['--gpus', '1', '--steps', '3', '--warmup', '1']).full is False
    args = bench.parse_args(['--full', '--no-pgd'])
    assert args.full and args.no_pgd and not args.no_second_trunk
