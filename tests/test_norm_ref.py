"""tests/_norm_ref.py against float64 autograd of torch, and the conditions its input generator promises, before a kernel is
involved (CPU only)."""
import numpy as np
import pytest
import torch

import _norm_ref as N

T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    tol = 1e-11 * max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    assert float(np.abs(a - b).max()) <= tol, (what, float(np.abs(a - b).max()), tol)


@pytest.mark.parametrize('relu,res', N.BN_MODES)
@pytest.mark.parametrize('shape,training', [(s, t) for s in N.BN_SHAPES for t in (True, False)] + [(N.BN_CAPPED, True)])
def test_batchnorm_reference_vs_float64_autograd(shape, training, relu, res):
    n, C = shape
    case = N.make_bn_case(n, C, seed=n + C, relu=relu, residual=res, training=training)
    f = N.bn_case_forward(case)
    b = N.bn_backward(case['x'], case['dy'], case['gamma'], f)
    assert N.relu_margin_violations(f['pre'], f['bounds']['y']) == 0 or not relu
    eps, m = float(np.float32(case['eps'])), float(np.float32(case['momentum']))
    if training and n == 1:
        # torch refuses one row in training mode; the kernel's definition: variance 0 (biased, also into the running buffer)
        assert (f['var'] == 0).all() and (f['mean'] == case['x'][0]).all()
        _close(f['pre'], case['beta'][None].astype(np.float64) + (case['residual'] if res else 0), 'y of one row')
        _close(f['running_var'], (1 - m) * case['running_var'].astype(np.float64), 'running_var of one row')
        _close(b['dx'], 0 * b['dx'], 'dx of one row')
        return
    x, gam, bet = (T(case[k]).requires_grad_(True) for k in ('x', 'gamma', 'beta'))
    r = T(case['residual']).requires_grad_(True) if res else None
    rm, rv = T(case['running_mean']), T(case['running_var'])
    y = torch.nn.functional.batch_norm(x, rm, rv, gam, bet, training, m, eps)
    y = y + r if res else y
    y = torch.relu(y) if relu else y
    grads = torch.autograd.grad(y, [x, gam, bet] + ([r] if res else []), T(case['dy']))
    _close(f['y'], y.detach().numpy(), 'y')
    _close(f['mask'], (y.detach().numpy() > 0) if relu else np.ones(shape, bool), 'mask')
    _close(f['running_mean'], rm.numpy(), 'running_mean')
    _close(f['running_var'], rv.numpy(), 'running_var')
    _close(b['dx'], grads[0].numpy(), 'dx')
    _close(b['d_gamma'], grads[1].numpy(), 'd_gamma')
    _close(b['d_beta'], grads[2].numpy(), 'd_beta')
    if res:
        _close(b['d_residual'], grads[3].numpy(), 'd_residual')
    if training:
        _close(f['mean'], x.detach().mean(0).numpy(), 'mean')
        _close(f['var'], x.detach().var(0, unbiased=False).numpy(), 'var')
        _close(f['invstd'], 1 / np.sqrt(x.detach().var(0, unbiased=False).numpy() + eps), 'invstd')


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('shape', N.GN_SHAPES)
def test_groupnorm_reference_vs_float64_autograd(shape, relu):
    B, C, G, H, W = shape
    case = N.make_gn_case(B, C, G, H, W, seed=C + H, relu=relu)
    f = N.gn_forward(case['x'], case['gamma'], case['beta'], G, case['eps'], relu)
    b = N.gn_backward(case['x'], case['dy'], case['gamma'], f)
    nchw = lambda a: T(a).reshape(B, H, W, C).permute(0, 3, 1, 2)
    back = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, C).numpy()
    x, gam, bet = nchw(case['x']).requires_grad_(True), T(case['gamma']).requires_grad_(True), T(case['beta']).requires_grad_(True)
    y = torch.nn.functional.group_norm(x, G, gam, bet, float(np.float32(case['eps'])))
    y = torch.relu(y) if relu else y
    gx, gg, gb = torch.autograd.grad(y, [x, gam, bet], nchw(case['dy']))
    _close(f['y'], back(y.detach()), 'y')
    _close(b['dx'], back(gx), 'dx')
    _close(b['d_gamma'], gg.numpy(), 'd_gamma')
    _close(b['d_beta'], gb.numpy(), 'd_beta')


def test_column_sums_and_partial_sums():
    x = np.random.default_rng(0).standard_normal((513, 8)).astype(np.float32)
    s, e = N.column_sums(x)
    _close(s, T(x).sum(0).numpy(), 'column sums')
    assert (e > 0).all() and (e <= N.SAFETY * N.BN_RUN * N.U * np.abs(x).sum(0)).all()
    # the run weights: a capped grid with 17 elements per thread is one full run and one run of a single element
    w = N.bn_run_weights(*N.BN_FLUSH)
    assert w.shape == N.BN_FLUSH and w.max() == N.BN_RUN - 1 and w[0, 0] == N.BN_RUN - 1 and w[-1, -1] == 0
    assert N.bn_run_weights(513, 4).max() == 1 and N.bn_run_weights(256, 4).max() == 0          # two elements / one per thread
    wg = N.gn_run_weights(96 * 96, 256)
    assert wg.max() == N.GN_RUN - 1 and wg[4 * 32, 0] == 3 and N.gn_run_weights(64, 64).max() == 0
    for n_partials in (1, 127, 600):
        p = N.partial_sums(x.astype(np.float64), x.astype(np.float64) ** 2, n_partials)
        _close(p.sum(0)[0], s, 'partials fold to the sums')
        _close(p.sum(0)[1], (T(x) ** 2).sum(0).numpy(), 'partials fold to the sums of squares')


# ---------------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize('relu,res', N.BN_MODES)
@pytest.mark.parametrize('shape', N.BN_SHAPES + [N.BN_CAPPED])
def test_batchnorm_generator_excludes_no_element(shape, relu, res):
    n, C = shape
    case = N.make_bn_case(n, C, seed=n + C, relu=relu, residual=res)
    f = N.bn_case_forward(case)
    if relu:
        assert N.relu_margin_violations(f['pre'], f['bounds']['y']) == 0
        assert float(f['mask'].mean()) > 0.1 and float((~f['mask']).mean()) > 0.1 or n * C < 64        # both branches taken
    # every channel its own location and scale
    loc, scale = N.unit_loc_scale(C)
    assert len({(round(float(a), 9), float(s)) for a, s in zip(loc, scale)}) == C
    assert np.isfinite(case['x']).all() and np.isfinite(case['dy']).all() and case['x'].dtype == np.float32


def test_batchnorm_flush_case_and_eval_cases_meet_the_conditions():
    # the flush case runs without ReLU: there is no decision to protect, the generator only has to be finite and of the size
    n, C = N.BN_FLUSH
    assert n * C // 4 > 2048 * 256 * N.BN_RUN           # more float4 than a capped grid reads in one run of every thread
    case = N.make_bn_case(64, 16, seed=1, relu=True, residual=True, training=False)
    f = N.bn_case_forward(case)
    assert N.relu_margin_violations(f['pre'], f['bounds']['y']) == 0


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('shape', N.GN_SHAPES + [N.GN_FLUSH])
def test_groupnorm_generator_excludes_no_element(shape, relu):
    B, C, G, H, W = shape
    case = N.make_gn_case(B, C, G, H, W, seed=C + H, relu=relu)
    f = N.gn_forward(case['x'], case['gamma'], case['beta'], G, case['eps'], relu)
    if relu:
        assert N.relu_margin_violations(f['pre'], f['bounds']['y']) == 0
    loc, scale = N.unit_loc_scale(B * G)
    assert len({(round(float(a), 9), float(s)) for a, s in zip(loc, scale)}) == B * G


@pytest.mark.parametrize('r', N.COND_BOUNDED)
def test_conditioning_cases_meet_the_conditions(r):
    # the cases of test_conditioning_within_the_derived_bounds (tests/test_norm_edges_gpu.py), seeds included
    case = N.make_bn_case(*N.BN_COND, seed=sum(N.BN_COND), relu=True, residual=True, r=r)
    f = N.bn_case_forward(case)
    assert N.relu_margin_violations(f['pre'], f['bounds']['y']) == 0
    got = abs(float(f['mean'][1])) / float(np.sqrt(f['var'][1]))
    assert abs(got - r) <= 0.5 + 0.25 * r          # the sample statistics of 65 rows
    B, C, G, H, W = N.GN_COND
    case = N.make_gn_case(B, C, G, H, W, seed=C + H, relu=True, r=r)
    f = N.gn_forward(case['x'], case['gamma'], case['beta'], G, case['eps'], True)
    assert N.relu_margin_violations(f['pre'], f['bounds']['y']) == 0
    got = abs(float(f['mean'].reshape(-1)[1])) / float(np.sqrt(f['var'].reshape(-1)[1]))
    assert abs(got - r) <= 0.5 + 0.25 * r          # the sample statistics of 65 rows


# ---------------------------------------------------------------------------------------------------- the bounds
def _rel(bound, value):
    return float(np.max(bound)) / float(np.abs(value).max())


@pytest.mark.parametrize('r', [0.0, 1.0])
def test_derived_bounds_are_tight_where_the_problem_is_well_conditioned(r):
    """The looseness check on the derivation: r <= 1 and >= 64 rows, every bound below 1e-5 of the output's largest
    magnitude."""
    case = N.make_bn_case(*N.BN_COND, seed=sum(N.BN_COND), relu=True, residual=True, r=r)
    f = N.bn_case_forward(case)
    b = N.bn_backward(case['x'], case['dy'], case['gamma'], f)
    for k in ('mean', 'var', 'invstd', 'y', 'running_mean', 'running_var'):
        assert _rel(f['bounds'][k], f[k]) < 1e-5, (k, _rel(f['bounds'][k], f[k]))
    for k in ('dx', 'd_gamma', 'd_beta'):
        assert _rel(b['bounds'][k], b[k]) < 1e-5, (k, _rel(b['bounds'][k], b[k]))
    B, C, G, H, W = N.GN_COND
    case = N.make_gn_case(B, C, G, H, W, seed=C + H, relu=True, r=r)
    f = N.gn_forward(case['x'], case['gamma'], case['beta'], G, case['eps'], True)
    b = N.gn_backward(case['x'], case['dy'], case['gamma'], f)
    for k in ('mean', 'var', 'invstd', 'y'):
        assert _rel(f['bounds'][k], f[k]) < 1e-5, (k, _rel(f['bounds'][k], f[k]))
    for k in ('dx', 'd_gamma', 'd_beta'):
        assert _rel(b['bounds'][k], b[k]) < 1e-5, (k, _rel(b['bounds'][k], b[k]))


def test_variance_bound_has_the_documented_form():
    """e_var <= SAFETY * (3 L - 2) u (var + mean^2), and it grows with r^2."""
    rel = []
    for r in (0.0, 30.0, 1e3):
        case = N.make_bn_case(*N.BN_COND, seed=7, relu=False, r=r)
        f = N.bn_case_forward(case)
        e2 = f['var'] + f['mean'] ** 2
        assert (f['bounds']['var'] <= N.SAFETY * (3 * N.BN_RUN - 2) * N.U * e2 * (1 + 1e-6)).all()
        rel.append(float(f['bounds']['var'][1] / f['var'][1]))
    assert rel[0] < 1e-5 and 100 < rel[2] / rel[1] < 1e4
    assert N.SAFETY <= 4
