"""The cases of tests/test_head_loss_gpu.py on the CPU: the float64 reference alone must meet the conditions that test
asserts (share of slots left out of a gradient comparison, compared slots per edge class), and the fp32 restatement goes
through the same comparison code in the kernel's place, so the harness is exercised without a GPU."""
import numpy as np
import pytest
import torch

import _head_cases as HC

# what fp32 torch may be off from float64, in the units of HC.box_errors: anything above means the harness is measuring wrongly
SANE = 2e-3


@pytest.mark.parametrize('c', ['second', 'pp'])
def test_head_cases_are_well_conditioned(c):
    seen = {}
    for name in HC.BOX_CASES:
        case = HC.make_box_case(c, name)
        r64 = HC.reference(case, torch.float64, scales=True)
        cond = HC.conditioning(case, r64)
        print(f"{c}/{name}: live {cond['n_live']} left out {cond['share']:.4f}; PAL objects {cond['n_pal']} left out "
              f"{cond['pal_share']:.4f}; compared {cond['counts']}")
        assert cond['share'] <= HC.CAP and cond['pal_share'] <= HC.CAP, name
        for k, v in HC.MIN_COUNTS.get(name, {}).items():
            assert cond['counts'].get(k, 0) >= v, (name, k, cond['counts'])
        assert torch.isfinite(r64['losses']).all() and torch.isfinite(r64['g_pred']).all()
        e32 = HC.box_errors(HC.reference(case, torch.float32), r64, cond, case)
        print('   fp32 restatement vs float64:', {k: f'{v:.2e}' for k, v in e32.items()})
        assert max(e32.values()) < SANE, (name, e32)
        assert HC.off_cells_are_zero(r64['g_maps'], case)
        seen[name] = e32
    # the comparison code must notice a gradient that is off in one channel of one slot
    bad = HC.reference(case, torch.float32)
    s = int(np.flatnonzero(cond['live'] & ~cond['exclude'])[0])
    bad['g_pred'].view(-1, 8)[s, 4] *= 1.01
    assert HC.box_errors(bad, r64, cond, case)['grad.pred'] > 100 * seen[name]['grad.pred']


def test_empty_case_is_exactly_zero_in_the_reference():
    case = HC.empty_case('second')
    r = HC.reference(case, torch.float64)
    assert float(r['losses'].abs().sum()) == 0.0 and float(r['g_pred'].abs().sum()) == 0.0
    assert int(case['slot'].numel()) > 0


@pytest.mark.parametrize('name', [k for k in HC.FOCAL_SIZES if k != 'wrap'])
def test_focal_cases_are_well_conditioned(name):
    for positives in (True, False):
        x, t = HC.focal_case(name, positives)
        beyond, near = HC.focal_kinks(x)
        assert near.mean() <= HC.FOCAL_CAP
        if x.numel() > 1000:
            band = np.abs(np.abs(x.numpy()) - HC.X_CLAMP) < 1.0
            assert band.mean() > 0.1 and beyond.mean() > 0.5 and (t == 1).any() == positives
        for alpha, gamma in HC.FOCAL_PAIRS:
            l64, g64, npos = HC.focal_reference(x, t, alpha, gamma, 5.0, torch.float64, 0.7)
            l32, g32, _ = HC.focal_reference(x, t, alpha, gamma, 5.0, torch.float32, 0.7)
            assert (npos > 0) == positives
            assert float(g64.abs()[torch.from_numpy(beyond)].sum()) == 0.0
            e32, share = HC.focal_errors(l32, g32, l64, g64, x)
            print(name, positives, alpha, gamma, {k: f'{v:.2e}' for k, v in e32.items()}, share)
            assert max(e32.values()) < 5e-3, e32
