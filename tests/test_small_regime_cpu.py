"""CPU: the input guard of tests/test_gpu_small_regime.py, on the fp64 oracle alone.

The GPU module judges an lml gradient relative to its largest entry.  A chunk of eight length-scale sums that small_eval_body's
pass B dropped or published at another chunk's offset would pass such a comparison if the chunk's entries were small, or if
the noise / amplitude lead towered over every length-scale entry.  So for the very inputs of the GPU cases
(tests/small_regime_cases.py), in both noise regimes:

- every group of eight length-scale entries of the lml gradient holds an entry of at least 1e-2 of the gradient's scale
  max(1, max |grad|) -- the threshold of tests/test_feature_counts_cpu.py's f32 guard, here for both element types;
- the lead's largest entry is at most 1e2 x the largest length-scale entry;
- every f32 fit box keeps cond(K) <= 12801 at its worst corner (largest amplitude, smallest noise, longest length scales), from
  the eigenvalues: the f32 oracle has digits everywhere the optimiser can go;
- the rotation of orders covers every (nu, element type) x {ragged d, full chunk}.

With one row there is no pair of rows: the length-scale entries are exactly zero, which is what the device must return; those
cases (n = 1) are checked for that and carry no group guard.

A case that fails here gets another data seed (small_regime_cases.DATA_SEED), not another guard."""
import numpy as np
import pytest

import small_regime_cases as SC
from oracle import gpr_oracle as O

GROUP_BAR = 1e-2
LEAD_BAR = 1e2


def test_the_tables_are_the_grid():
    assert SC.D_SMALL == (1, 8, 9, 13, 16, 17, 24, 25, 31, 32) and SC.D_CONTROL == 33
    assert SC.N_SMALL == (1, 17, 63, 64, 65, 100, 127, 128)
    for dtype in SC.DTYPES:
        cases = SC.eval_cases(dtype)
        assert len(cases) == 2 * len(SC.D_SMALL) == len(set(cases))
        assert {c[0] for c in cases} == set(SC.D_SMALL)
        assert {c[1] for c in cases} == set(SC.N_SMALL)  # every tile edge occurs
        for nu in SC.NUS:
            assert any(d in SC.RAGGED_D and v == nu for d, _, v in cases), (dtype, nu, "no ragged d")
            assert any(d in SC.FULL_D and v == nu for d, _, v in cases), (dtype, nu, "no full chunk")
    for d in SC.D_SMALL:  # and every d meets all four orders over its two row counts and two element types
        assert {SC.nu_of(d, j, t) for j in (0, 1) for t in SC.DTYPES} == set(SC.NUS)
    fits = SC.FIT_CASES
    f64 = [c for c in fits if c[3] == np.float64 and not c[4]]
    f32 = [c for c in fits if c[3] == np.float32]
    assert {(c[0], c[2]) for c in f64} == {(d, nu) for d in SC.FIT_D for nu in SC.NUS} and len(f64) == 20
    assert len(f32) == 10 and {c[0] for c in f32} == set(SC.FIT_D) and {c[2] for c in f32} == set(SC.NUS)
    assert {c[:3] for c in f32} <= {c[:3] for c in f64}
    assert {c[1] for c in fits} == set(SC.FIT_N)
    assert [c for c in fits if c[4]] == [(17, 100, 1.5, np.float64, True)]
    assert SC.FIT_CONTROL[:2] == (33, 90)
    assert {c[0] + 2 for c in SC.LONG_FIT_CASES} == {11, 19, 27, 34} and {c[3] for c in SC.LONG_FIT_CASES} == set(SC.DTYPES)


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=lambda t: np.dtype(t).name)
def test_no_chunk_of_the_lml_gradient_is_small_and_no_lead_towers(dtype):
    worst_group, worst_lead = np.inf, 0.0
    for d, n, nu in SC.eval_cases(dtype) + [SC.CONTROL_CASE]:
        X, y, theta = SC.inputs(d, n, dtype)
        v = np.exp(theta)
        grad = np.abs(O.lml_with_gradient(X.astype(np.float64), y.astype(np.float64), v[0], v[1], v[2:], nu)["grad"])
        if n == 1:
            assert not grad[2:].any() and grad[:2].all(), (d, n, grad)
            continue
        scale = max(1.0, grad.max())
        groups = [grad[sl].max() / scale for _, sl in SC.grad_groups(d)[1:]]
        assert min(groups) >= GROUP_BAR, (d, n, nu, groups)
        lead = grad[:2].max() / grad[2:].max()
        assert lead <= LEAD_BAR, (d, n, nu, lead)
        worst_group, worst_lead = min(worst_group, min(groups)), max(worst_lead, lead)
    print(f"{np.dtype(dtype).name} regime: worst group of eight {worst_group:.1e} of the scale (bar {GROUP_BAR:g}), largest lead "
          f"{worst_lead:.1f} x the largest length-scale entry (bar {LEAD_BAR:g})")


def test_every_f32_fit_box_keeps_the_f32_oracle_in_digits():
    worst = 0.0
    for d, n, nu, dtype, _ in dict.fromkeys(SC.FIT_CASES + SC.LONG_FIT_CASES):
        if not SC.is_f32(dtype):
            continue
        X, y, theta = SC.inputs(d, n, dtype)
        lo, hi = SC.fit_box(theta, dtype)
        assert lo[0] == 1e-2 * hi[1] and np.all(lo < np.exp(theta)) and np.all(np.exp(theta) < hi)
        K = O.product_kernel(X.astype(np.float64), X.astype(np.float64), hi[1], hi[2:], nu)
        ev = np.linalg.eigvalsh(K + lo[0] * np.eye(n))
        cond = ev[-1] / ev[0]
        assert cond <= SC.COND32_BOUND and 1 + n * hi[1] / lo[0] <= SC.COND32_BOUND, (d, n, nu, cond)
        worst = max(worst, cond)
    print(f"f32 fit boxes: largest cond(K) at the worst corner {worst:.0f} (bound {SC.COND32_BOUND:.0f})")
