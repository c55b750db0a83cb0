"""CPU: the input guard of tests/test_gpu_feature_counts.py, on the restatements alone.

The GPU module compares a gradient relative to its largest entry.  A chunk of eight length scales that gradtrace_tile dropped
or published at the wrong offset, or a pass of 16 features that pred_grad_kernel lost, would pass such a comparison if the
chunk's entries were small.  So for the very inputs of the GPU cases (tests/feature_count_cases.py), in both noise regimes:

- every group of eight length-scale entries of the leave-one-out gradient holds an entry of at least 100 tol of the gradient's
  scale max(1, max |grad|), and every single entry is above tol of it: a lost entry is a failure, a lost chunk one by 100 x;
- every group of 16 columns of dmean holds, at m = 5 and at m = 70, an entry above 100 tol of its row's largest.

A case that fails here gets another data seed (feature_count_cases.DATA_SEED), not another guard."""
import numpy as np
import pytest

import feature_count_cases as FC
import loo_ref as LR
import predict_grad_ref as PG
from oracle import gpr_oracle as O


def test_the_table_is_the_grid():
    assert FC.D_CLASSES == (1, 8, 9, 16, 17, 33, 64) and FC.N_GENERAL == (257, 320)
    assert [FC.nu_of(d) for d in (9, 16, 17, 33)] == [2.5, np.inf, 0.5, 1.5]  # every order meets a d > 8
    assert {(d, n) for d in FC.D_CLASSES for n in FC.N_GENERAL} <= set(FC.LOO_CASES)
    assert {(9, 256), (64, 256), (33, 90), (64, 90)} <= set(FC.LOO_CASES)
    assert set(FC.QUERY_CASES) == {(d, 320) for d in FC.D_CLASSES} | {(d, 257) for d in (9, 17, 64)}
    assert {c[:2] for c in FC.PATH_CASES} == set(FC.QUERY_CASES) and (64, 320, 0.5) in FC.PATH_CASES
    assert len(set(FC.LOO_CASES)) == len(FC.LOO_CASES) and len(set(FC.PATH_CASES)) == len(FC.PATH_CASES)


@pytest.mark.parametrize("dtype", FC.DTYPES, ids=lambda t: np.dtype(t).name)
def test_no_chunk_of_the_loo_gradient_is_small(dtype):
    tol = FC.tol_of(dtype)
    worst_group = worst_entry = np.inf
    for d, n in FC.LOO_CASES:
        X, y, theta = FC.inputs(d, n, dtype)
        grad = np.abs(LR.loo_at_theta(X, y, theta, FC.nu_of(d))["grad"])
        scale = max(1.0, grad.max())
        groups = [grad[2:][sl].max() / scale for sl in FC.groups(d, FC.GROUP_LOO)]
        assert min(groups) >= 100 * tol, (d, n, groups)
        assert grad.min() / scale > tol, (d, n, grad / scale)
        worst_group, worst_entry = min(worst_group, min(groups)), min(worst_entry, grad.min() / scale)
    print(f"{np.dtype(dtype).name} regime: worst group {worst_group:.1e}, worst entry {worst_entry:.1e} of the scale (bars "
          f"{100 * tol:g}, {tol:g})")


@pytest.mark.parametrize("dtype", FC.DTYPES, ids=lambda t: np.dtype(t).name)
def test_no_pass_of_dmean_is_small(dtype):
    tol = FC.tol_of(dtype)
    worst = np.inf
    for d, n in FC.QUERY_CASES:
        X, y, theta = FC.inputs(d, n, dtype)
        X64, v, nu = X.astype(np.float64), np.exp(theta), FC.nu_of(d)
        alpha = O.extend(X64, y.astype(np.float64), v[0], v[1], v[2:], nu)["alpha"]
        pool = FC.query_points(X, dtype)
        assert np.array_equal(pool[1], X[7]) and np.array_equal(pool[3], X[n - 1])  # the two rows on training rows
        dmean = np.abs(PG.dmean_ref(pool.astype(np.float64), X64, alpha, v[1], v[2:], nu))
        rel = dmean / dmean.max(axis=1, keepdims=True)
        for m in FC.M_QUERY:
            groups = [rel[:m, sl].max() for sl in FC.groups(d, FC.GROUP_DMEAN)]
            assert min(groups) > 100 * tol, (d, n, m, groups)
            worst = min(worst, min(groups))
    print(f"{np.dtype(dtype).name} regime: worst group of 16 columns {worst:.1e} of its row's largest (bar {100 * tol:g})")
