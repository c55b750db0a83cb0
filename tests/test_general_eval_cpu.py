"""CPU: the input guard of tests/test_gpu_general_eval.py, on the references alone.

The GPU module compares the lml gradient relative to its largest entry, a kernel matrix in f32 against an fp64 matrix, and
everything against LAPACK.  Each of these can pass or fail for the wrong reason, so for the very inputs of the GPU cases
(tests/general_eval_cases.py), in both noise regimes:

- every gradient group -- the noise / amplitude lead and each chunk of eight length scales -- holds a reference entry of at least
  20 bars of the gradient's scale max(1, max |grad|): a chunk gradtrace_tile dropped or published at the wrong offset is at least
  20 bars wrong;
- cond(K) <= 2.5e4 up to n = 320 (DESIGN.md section 17's figure) and <= 1e5 at n = 1921, also at the worst corner of each fit
  box: LAPACK's digits are not the limit of any comparison (tests/test_gpu_parity.py holds the 1e-8 bar at cond(K) = 8.5e6);
- the lean reference of the n = 1921 cases equals the oracle to 1e-12 wherever the oracle can be run;
- kmat_kernel's arithmetic, restated in the element type, reproduces the oracle's matrix exactly in f64 and stays within
  4 eps32 c of the fp64 matrix in f32: the device's bar of 8 eps32 c leaves the other half to its expf and sqrtf.

A case that fails here gets another data seed (general_eval_cases.DATA_SEED), not another guard."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import general_eval_cases as GE
import parity_rules as PRU
from hbetune_rs_amd import _lib

EPS32 = float(np.finfo(np.float32).eps)
_name = lambda t: np.dtype(t).name  # noqa: E731


def test_the_table_is_the_grid():
    cases = set(GE.EVAL_CASES)
    assert len(cases) == len(GE.EVAL_CASES) == 20
    assert GE.D_CLASSES == (1, 8, 9, 16, 17, 33, 64)
    assert {(d, 320, GE.nu_of(d)) for d in GE.D_CLASSES} <= cases
    assert {(d, 257, GE.nu_of(d)) for d in (9, 17, 64)} | {(d, 192, GE.nu_of(d)) for d in (9, 33)} <= cases
    assert {(d, 1921, GE.nu_of(d)) for d in (9, 64)} <= cases
    # every <T, NU2> instantiation of both kernels meets a ragged second chunk (d = 9) and eight full chunks (d = 64)
    assert {(9, 320, nu) for nu in GE.NUS} | {(64, 257, nu) for nu in GE.NUS} <= cases
    assert set(GE.PADDING_CASES) | set(GE.HOSTIO_CASES) <= {c[:2] for c in cases}
    assert [d + 2 for d, _ in GE.FIT_CASES] == [35, 66]  # 66 = LBFGS_MAXN
    for d in GE.D_CLASSES:
        names = [g[0] for g in GE.grad_groups(d)]
        assert len(names) == 1 + (d + 7) // 8
        assert sum(sl.stop - sl.start for _, sl in GE.grad_groups(d)) == d + 2


def test_the_finaliser_rule_is_enqueue_evals():
    """n = 1921 is the smallest n whose launch has more tiles than a fused finaliser takes; up to n = 320 it is fused (HBEGP_HOSTIO
    decides).  The rule restated in general_eval_cases is the one written in enqueue_eval, in both of its modes."""
    assert GE.tiles(GE.N_BIG) == 528 > GE.FUSE_GRAD_MAX_TILES >= GE.tiles(GE.N_BIG - 1) == 465
    assert all(GE.tiles(n) <= GE.FUSE_GRAD_MAX_TILES for _, n, _ in GE.EVAL_CASES if n != GE.N_BIG)
    assert GE.tiles(192) == 10 and GE.tiles(257) == GE.tiles(320) == 21
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "hbegp.cpp")).read()
    rules = re.findall(r"fuse_grad = (hostio && )?\(np / 64\) \* \(np / 64 \+ 1\) / 2 <= (\d+);", src)
    assert rules == [("", str(GE.FUSE_GRAD_MAX_TILES)), ("hostio && ", str(GE.FUSE_GRAD_MAX_TILES))], rules
    lb = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "lbfgs_step.hpp")).read()
    assert re.search(r"constexpr int LBFGS_MAXN = 66;", lb)


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=_name)
def test_the_lean_reference_is_the_oracle(dtype):
    worst = 0.0
    for d, n, nu in GE.EVAL_CASES:
        if n > GE.N_ORACLE_MAX:
            continue
        X, y, theta = GE.rounded_inputs(d, n, dtype)
        v = np.exp(theta)
        ref = GE.reference(d, n, nu, _name(dtype))
        lean = GE.lean_reference(X, y, v[0], v[1], v[2:], nu)
        assert np.array_equal(lean["kernel_matrix"], ref["kernel_matrix"]) and np.array_equal(lean["alpha"], ref["alpha"])
        devs = [PRU.dev(lean["lml"], ref["lml"]), PRU.dev(lean["grad"], ref["grad"]), PRU.dev(lean["k_inv"], ref["k_inv"])]
        assert max(devs) <= 1e-12, (d, n, nu, devs)
        worst = max(worst, max(devs))
    print(f"{_name(dtype)} regime: the lean reference is within {worst:.1e} of the oracle (bar 1e-12)")


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=_name)
@pytest.mark.parametrize("d,n,nu", GE.EVAL_CASES, ids=lambda v: str(v))
def test_no_group_of_the_gradient_is_small(d, n, nu, dtype):
    need = GE.GUARD_BARS * GE.tol_of(dtype)
    grad = np.abs(GE.reference(d, n, nu, _name(dtype))["grad"])
    scale = max(1.0, grad.max())
    groups = [(name, grad[sl].max() / scale) for name, sl in GE.grad_groups(d)]
    print(f"d={d} n={n} nu={nu} {_name(dtype)}: smallest group {min(g for _, g in groups):.1e} of the scale (need {need:g})")
    assert min(g for _, g in groups) >= need, (d, n, nu, _name(dtype), groups)


@pytest.mark.parametrize("d,n,nu", GE.EVAL_CASES, ids=lambda v: str(v))
def test_every_case_is_well_conditioned(d, n, nu):
    bound = GE.COND_MAX if n <= GE.N_ORACLE_MAX else GE.COND_MAX_BIG
    for dtype in GE.DTYPES:
        c = GE.cond(GE.reference(d, n, nu, _name(dtype))["kernel_matrix"])
        print(f"d={d} n={n} nu={nu} {_name(dtype)}: cond(K) = {c:.3g} (bound {bound:g})")
        assert c <= bound, (d, n, nu, _name(dtype), c)


@pytest.mark.parametrize("d,n", GE.FIT_CASES + (GE.TWO_PHASE_CASE,))
def test_every_fit_box_is_well_conditioned_at_its_worst_corner(d, n):
    for dtype in GE.DTYPES:
        X, _, theta = GE.rounded_inputs(d, n, dtype)
        lo, hi = GE.fit_box(theta)
        v = np.exp(theta)
        assert np.allclose(lo / v, [0.5, 0.6] + [0.7] * d) and np.allclose(hi / v, [4.0, 1.5] + [1.25] * d)
        corner = GE.worst_corner(theta)
        assert np.allclose(np.exp(corner), np.concatenate([[lo[0]], hi[1:]]))
        c = GE.cond(GE.kmat_reference(X, corner, GE.nu_of(d)))  # the order the fit runs at
        print(f"d={d} n={n} {_name(dtype)}: cond(K) at the worst corner of the fit box = {c:.3g} (bound {GE.COND_MAX:g})")
        assert c <= GE.COND_MAX, (d, n, _name(dtype), c)
        if (d, n) == GE.TWO_PHASE_CASE:
            theta0, starts = GE.two_phase_starts(d, n, theta)
            starts = [theta0, starts[0]]
        else:
            starts = list(GE.fit_starts(d, n, theta, 1))
        for s in starts:
            assert (s >= np.log(lo) - 1e-12).all() and (s <= np.log(hi) + 1e-12).all()


def _decisions(x0, lnlo, lnhi, f, g, maxeval):
    """hbegp_debug_lbfgs_decisions (host code only): the points the fit's state machine asks for, given the values so far, and per
    value whether it was a line-search trial and whether the trial was accepted."""
    n, count = len(x0), len(f)
    req = np.zeros((count, n))
    trial, acc, took = (np.zeros(count, dtype=np.int32) for _ in range(3))
    nreq = C.c_int(0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    cd = lambda a: _lib.dptr(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    f, g = np.ascontiguousarray(f, dtype=np.float64), np.ascontiguousarray(g, dtype=np.float64)
    _lib.check(_lib.load().hbegp_debug_lbfgs_decisions(n, cd(x0), cd(lnlo), cd(lnhi), maxeval, 0, 0, count, _lib.dptr(f), _lib.dptr(g),
                                                       _lib.dptr(req), ip(trial), ip(acc), ip(took), C.byref(nreq)))
    return req, trial, acc, nreq.value


def _rejected_and_no_new_best(d, n, dtype, x0, maxeval):
    """One run of the fit with the fp64 reference as its objective: (evaluations, trials the line search rejects that are no new
    best of the run -- the ones a fit ends after their lml)."""
    X, y, theta = GE.rounded_inputs(d, n, dtype)
    lo, hi = GE.fit_box(theta)
    f, g, x = [], [], np.array(x0)
    while len(f) < maxeval:
        ref = GE.reference_at(X, y, x, GE.nu_of(d), lo, hi)
        f.append(-ref["lml"])
        g.append(-ref["grad"])
        # one value more than there are: the state machine hands out the next point before it reads the last value
        req, trial, acc, nreq = _decisions(x0, np.log(lo), np.log(hi), f + [0.0], g + [np.zeros(d + 2)], maxeval)
        if nreq <= len(f):
            break
        x = req[len(f)].copy()
    best, count = np.inf, 0
    for i, fi in enumerate(f):
        new_best = fi < best
        best = min(best, fi)
        count += int(trial[i] and not acc[i] and not new_best)
    return len(f), count


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=_name)
def test_the_two_phase_starts_have_rejected_trials(dtype):
    """The GPU module asserts n_lml_only >= 1 on the fit from these starts; with the reference as the objective the state machine
    rejects 3 trials (f64 regime, the run from theta0) and 2 (f32 regime, the run from the start)."""
    d, n = GE.TWO_PHASE_CASE
    _, _, theta = GE.inputs(d, n, dtype)
    theta0, starts = GE.two_phase_starts(d, n, theta)
    runs = [_rejected_and_no_new_best(d, n, dtype, x0, GE.TWO_PHASE_MAXEVAL) for x0 in (theta0, starts[0])]
    print(f"{_name(dtype)} regime: (evaluations, lml-only trials) of the two runs: {runs}")
    assert [r[1] for r in runs] == ([3, 0] if np.dtype(dtype) == np.float64 else [0, 2]), runs
    assert all(np.abs(x0 - theta).max() > 0.3 for x0 in (theta0, starts[0]))  # well away from the case's theta


def test_kmat_restated_in_f64_is_the_oracles_matrix():
    for d, n, nu in GE.EVAL_CASES:
        if n > GE.N_ORACLE_MAX:
            continue
        X, _, theta = GE.rounded_inputs(d, n, np.float64)
        want = GE.reference(d, n, nu, "float64")["kernel_matrix"]
        assert np.array_equal(GE.kmat_reference(X, theta, nu), want), (d, n, nu)
        got = GE.kmat_restated(X, theta, nu, np.float64, oracle_poly=True)
        assert np.array_equal(got, want), (d, n, nu, float(np.abs(got - want).max()))
        # matern_map's own grouping of the nu = 5/2 polynomial: three roundings of half an eps each way of the oracle's
        dev = GE.kmat_restated(X, theta, nu, np.float64)
        if nu == 2.5:
            assert (np.abs(dev - want) <= 3 * np.finfo(np.float64).eps * np.abs(want)).all(), (d, n)
        else:
            assert np.array_equal(dev, want), (d, n, nu)


@pytest.mark.parametrize("nu", GE.NUS)
def test_kmat_restated_in_f32_is_within_four_eps_of_the_fp64_matrix(nu):
    """All 28 (d, nu) at n = 320: the roundings of x / ell, of the d-term sum, of matern_map's products and of amp * k, with a
    correctly rounded sqrt and exp, cost at most 4 eps32 c."""
    worst = (0.0, None)
    for d in GE.D_CLASSES:
        X, _, theta = GE.inputs(d, 320, np.float32)
        c = math.exp(theta[1])
        got = GE.kmat_restated(X, theta, nu, np.float32)
        want = GE.kmat_reference(X.astype(np.float64), theta, nu)  # the rounded inputs, everything else in fp64
        dev = float(np.abs(got.astype(np.float64) - want).max()) / (EPS32 * c)
        worst = max(worst, (dev, d))
        assert dev <= GE.KMAT_BAR32_CPU, (d, nu, dev)
    print(f"nu={nu}: f32 restatement of kmat_kernel within {worst[0]:.2f} eps32 c of the fp64 matrix (worst at d={worst[1]}; bar "
          f"{GE.KMAT_BAR32_CPU})")
