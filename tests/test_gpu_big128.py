"""GPU: the 128x128 task-queue tile (DAG_GEMM_128x128, csrc/dag_kernel.inc.hpp) at the smallest sizes that reach it.

The tile does the bulk of a large fit's work (HBEGP_DAG_BIG128 defaults to 2 for a fit's slots from 32 blocks on and for any
problem from 64) and has code of its own: with beta = 1 the old values are fetched in the epilogue, the f32 fragment reads are
split in two halves beside 64 fp64 chunk totals, the f32 flush has scheduling barriers, and a contraction range is the union of
the two column halves' ranges ("only adds exact zeros").  The plan switches are read per problem, so forcing
them builds the large problems' queues at six to seventeen blocks; tests/big128_cases.py holds the configurations and
tests/test_dag_plan_cpu.py asserts on the host that each of them really holds 128x128 tasks of every class it claims.

  A  the tile shape changes no bit: BIG128 in {1, 2} against 0, the same plan, any number of workgroups -- lml, gradient, alpha, the
     whole K^-1, diag(L) and the raw W2, padding included; the recursion plan also against the launch path
  B  the BIG128 = 2 evaluations of A against the oracle (an error both tile shapes share would pass A)
  C  three slots sharing the chip from three threads against a quiet single-slot BIG128 = 0 problem
  D  fits: fused and two-phase trials, even and lead / lag launches, against the BIG128 = 0 fit; `extend` repeats the evaluation
  E  a not positive definite matrix drains the queue and leaves the slot usable
  F  nothing depends on what a recycled pool block held (the union range reads parts of triangular operands no 128x64 tile reads)

Everything but B is bit for bit; B uses the project's bars (1e-8 / 1e-4 of the scale) and nothing else."""
import contextlib
import functools
import math
import os
import threading

import numpy as np
import pytest

import big128_cases as BC
import test_gpu_pool_hygiene as PH
from hbetune_rs_amd import gpr, synth
from oracle import gpr_oracle as O

pytestmark = pytest.mark.gpu

# every switch a case of this module sets: cleared before a forced problem is built, put back behind it
SWITCHES = ("HBEGP_DAG", "HBEGP_DAG_RL", "HBEGP_DAG_PROG", "HBEGP_DAG_SMALLH", "HBEGP_DAG_BIG128", "HBEGP_DAG_VALIDATE", "HBEGP_DAG_WG",
            "HBEGP_DAG_MIN_BLOCKS", "HBEGP_LAZY_GRAD", "HBEGP_RUN_BALANCE", "HBEGP_RUN_BALANCE_FORCE")


@contextlib.contextmanager
def forced(env):
    """The environment of a forced problem for the length of a `with` block (the library reads the switches when a problem is created)."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    assert set(env) <= set(SWITCHES), env
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in env.items()})
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def eval_inputs(n, dtype):
    """Config M in f64, config C5 in f32 with sigma^2 = 0.5 c (as tests/test_gpu_dag.py); two theta per problem."""
    w = synth.make_workload("M" if dtype == BC.F64 else "C5", n=n)
    X, y, theta = w["X"].astype(dtype), w["y"].astype(dtype), w["theta"].copy()
    if dtype == BC.F32:
        theta[0] = theta[1] + math.log(0.5)
    return X, y, (theta, theta + 0.02)


def evaluate(env, n, dtype, want_w2=True):
    """One evaluation per theta on a fresh single-slot problem: [dict(lml, grad, alpha, kinv, ldiag, w2)]."""
    X, y, thetas = eval_inputs(n, dtype)
    out = []
    with forced(env):
        prob = gpr.Problem(X, y)
        for theta in thetas:
            r = prob.lml_with_gradient(theta)
            assert r is not None, (env, n, dtype)
            alpha, kinv, ldiag = prob.results()
            got = dict(lml=np.array([r[0]]), grad=r[1], alpha=alpha, kinv=kinv, ldiag=ldiag)
            if want_w2:
                got["w2"] = prob.debug_work_matrix(2)
            out.append(got)
        prob.close()
    return out


def same_bits(ref, got, what, keys=None):
    for k in keys or ref:
        a, b = ref[k], got[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        if a.tobytes() != b.tobytes():
            bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
            raise AssertionError(f"{what}: {k} differs in {int(bad.sum())} of {a.size} entries, first at {np.argwhere(np.atleast_1d(bad))[:3].tolist()}, "
                                 f"largest difference {float(np.nanmax(np.abs(a.astype(float) - b.astype(float)))):.3e}")


def case_id(plan, n, dtype):
    return f"{plan[0]}-n{n}-{dtype}"


_kept = {}  # (plan name, n, dtype) -> the BIG128 = 2 evaluation at the default launch size: what B judges is what A compared


def big128_evaluation(plan, n, dtype):
    key = (plan[0], n, dtype)
    if key not in _kept:
        _kept[key] = evaluate(BC.env(plan, 2), n, dtype)
    return _kept[key]


# ---- A ------------------------------------------------------------------------------------------------------------------------------
EVAL_PARAMS = [pytest.param(plan, n, dtype, id=case_id(plan, n, dtype)) for plan, n, dtypes, _ in BC.EVAL_CASES for dtype in dtypes]


@pytest.mark.parametrize("plan,n,dtype", EVAL_PARAMS)
def test_the_tile_shape_changes_no_bit(plan, n, dtype):
    ref = evaluate(BC.env(plan, 0), n, dtype)
    for r in ref:
        assert all(np.isfinite(v).all() for v in r.values())
    for big128 in (1, 2):
        for wg in (0, 3, 40, 128):  # any number of workgroups: the same bits, and the launch ends
            if (big128, wg) == (2, 0) and (plan, n) in BC.ORACLE_CASES:
                got = big128_evaluation(plan, n, dtype)
            else:
                got = evaluate(dict(BC.env(plan, big128), HBEGP_DAG_WG=wg), n, dtype)
            for i, (r, g) in enumerate(zip(ref, got)):
                same_bits(r, g, (plan[0], n, dtype, "BIG128", big128, "workgroups", wg, "theta", i))
    if plan[1]["HBEGP_DAG_RL"] == "0":
        # the recursion plan runs the launch path's accumulations (tests/test_gpu_dag.py asserts it without the tile)
        launches = evaluate(dict(HBEGP_DAG="0"), n, dtype, want_w2=False)
        for i, (r, g) in enumerate(zip(launches, ref)):
            same_bits(r, g, (plan[0], n, dtype, "launch path", "theta", i), keys=("lml", "grad", "alpha", "kinv", "ldiag"))


# ---- B ------------------------------------------------------------------------------------------------------------------------------
def close(want, got, tol, what):
    want, got = np.asarray(want, dtype=np.float64), np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), what
    dev, scale = float(np.abs(want - got).max()), max(1.0, float(np.abs(want).max()))
    print(what, f"off by {dev / scale:.2e} of the scale (bar {tol:.0e})")
    assert dev <= tol * scale, (what, dev, scale)


@pytest.mark.parametrize("plan,n,dtype", [pytest.param(plan, n, dtype, id=case_id(plan, n, dtype)) for plan, n in BC.ORACLE_CASES for dtype in (BC.F64, BC.F32)])
def test_the_128x128_evaluations_against_the_oracle(plan, n, dtype):
    X, y, thetas = eval_inputs(n, dtype)
    tol = 1e-8 if dtype == BC.F64 else 1e-4
    for i, (theta, got) in enumerate(zip(thetas, big128_evaluation(plan, n, dtype))):
        ref = O.lml_with_gradient(X.astype(np.float64), y.astype(np.float64), math.exp(theta[0]), math.exp(theta[1]), np.exp(theta[2:]), 2.5)
        what = (plan[0], n, dtype, "theta", i)
        close(ref["lml"], got["lml"][0], tol, what + ("lml",))
        close(ref["grad"], got["grad"], tol, what + ("gradient",))
        close(ref["alpha"], got["alpha"], tol, what + ("alpha",))
        close(np.tril(ref["k_inv"]), np.tril(got["kinv"]), tol, what + ("tril K^-1",))


# ---- C ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BC.SOAK_CASE[2])
def test_three_slots_sharing_the_chip_equal_a_quiet_128x64_problem(dtype):
    # tests/test_gpu_dag.py::test_concurrent_soak_against_launch_path over 128x128 tiles: 3 slots x 20 rounds of different theta at
    # once, every result bit for bit what a single slot on 128x64 tiles returns on a quiet device -- a stale operand anywhere would show
    plan, n = BC.SOAK_CASE[:2]
    X, y, (theta, _) = eval_inputs(n, dtype)
    rounds = 20
    thetas = theta[None, :] + 0.15 * np.random.default_rng(7).standard_normal((3 * rounds, len(theta)))
    got, errors = [None] * len(thetas), []
    with forced(BC.env(plan, 2)):
        prob = gpr.Problem(X, y, n_slots=3)

        def work(slot):
            try:
                for r in range(rounds):
                    got[3 * r + slot] = prob.lml_with_gradient(thetas[3 * r + slot], slot=slot)
            except Exception as e:  # noqa: BLE001 -- reported below
                errors.append(repr(e))

        ts = [threading.Thread(target=work, args=(s,)) for s in range(3)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        prob.close()
    assert not errors, errors
    with forced(BC.env(plan, 0)):
        quiet = gpr.Problem(X, y)
        n_finite = 0
        for i, th in enumerate(thetas):
            r = quiet.lml_with_gradient(th)
            assert (r is None) == (got[i] is None), i
            if r is not None:
                assert r[0] == got[i][0] and np.array_equal(r[1], got[i][1]), i
                n_finite += 1
        quiet.close()
    assert n_finite >= len(thetas) // 2  # (the comparison is not of failures with failures)


# ---- D ------------------------------------------------------------------------------------------------------------------------------
FIT_MAXEVAL = 25


@functools.lru_cache(maxsize=None)
def fit_inputs(n, dtype):
    w = synth.make_workload("M", n=n, dtype=dtype)
    return w, synth.restart_points("M", w["lo"], w["hi"], 2), synth.candidates("M", 64, w["d"]).astype(w["dtype"])


def fit(env, n, dtype, trace):
    """One fit of 1 + 2 runs: what it hands back (compared bit for bit), and its trace and launch counts."""
    w, starts, cand = fit_inputs(n, dtype)
    with forced(env):
        fk = gpr.FittedKernel.new(w["X"], w["y"], w["theta0"], w["lo"], w["hi"], starts, maxeval=FIT_MAXEVAL, trace=trace)
    alpha, kinv = fk.arrays()
    mean, var, _ = fk.predict(cand)
    out = dict(theta=fk.theta.copy(), lml=np.array([fk.lml]), alpha=alpha, kinv_lower=np.tril(kinv), counts=np.array([fk.n_evals, fk.n_not_pd]),
               mean=mean, var=var)
    extra = dict(n_lml_only=fk.n_lml_only, trace=fk.trace, kinv=kinv, **fk.run_counts)
    fk.release()
    return out, extra


@pytest.mark.parametrize("dtype", BC.FIT_CASE[2])
def test_fits_on_128x128_tiles_equal_the_128x64_fit(dtype):
    plan, n = BC.FIT_CASE[:2]
    ref, rx = fit(BC.env(plan, 0), n, dtype, True)
    assert np.isfinite(ref["lml"]).all() and ref["counts"][0] >= 3 and rx["n_lml_only"] == 0
    first = None
    for lazy in (0, 1):
        for force in (None, "lag,lead,lead"):
            env = dict(BC.env(plan, 2), HBEGP_LAZY_GRAD=lazy)
            if force:
                env["HBEGP_RUN_BALANCE_FORCE"] = force
            # a trace with gradients evaluates every trial whole; one that records (theta, lml) leaves the trials in two phases
            for trace in (True,) + (("lml",) if lazy else ()):
                got, gx = fit(env, n, dtype, trace)
                what = (n, dtype, "lazy", lazy, "force", force, "trace", trace)
                same_bits(ref, got, what)
                for k in ("theta", "lml", "run"):
                    assert np.array_equal(rx["trace"][k], gx["trace"][k]), (what, k)
                if trace is True:
                    assert np.array_equal(rx["trace"]["grad"], gx["trace"]["grad"]), what
                    assert gx["n_lml_only"] == 0, what
                else:
                    assert gx["n_lml_only"] > 0 and gx["phase2"].sum() > 0, what  # the two queues of a trial really ran
                print(what, "lml-only", gx["n_lml_only"], "lead", gx["lead"].tolist(), "lag", gx["lag"].tolist())
                if force:  # as tests/test_gpu_run_balance.py: run 0 on the lag launches, the others on the lead ones
                    assert gx["lag"][0] > 0 and gx["lag"].sum() == gx["lag"][0], (what, gx["lag"])
                    assert gx["lead"][1] > 0 and gx["lead"][2] > 0 and gx["lead"][0] == 0, (what, gx["lead"])
                else:
                    assert gx["lead"].sum() == 0 and gx["lag"].sum() == 0, what
                first = first or (got, gx)
    # `extend` (one slot, 128x64 tiles, split K^-1 sums in f64) at the captured theta repeats the fit's evaluation on 128x128 tiles
    got, gx = first
    w = fit_inputs(n, dtype)[0]
    best = int(np.argmax(gx["trace"]["lml"]))
    assert gx["trace"]["lml"][best] == got["lml"][0]
    with forced(BC.env(plan, 0)):
        ex = gpr.FittedKernel.extend(w["X"], w["y"], gx["trace"]["theta"][best], w["lo"], w["hi"])
    a2, k2 = ex.arrays()
    assert ex.lml == got["lml"][0] and np.array_equal(a2, got["alpha"]) and np.array_equal(k2, gx["kinv"])
    ex.release()


# ---- E ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BC.F64, BC.F32])
def test_the_queue_drains_when_not_positive_definite(dtype):
    # the input of tests/test_gpu_dag.py::test_task_queue_drains_when_not_positive_definite: 144 copies of one row and vanishing noise,
    # so the third diagonal block flags the evaluation; every later task, 128x128 ones included, skips its work and bumps its counters
    plan, n = BC.NOT_PD_CASE[:2]
    rng = np.random.default_rng(5)
    X = rng.random((n, 3))
    X[256:] = X[10]
    y = rng.random(n)
    with forced(BC.env(plan, 2)):
        prob = gpr.Problem(X.astype(dtype), y.astype(dtype))
        assert prob.lml_with_gradient(np.array([math.log(1e-300), 0.0, 0.0, 0.0, 0.0])) is None
        ok = prob.lml_with_gradient(np.array([math.log(1e-2), 0.0, 0.0, 0.0, 0.0]))
        prob.close()
    assert ok is not None and np.isfinite(ok[0]) and np.all(np.isfinite(ok[1]))


# ---- F ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", PH.DTYPES, ids=PH._id)
def test_128x128_tiles_ignore_what_their_blocks_held(dtype):
    plan, n = BC.POOL_CASE[:2]
    case = (n, 8, 2.5)

    def subject():
        X, y, theta = PH._inputs(case, dtype)
        lo, hi, starts = PH._fit_box(theta, case[1])
        with forced(BC.env(plan, 2)):
            out = PH._s_lml(case, dtype)
            fk = gpr.FittedKernel.new(X, y, theta, lo, hi, starts, nu=case[2], maxeval=10)
        out += [fk.theta, fk.lml, *fk.arrays()]
        fk.release()
        return out

    # at least the evaluation's slot (7 blocks, 4 work matrices) and the fit's three (17 blocks, 12 work matrices)
    PH._check(subject, 24, 16 * PH._mat_bytes(n, dtype))
