"""GPU: the 128x128 task-queue tile skips the MFMAs of structurally zero operand halves (HBEGP_DAG_ZERO_SKIP, default on; DESIGN
section 7d) -- and no bit moves.

tests/test_gpu_big128.py compares the tile, skip and all, with the 128x64 tiles.  This module compares the tile with itself:
HBEGP_DAG_ZERO_SKIP = 0 (every wave multiplies the zeros, as the tile always did) against the default, at the smallest sizes whose
queues hold leading AND trailing half-zero stages on the A side AND on the B side (asserted on the host, with the rule the device
uses), on 3, 40 and 128 workgroups, in lml, gradient, alpha, the whole K^-1, diag(L) and the raw W2, padding included; three slots
sharing the chip; and a fit whose trials run in two phases.  tests/test_zero_half_cpu.py checks the rule itself.
"""
import contextlib
import os
import threading

import numpy as np
import pytest

import big128_cases as BC
import test_gpu_big128 as B
import test_zero_half_cpu as ZH
from hbetune_rs_amd import gpr

pytestmark = pytest.mark.gpu

SWITCHES = B.SWITCHES + ("HBEGP_DAG_ZERO_SKIP",)

# (plan, n, several slots): six blocks row by row and in the recursion, nine blocks (an odd split) with the divide-and-conquer inverse
EVAL_CASES = [(BC.RL_PROG, 700, False), (BC.REC_0, 700, False), (BC.RL_DC, 1100, False)]
SLOTS_CASE = (BC.RL_DC, 1300, True)
FIT_CASE = (BC.RL_PROG, 768, True)


@contextlib.contextmanager
def forced(env):
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


def assert_half_zero_stages_on_every_side(plan, n, several_slots, dtype, queues=(0,)):
    """On the host: the case's queue holds at least one leading and one trailing half-zero stage on the A side and on the B side."""
    bk = BC.stage_depth(dtype)
    sides = np.zeros((2, 2), dtype=int)
    for which in queues:
        tasks = ZH.queue(BC.blocks(n), bk, plan[2], 96, BC.fine_bits(plan, several_slots), 2, which)
        sides += ZH.check_queue(tasks, bk, (plan[0], n, dtype, which))[2]
    assert (sides > 0).all(), (plan[0], n, dtype, sides.tolist())  # [[A leading, A trailing], [B leading, B trailing]]
    return sides


def evaluate(env, n, dtype):
    """One evaluation per theta on a fresh single-slot problem (as tests/test_gpu_big128.py, with the switch of this module)."""
    X, y, thetas = B.eval_inputs(n, dtype)
    out = []
    with forced(env):
        prob = gpr.Problem(X, y)
        for theta in thetas:
            r = prob.lml_with_gradient(theta)
            assert r is not None, (env, n, dtype)
            alpha, kinv, ldiag = prob.results()
            out.append(dict(lml=np.array([r[0]]), grad=r[1], alpha=alpha, kinv=kinv, ldiag=ldiag, w2=prob.debug_work_matrix(2)))
        prob.close()
    return out


@pytest.mark.parametrize("plan,n,dtype", [pytest.param(p, n, t, id=B.case_id(p, n, t)) for p, n, _ in EVAL_CASES for t in (BC.F64, BC.F32)])
def test_skipping_the_zero_halves_changes_no_bit(plan, n, dtype):
    print(plan[0], n, dtype, "half-zero stages [[A lead, A trail], [B lead, B trail]]", assert_half_zero_stages_on_every_side(plan, n, False, dtype).tolist())
    for wg in (3, 40, 128):
        env = dict(BC.env(plan, 2), HBEGP_DAG_WG=wg)
        ref = evaluate(dict(env, HBEGP_DAG_ZERO_SKIP=0), n, dtype)
        got = evaluate(env, n, dtype)
        for i, (r, g) in enumerate(zip(ref, got)):
            assert all(np.isfinite(v).all() for k, v in r.items() if k != "w2"), (plan[0], n, dtype, wg, i)
            B.same_bits(r, g, (plan[0], n, dtype, "workgroups", wg, "theta", i))


def three_slots(env, n, dtype, thetas):
    """Three slots of one problem evaluate three theta at once, from three threads; per slot the results and the raw W2."""
    X, y, _ = B.eval_inputs(n, dtype)
    got, errors = [None] * 3, []
    with forced(env):
        prob = gpr.Problem(X, y, n_slots=3)

        def work(slot):
            try:
                r = prob.lml_with_gradient(thetas[slot], slot=slot)
                assert r is not None
                alpha, kinv, ldiag = prob.results(slot=slot)
                got[slot] = dict(lml=np.array([r[0]]), grad=r[1], alpha=alpha, kinv=kinv, ldiag=ldiag, w2=prob.debug_work_matrix(2, slot=slot))
            except Exception as e:  # noqa: BLE001 -- reported below
                errors.append(repr(e))

        ts = [threading.Thread(target=work, args=(s,)) for s in range(3)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        prob.close()
    assert not errors, errors
    return got


@pytest.mark.parametrize("dtype", [BC.F64, BC.F32])
def test_three_slots_sharing_the_chip(dtype):
    plan, n, several = SLOTS_CASE
    assert_half_zero_stages_on_every_side(plan, n, several, dtype)
    theta = B.eval_inputs(n, dtype)[2][0]
    thetas = theta[None, :] + 0.05 * np.random.default_rng(11).standard_normal((3, len(theta)))
    for wg in (3, 40, 128):
        env = dict(BC.env(plan, 2), HBEGP_DAG_WG=wg)
        ref = three_slots(dict(env, HBEGP_DAG_ZERO_SKIP=0), n, dtype, thetas)
        got = three_slots(env, n, dtype, thetas)
        for slot, (r, g) in enumerate(zip(ref, got)):
            B.same_bits(r, g, (n, dtype, "workgroups", wg, "slot", slot))


def fit(env, n, dtype):
    """One fit of 1 + 2 runs whose trace records (theta, lml), which leaves the line-search trials in two phases (as
    tests/test_gpu_big128.py's fit)."""
    w, starts, cand = B.fit_inputs(n, dtype)
    with forced(env):
        fk = gpr.FittedKernel.new(w["X"], w["y"], w["theta0"], w["lo"], w["hi"], starts, maxeval=B.FIT_MAXEVAL, trace="lml")
    alpha, kinv = fk.arrays()
    mean, var, _ = fk.predict(cand)
    out = dict(theta=fk.theta.copy(), lml=np.array([fk.lml]), alpha=alpha, kinv_lower=np.tril(kinv), counts=np.array([fk.n_evals, fk.n_not_pd]),
               mean=mean, var=var)
    extra = dict(n_lml_only=fk.n_lml_only, trace=fk.trace, kinv=kinv, **fk.run_counts)
    fk.release()
    return out, extra


def test_a_two_phase_fit_equals_its_twin_without_the_skip():
    plan, n, several = FIT_CASE
    dtype = BC.F64
    # the fused queue, the first phase's and the K^-1 tasks alone all run in such a fit; together they hold every kind of stage
    assert_half_zero_stages_on_every_side(plan, n, several, dtype, queues=(0, 1, 2))
    env = dict(BC.env(plan, 2), HBEGP_LAZY_GRAD=1)
    ref, rx = fit(dict(env, HBEGP_DAG_ZERO_SKIP=0), n, dtype)
    got, gx = fit(env, n, dtype)
    assert np.isfinite(ref["lml"]).all() and ref["counts"][0] >= 3
    assert gx["n_lml_only"] > 0 and gx["phase2"].sum() > 0 and rx["n_lml_only"] == gx["n_lml_only"]  # the two queues of a trial really ran
    B.same_bits(ref, got, (n, dtype, "two-phase fit"))  # theta, lml, alpha, lower K^-1, counts, 64 predictions (mean and variance)
    assert np.array_equal(rx["kinv"], gx["kinv"])
    for k in ("theta", "lml", "run"):
        assert np.array_equal(rx["trace"][k], gx["trace"][k]), k
