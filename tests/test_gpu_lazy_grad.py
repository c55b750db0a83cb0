"""GPU: line-search trials evaluated in two phases (HBEGP_LAZY_GRAD, the default: lml first; K^-1 and the gradient only for trials
the optimiser accepts or the capture rule keeps) against the fused evaluation of every trial (HBEGP_LAZY_GRAD=0), same build.

The values the optimiser reads must have the same bits, so everything a fit hands back does: theta, lml, alpha, the lower triangle
of K^-1, the evaluation counts, and predictions.  And the work must really be skipped: the fit's count of lml-only evaluations is
what a replay of its evaluations through the host state machine and the decision query says, exactly."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from hbetune_rs_amd import _lib, gpr, synth

pytestmark = pytest.mark.gpu

MAXEVAL = 150


@functools.lru_cache(maxsize=None)
def workload(n, dtype):
    w = synth.make_workload("M", n=n, dtype=dtype)
    starts = synth.restart_points("M", w["lo"], w["hi"], 2)
    cand = synth.candidates("M", 64, w["d"]).astype(w["dtype"])
    return w, starts, cand


def fit(n, dtype, fixed_work, ctx=None, trace=False):
    """One fit with whatever HBEGP_LAZY_GRAD is in the environment now (the library reads it when the fit's problem is created)."""
    w, starts, cand = workload(n, dtype)
    fk = gpr.FittedKernel.new(w["X"], w["y"], w["theta0"], w["lo"], w["hi"], starts, maxeval=MAXEVAL, fixed_work=fixed_work, ctx=ctx, trace=trace)
    alpha, kinv = fk.arrays()
    mean, var, _ = fk.predict(cand)
    out = dict(theta=fk.theta.copy(), lml=np.array([fk.lml]), alpha=alpha, kinv_lower=np.tril(kinv), counts=np.array([fk.n_evals, fk.n_not_pd]),
               mean=mean, var=var)
    extra = dict(n_lml_only=fk.n_lml_only, trace=getattr(fk, "trace", None))
    fk.release()
    return out, extra


def same_bits(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k, float(np.max(np.abs(a[k].astype(float) - b[k].astype(float)))))


# n = 256: the launch path (K^-1 is a launch of its own behind the decision); 700: ragged, the smallest task-queue sizes (row-progressive
# plan: the K^-1-only queue keeps its range-after-range gates); 1024: the task queue on whole blocks.  f32 at 700: per-range rounding.
@pytest.mark.parametrize("n,dtype", [(256, "float64"), (700, "float64"), (1024, "float64"), (700, "float32")])
@pytest.mark.parametrize("fixed_work", [True, False])
def test_lazy_fit_equals_fused_fit_bit_for_bit(n, dtype, fixed_work, monkeypatch):
    monkeypatch.setenv("HBEGP_LAZY_GRAD", "0")
    fused, fx = fit(n, dtype, fixed_work)
    monkeypatch.delenv("HBEGP_LAZY_GRAD")
    lazy, lx = fit(n, dtype, fixed_work)
    print(f"n = {n} {dtype} fixed_work = {fixed_work}: {int(lazy['counts'][0])} evaluations, {lx['n_lml_only']} of them lml only")
    assert fx["n_lml_only"] == 0
    same_bits(fused, lazy, (n, dtype, fixed_work))
    if fixed_work:
        assert lazy["counts"][0] == 3 * MAXEVAL


def test_two_lazy_fits_in_flight_on_one_context_equal_each_fit_alone():
    # two host threads, one context: each fit's two-phase trials run beside the other's (crowded-device queue variants included);
    # each result is the same fit's alone
    ctx = gpr.Context(device_ids=[0])
    jobs = [(700, "float64", True), (1024, "float64", False)]
    alone = [fit(*j, ctx=ctx) for j in jobs]
    got, errors = [None, None], []

    def work(i):
        try:
            got[i] = fit(*jobs[i], ctx=ctx)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    ctx.close()
    assert not errors, errors
    for i in range(2):
        same_bits(alone[i][0], got[i][0], jobs[i])
        assert alone[i][1]["n_lml_only"] == got[i][1]["n_lml_only"] > 0


def replay_count(w, starts, trace, fixed_work):
    """The number of evaluations for which neither the decision query (accepted) nor the capture rule (a new best lml of the run's
    slot: one run per slot here) asks for K^-1 and the gradient, from the recorded (theta, lml, gradient) of every evaluation."""
    lib = _lib.load()
    p = len(w["theta0"])
    lnlo, lnhi = np.log(w["lo"]), np.log(w["hi"])
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    total = 0
    for r in range(3):
        sel = trace["run"] == r
        theta, lml, grad = trace["theta"][sel], trace["lml"][sel], trace["grad"][sel]
        k = len(lml)
        f = np.ascontiguousarray(-lml)  # the objective the optimiser minimises; +inf for a failed evaluation
        g = np.ascontiguousarray(-grad)
        x0 = w["theta0"] if r == 0 else starts[r - 1]
        req = np.zeros((k, p))
        trial, acc, took = (np.zeros(k, dtype=np.int32) for _ in range(3))
        nreq = C.c_int(0)
        _lib.check(lib.hbegp_debug_lbfgs_decisions(p, _lib.dptr(np.ascontiguousarray(x0, dtype=float)), _lib.dptr(lnlo), _lib.dptr(lnhi), MAXEVAL, 0,
                                                   int(fixed_work), k, _lib.dptr(f), _lib.dptr(g), _lib.dptr(req), ip(trial), ip(acc), ip(took),
                                                   C.byref(nreq)))
        assert nreq.value == k and np.array_equal(req, theta)  # the replay walks the fit's own points
        assert np.array_equal(acc, took)
        best = -np.inf
        for i in range(k):
            new_best = np.isfinite(lml[i]) and lml[i] > best
            if new_best:
                best = lml[i]
            if trial[i] and not acc[i] and not new_best:
                total += 1
    return total


@pytest.mark.parametrize("fixed_work", [True, False])
def test_the_work_is_really_skipped(fixed_work, monkeypatch):
    n = 1024
    monkeypatch.setenv("HBEGP_MAX_CONCURRENT", "3")  # replay_count's capture rule: one run per slot
    w, starts, _ = workload(n, "float64")
    lazy, lx = fit(n, "float64", fixed_work, trace="lml")  # records (theta, lml): the evaluation stays lazy
    assert lx["n_lml_only"] > 0
    # a trace that records gradients evaluates every trial whole: the same points, the same values, and their gradients
    full, fx = fit(n, "float64", fixed_work, trace=True)
    assert fx["n_lml_only"] == 0
    same_bits(lazy, full, "traced")
    for k in ("theta", "lml", "run"):
        assert np.array_equal(lx["trace"][k], fx["trace"][k]), k
    want = replay_count(w, starts, fx["trace"], fixed_work)
    print(f"n = {n} fixed_work = {fixed_work}: {lx['n_lml_only']} lml-only evaluations of {int(lazy['counts'][0])}; the replay says {want}")
    assert lx["n_lml_only"] == want
    monkeypatch.setenv("HBEGP_LAZY_GRAD", "0")
    _, off = fit(n, "float64", fixed_work)
    assert off["n_lml_only"] == 0
