"""GPU: task queues ordered for another worker count than they are launched with (HBEGP_DAG_ORDER_WG, _P1, _KINV, _LEAD, _LAG;
csrc/dag_plan.hpp).  The order decides when a workgroup claims a task, never what the task computes, so the only way a new order
can go wrong on the device is by being unsound for the resident workgroups: at the smallest sizes that take the task queue with three
slots, with every queue of every variant forced to an order for one worker, for a count far below the launch size and for one above
it, a fit equals the default-order fit bit for bit -- theta, lml, alpha, the lower triangle of K^-1, the counts and 64 predictions --
under HBEGP_RUN_BALANCE=1 (so the lead and lag variants are built and used) and HBEGP_DAG_VALIDATE=1.  An evaluation that ended in
DAG_INFO_TIMEOUT would raise out of the fit."""
import ctypes as C
import functools

import numpy as np
import pytest

from hbetune_rs_amd import _lib, gpr, synth

pytestmark = pytest.mark.gpu

MAXEVAL = 150
SWITCHES = ("HBEGP_DAG_ORDER_WG", "HBEGP_DAG_ORDER_WG_P1", "HBEGP_DAG_ORDER_WG_KINV", "HBEGP_DAG_ORDER_WG_LEAD", "HBEGP_DAG_ORDER_WG_LAG")
# one worker | far below the launch size (96 even, 80 lead, 128 lag) | above every launch size
FORCED = (1, 8, 200)
# n = 700: 6 blocks, ragged, the smallest task-queue size (row-progressive plan); 1024: whole blocks; f32 at 700: per-range rounding
CASES = [(700, "float64"), (1024, "float64"), (700, "float32")]


@functools.lru_cache(maxsize=None)
def workload(n, dtype):
    w = synth.make_workload("M", n=n, dtype=dtype)
    starts = synth.restart_points("M", w["lo"], w["hi"], 2)
    cand = synth.candidates("M", 64, w["d"]).astype(w["dtype"])
    return w, starts, cand


def fit(n, dtype, fixed_work):
    """One three-run fit with whatever switches are in the environment now (read when the fit's problem is created)."""
    w, starts, cand = workload(n, dtype)
    fk = gpr.FittedKernel.new(w["X"], w["y"], w["theta0"], w["lo"], w["hi"], starts, maxeval=MAXEVAL, fixed_work=fixed_work)
    alpha, kinv = fk.arrays()
    mean, var, _ = fk.predict(cand)
    out = dict(theta=fk.theta.copy(), lml=np.array([fk.lml]), alpha=alpha, kinv_lower=np.tril(kinv),
               counts=np.array([fk.n_evals, fk.n_not_pd, fk.n_lml_only]), mean=mean, var=var)
    runs = dict(lead=fk.run_counts["lead"].copy(), lag=fk.run_counts["lag"].copy())
    fk.release()
    return out, runs


@functools.lru_cache(maxsize=None)
def reference(n, dtype, fixed_work):
    """The default-order fit: computed once per case (the caller has cleared the switches), shared and never changed."""
    return fit(n, dtype, fixed_work)


def same_bits(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k, float(np.max(np.abs(a[k].astype(float) - b[k].astype(float)))))


def test_the_forced_orders_are_other_orders():
    # what the switches select at six blocks really differs from the default queue (otherwise the fits below compare nothing)
    lib = _lib.load()

    def tiles(order_wg):
        nt, err = C.c_int(), C.create_string_buffer(400)
        tasks = np.zeros((2000, 18), dtype=np.int32)
        rc = lib.hbegp_debug_dag_replay(6, 16, 4, 96, order_wg, 1 | 8 | 16 | 32, 0, 0, 0, C.byref(nt), tasks.ctypes.data_as(C.POINTER(C.c_int)),
                                        2000, None, err, 400)
        assert rc == 0, err.value.decode()
        return tasks[: nt.value]

    base = tiles(0)
    for order_wg in FORCED[:2]:
        assert not np.array_equal(tiles(order_wg), base), order_wg


@pytest.mark.parametrize("n,dtype", CASES)
@pytest.mark.parametrize("fixed_work", [True, False])
def test_fits_on_forced_orders_equal_the_default_order_fit_bit_for_bit(n, dtype, fixed_work, monkeypatch):
    for k in SWITCHES + ("HBEGP_RUN_BALANCE_FORCE", "HBEGP_RUN_BALANCE_WG", "HBEGP_RUN_BALANCE_HYST"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HBEGP_RUN_BALANCE", "1")  # below 32 blocks the lead / lag variants exist only when asked for
    monkeypatch.setenv("HBEGP_DAG_VALIDATE", "1")
    ref, _ = reference(n, dtype, fixed_work)
    if fixed_work:
        assert ref["counts"][0] == 3 * MAXEVAL
    for order_wg in FORCED:
        for k in SWITCHES:
            monkeypatch.setenv(k, str(order_wg))
        got, runs = fit(n, dtype, fixed_work)
        print((n, dtype, fixed_work, order_wg), "evaluations", got["counts"].tolist(), "lead", runs["lead"].tolist(), "lag", runs["lag"].tolist())
        same_bits(ref, got, (n, dtype, fixed_work, order_wg))


def test_the_lead_and_lag_queues_on_forced_orders_keep_the_bits(monkeypatch):
    # every slot pinned to a class, so that the lead and the lag variant's reordered queues certainly run
    for k in SWITCHES + ("HBEGP_RUN_BALANCE_WG", "HBEGP_RUN_BALANCE_HYST"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HBEGP_RUN_BALANCE", "1")
    monkeypatch.setenv("HBEGP_DAG_VALIDATE", "1")
    monkeypatch.delenv("HBEGP_RUN_BALANCE_FORCE", raising=False)
    ref, _ = reference(700, "float64", True)
    monkeypatch.setenv("HBEGP_RUN_BALANCE_FORCE", "lag,lead,lead")
    for order_wg in FORCED:
        monkeypatch.setenv("HBEGP_DAG_ORDER_WG_LEAD", str(order_wg))
        monkeypatch.setenv("HBEGP_DAG_ORDER_WG_LAG", str(order_wg))
        got, runs = fit(700, "float64", True)
        same_bits(ref, got, ("pinned", order_wg))
        assert runs["lag"][0] > 0 and runs["lead"][1] > 0 and runs["lead"][2] > 0, (order_wg, runs)
