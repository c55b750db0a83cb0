"""GPU: unequal shares of the compute units for the runs of a fit (HBEGP_RUN_BALANCE, csrc/slot_share.hpp: the run that is behind
launches a larger task queue, the others smaller ones).  Which launch size an evaluation gets now depends on how far the other runs
have come, that is on timing -- so nothing a fit hands back may depend on the launch size: with every slot pinned to a class, in
all three rotations, and with the policy deciding, the fit equals the HBEGP_RUN_BALANCE=0 fit bit for bit.  The per-run clocks and
launch counts of hbegp_last_fit_stats show that the variants were really used, and that the cases that must keep today's choice --
one slot, a second fit in flight on the context -- never use one."""
import functools
import threading
import time

import numpy as np
import pytest

from hbetune_rs_amd import _lib, gpr, synth

pytestmark = pytest.mark.gpu

MAXEVAL = 150
FORCED = ("lag,lead,lead", "lead,lag,lead", "lead,lead,lag")
# n = 700: ragged, the smallest task-queue size (row-progressive plan); 1024: whole blocks; f32 at 700: per-range rounding
CASES = [(700, "float64"), (1024, "float64"), (700, "float32")]


@functools.lru_cache(maxsize=None)
def workload(n, dtype):
    w = synth.make_workload("M", n=n, dtype=dtype)
    starts = synth.restart_points("M", w["lo"], w["hi"], 2)
    cand = synth.candidates("M", 64, w["d"]).astype(w["dtype"])
    return w, starts, cand


def fit(n, dtype, fixed_work, ctx=None, n_starts=2):
    """One fit with whatever HBEGP_RUN_BALANCE* is in the environment now (the library reads them when the fit's problem is created)."""
    w, starts, cand = workload(n, dtype)
    t0 = time.perf_counter()
    fk = gpr.FittedKernel.new(w["X"], w["y"], w["theta0"], w["lo"], w["hi"], starts[:n_starts] if n_starts else None, maxeval=MAXEVAL,
                              fixed_work=fixed_work, ctx=ctx)
    wall_ms = (time.perf_counter() - t0) * 1e3
    alpha, kinv = fk.arrays()
    mean, var, _ = fk.predict(cand)
    out = dict(theta=fk.theta.copy(), lml=np.array([fk.lml]), alpha=alpha, kinv_lower=np.tril(kinv),
               counts=np.array([fk.n_evals, fk.n_not_pd, fk.n_lml_only]), mean=mean, var=var)
    extra = dict(wall_ms=wall_ms, end_ms=fk.run_end_ms, **fk.run_counts)
    fk.release()
    return out, extra


def same_bits(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k, float(np.max(np.abs(a[k].astype(float) - b[k].astype(float)))))


def clear_env(monkeypatch):
    for k in ("HBEGP_RUN_BALANCE", "HBEGP_RUN_BALANCE_FORCE", "HBEGP_RUN_BALANCE_WG", "HBEGP_RUN_BALANCE_HYST"):
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def reference(n, dtype, fixed_work):
    """The HBEGP_RUN_BALANCE=0 fit: computed once per case (the callers set the environment), shared and never changed."""
    return fit(n, dtype, fixed_work)


def off_fit(monkeypatch, n, dtype, fixed_work):
    clear_env(monkeypatch)
    monkeypatch.setenv("HBEGP_RUN_BALANCE", "0")
    ref = reference(n, dtype, fixed_work)
    monkeypatch.delenv("HBEGP_RUN_BALANCE")
    return ref


def check_clocks(x, out, what):
    """The per-run end times are finite, positive and no later than the fit's wall time, and the counts beside them are consistent:
    every run made between one evaluation and the cap, the runs' evaluations add up to the fit's and their lml-only ones to
    n_lml_only, and no run has more lead / lag evaluations than evaluations."""
    ends = x["end_ms"]
    evals = x["fused"] + x["lml_only"] + x["phase2"]
    print(what, "run ends (ms)", np.round(ends, 2).tolist(), "wall", round(x["wall_ms"], 2), "evaluations", evals.tolist(), "lead", x["lead"].tolist(),
          "lag", x["lag"].tolist())
    assert len(ends) == 3 and np.all(np.isfinite(ends)) and np.all(ends > 0)
    assert ends.max() <= x["wall_ms"]
    assert evals.sum() == out["counts"][0] and x["lml_only"].sum() == out["counts"][2]
    assert np.all(evals >= 1) and np.all(evals <= MAXEVAL)
    assert np.all(x["lead"] + x["lag"] <= evals)


@pytest.mark.parametrize("n,dtype", CASES)
@pytest.mark.parametrize("fixed_work", [True, False])
def test_fits_with_unequal_shares_equal_the_even_fit_bit_for_bit(n, dtype, fixed_work, monkeypatch):
    ref, rx = off_fit(monkeypatch, n, dtype, fixed_work)
    check_clocks(rx, ref, (n, dtype, fixed_work, "off"))
    assert rx["lead"].sum() == 0 and rx["lag"].sum() == 0
    if fixed_work:
        assert ref["counts"][0] == 3 * MAXEVAL
    for i, force in enumerate(FORCED):
        monkeypatch.setenv("HBEGP_RUN_BALANCE_FORCE", force)
        got, gx = fit(n, dtype, fixed_work)
        check_clocks(gx, got, (n, dtype, fixed_work, force))
        same_bits(ref, got, (n, dtype, fixed_work, force))
        # the forced leg really ran on the other launch sizes: run i (slot i) lag, the others lead, while all three were running
        assert gx["lag"][i] > 0 and gx["lag"].sum() == gx["lag"][i], (force, gx["lag"])
        assert all(gx["lead"][j] > 0 for j in range(3) if j != i) and gx["lead"][i] == 0, (force, gx["lead"])
    monkeypatch.delenv("HBEGP_RUN_BALANCE_FORCE")
    monkeypatch.setenv("HBEGP_RUN_BALANCE", "1")
    got, gx = fit(n, dtype, fixed_work)
    check_clocks(gx, got, (n, dtype, fixed_work, "policy on"))
    same_bits(ref, got, (n, dtype, fixed_work, "policy on"))


def test_the_policy_at_another_threshold_and_other_sizes_keeps_the_bits(monkeypatch):
    # n = 1024, fixed work: the runs' accepted trials differ (each is two launches), so their progress usually drifts apart by more
    # than the threshold long before the first one ends.  Which run is behind, and whether any is, depends on timing (two slots whose
    # streams share a hardware queue stay level): the lead / lag counts are printed, the assertions on them are the forced legs'.
    ref, _ = off_fit(monkeypatch, 1024, "float64", True)
    monkeypatch.setenv("HBEGP_RUN_BALANCE", "1")
    monkeypatch.setenv("HBEGP_RUN_BALANCE_HYST", "1")
    got, gx = fit(1024, "float64", True)
    check_clocks(gx, got, "policy on, threshold 1")
    same_bits(ref, got, "policy on, threshold 1")
    # other launch sizes change the timing, never the bits
    monkeypatch.setenv("HBEGP_RUN_BALANCE_WG", "72,144")
    got, gx = fit(1024, "float64", True)
    same_bits(ref, got, "policy on, 72 / 144 workgroups")


def test_the_default_is_off_below_32_blocks(monkeypatch):
    # nothing in the environment: below 32 blocks no lead / lag variant exists (measured: no gain there)
    clear_env(monkeypatch)
    _, small = fit(1024, "float64", True)
    assert small["lead"].sum() == 0 and small["lag"].sum() == 0


def test_a_single_slot_never_uses_an_unequal_share(monkeypatch):
    clear_env(monkeypatch)
    monkeypatch.setenv("HBEGP_RUN_BALANCE", "0")
    ref, _ = fit(1024, "float64", False, n_starts=0)
    monkeypatch.setenv("HBEGP_RUN_BALANCE", "1")
    monkeypatch.setenv("HBEGP_RUN_BALANCE_FORCE", "lag,lead,lead")
    got, gx = fit(1024, "float64", False, n_starts=0)
    same_bits(ref, got, "one run")
    assert len(gx["end_ms"]) == 1 and gx["lead"].sum() == 0 and gx["lag"].sum() == 0
    # three runs over two slots: a slot takes two runs in turn and has no single progress count -- today's choice as well
    monkeypatch.setenv("HBEGP_MAX_CONCURRENT", "2")
    got, gx = fit(700, "float64", False)
    assert len(gx["end_ms"]) == 3 and gx["lead"].sum() == 0 and gx["lag"].sum() == 0


def test_a_fit_beside_another_fit_on_the_context_never_uses_an_unequal_share(monkeypatch):
    # a long fit (n = 1024, fixed work) in a thread of its own; once it is in flight, a short one (n = 700, early stopping) beside it
    # on the same context: the short fit finds the other one at its first evaluation and keeps the even / crowded-device launch sizes
    # to its end, although every slot is pinned to a class.  Both equal the same fits alone.
    ctx = gpr.Context(device_ids=[0])
    clear_env(monkeypatch)
    monkeypatch.setenv("HBEGP_RUN_BALANCE", "0")
    alone = [fit(1024, "float64", True, ctx=ctx), fit(700, "float64", False, ctx=ctx)]
    monkeypatch.setenv("HBEGP_RUN_BALANCE", "1")
    monkeypatch.setenv("HBEGP_RUN_BALANCE_FORCE", "lag,lead,lead")
    lib = _lib.load()
    got, errors = [None, None], []

    def long_fit():
        try:
            got[0] = fit(1024, "float64", True, ctx=ctx)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))

    t = threading.Thread(target=long_fit)
    t.start()
    t0 = time.perf_counter()
    while lib.hbegp_debug_fits_in_flight(0) < 1 and t.is_alive() and time.perf_counter() - t0 < 20:
        pass
    in_flight = lib.hbegp_debug_fits_in_flight(0)
    got[1] = fit(700, "float64", False, ctx=ctx)
    still = t.is_alive()
    t.join()
    ctx.close()
    assert not errors, errors
    assert in_flight >= 1
    for i in range(2):
        same_bits(alone[i][0], got[i][0], i)
    print("long fit still in flight when the short one was over:", still, "short fit lead / lag:", got[1][1]["lead"].tolist(), got[1][1]["lag"].tolist())
    assert got[1][1]["lead"].sum() == 0 and got[1][1]["lag"].sum() == 0
