"""GPU: the reference's own regime -- up to 128 rows -- at every feature chunk, Matern order and stop decision (DESIGN.md
section 27).

There an evaluation is one launch (small_eval_kernel: everything in the LDS, features staged eight at a time, pass A upwards,
pass B backwards from the chunk pass A left staged) and an optimiser run is one launch too (small_fit_kernel: the evaluation,
the wave-wide L-BFGS wl_*, the capture of the best evaluation into a ping-pong buffer): 2 kernels x 4 orders x 2 element types.

A. One evaluation in one launch over D_SMALL x two row counts per d, both element types, orders rotating: lml, gradient, alpha,
   K^-1, diag(L), extend's model and predict at five points against the fp64 oracle and against the general path
   (HBEGP_SMALL=0).  The gradient is judged per group -- the noise / amplitude lead, then each chunk of eight length scales -- on
   the scale of the whole gradient, so a failure names the chunk.  d = 33 is the control: the general path both times, bit-equal.
B. The device-driven fit at d in {1, 9, 17, 25, 32} x the four orders: every traced evaluation against the oracle of the element
   type (parity_rules.Judge, gradient per group), the capture rule and the model copied out of ping-pong buffer 0 or 1, the
   optimiser against the host state machine in BOTH directions (the host asks for the points the device evaluated, and stops
   where the device stopped), and predict of the fitted model.  d = 33 is the host-driven control.  Six fits of 150 evaluations
   on top, whose runs end by the pgtol / ftol tests at p = 11, 19, 27 and 34: capture and replay only.

The cases and data come from tests/small_regime_cases.py, which tests/test_small_regime_cpu.py guards.  No bar is new: TOL64 /
TOL32 against the oracle, the Judge rule along a fit, 1e-12 / 2e-5 single launch against general, 1e-9 per replayed step.  The
f32 fit boxes keep cond(K) <= 12801, so the "reference has no correct digit" exit must not fire anywhere in this module."""
import math

import numpy as np
import pytest

import parity_rules as PR
import small_regime_cases as SC
from hbetune_rs_amd import gpr
from oracle import gpr_oracle as O
from oracle import referee as R
from test_gpu_fit import replay_on_host_state_machine
from test_gpu_model_kinds import captured_buffer

pytestmark = pytest.mark.gpu

CMP_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 2e-5}  # single launch against the general path
REPLAY_TOL = 1e-9


def _name(dtype):
    return np.dtype(dtype).name


# ------------------------------------------------------------------------------------------------------------- A. evaluation
def _evaluate(X, y, theta, nu, Xq):
    prob = gpr.Problem(X, y, nu=nu)
    lml, grad = prob.lml_with_gradient(theta)
    alpha, kinv, ldiag = prob.results()
    prob.close()
    fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    mean, var, _ = fk.predict(Xq)
    a2, k2 = fk.arrays()
    out = dict(lml=lml, grad=grad, alpha=alpha, kinv=kinv, ldiag=ldiag, model_lml=fk.lml, mean=mean, var=var, a2=a2, k2=k2)
    fk.release()
    return out


def check_grad_groups(what, grad, ref_grad, tol):
    """Per group, relative to max(1, max |ref|) of the WHOLE gradient (parity_rules.dev's scale): a failure names the chunk."""
    grad, ref_grad = np.asarray(grad, np.float64), np.asarray(ref_grad, np.float64)
    scale = max(1.0, float(np.abs(ref_grad).max()))
    devs = [(name, float(np.abs(grad[sl] - ref_grad[sl]).max()) / scale) for name, sl in SC.grad_groups(len(ref_grad) - 2)]
    for name, v in devs:
        assert v <= tol, f"{what}: gradient group {name} off by {v:.2e} of the gradient's scale (bar {tol:g}); all groups: {devs}"
    return max(v for _, v in devs)


def check_against_oracle(what, got, X, y, theta, nu, Xq, tol):
    """One evaluation's results against the fp64 oracle at exp(theta); returns the deviations by quantity."""
    X64, y64, v = X.astype(np.float64), y.astype(np.float64), np.exp(theta)
    ref = O.lml_with_gradient(X64, y64, v[0], v[1], v[2:], nu)
    rm, rv, _ = O.predict(Xq.astype(np.float64), X64, ref["alpha"], ref["k_inv"], v[1], v[2:], nu)
    devs = dict(lml=PR.dev(got["lml"], ref["lml"]), model_lml=PR.dev(got["model_lml"], ref["lml"]),
                alpha=PR.dev(got["alpha"], ref["alpha"]), kinv=PR.dev(got["kinv"], ref["k_inv"]),
                ldiag=PR.dev(got["ldiag"], np.diag(ref["chol"])), a2=PR.dev(got["a2"], ref["alpha"]), k2=PR.dev(got["k2"], ref["k_inv"]),
                mean=PR.dev(got["mean"], rm), var=PR.dev(got["var"], np.maximum(rv, 0.0), scale=1.0) / v[1])
    for k, dv in devs.items():
        assert dv <= tol, f"{what}: {k} off by {dv:.2e} (bar {tol:g})"
    devs["grad"] = check_grad_groups(what, got["grad"], ref["grad"], tol)
    if len(y) == 1:  # one row: no pair of rows, the length-scale entries are exactly zero
        assert not np.asarray(got["grad"])[2:].any(), (what, got["grad"])
    return devs


def check_against_general(what, small, general, dtype):
    tol = CMP_TOL[np.dtype(dtype)]
    devs = {}
    for key in small:
        a, b = np.asarray(small[key], np.float64), np.asarray(general[key], np.float64)
        assert np.all(np.isfinite(a)), (what, key)
        if key == "grad":
            devs[key] = check_grad_groups(f"{what} against the general path", a, b, tol)
        else:
            devs[key] = PR.dev(a, b)
            assert devs[key] <= tol, f"{what}: {key} differs from the general path by {devs[key]:.2e} (bar {tol:g})"
    return devs


def _eval_params():
    return [pytest.param(d, n, nu, dt, id=f"d{d}-n{n}-nu{nu}-{_name(dt)}") for dt in SC.DTYPES for d, n, nu in SC.eval_cases(dt)]


@pytest.mark.parametrize("d,n,nu,dtype", _eval_params())
def test_one_evaluation_in_one_launch(d, n, nu, dtype, monkeypatch):
    X, y, theta = SC.inputs(d, n, dtype)
    Xq = SC.query_points(X, dtype)
    what = f"d={d} n={n} nu={nu} {_name(dtype)}"
    small = _evaluate(X, y, theta, nu, Xq)
    monkeypatch.setenv("HBEGP_SMALL", "0")
    general = _evaluate(X, y, theta, nu, Xq)
    tol = SC.tol_of(dtype)
    d_o = check_against_oracle(f"single launch {what}", small, X, y, theta, nu, Xq, tol)
    d_g = check_against_general(f"single launch {what}", small, general, dtype)
    print(f"SR eval {what}: oracle " + " ".join(f"{k} {v:.2e}" for k, v in d_o.items()) + f" (bar {tol:g}); general " +
          " ".join(f"{k} {v:.2e}" for k, v in d_g.items()) + f" (bar {CMP_TOL[np.dtype(dtype)]:g})")


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=_name)
def test_past_32_features_an_evaluation_takes_the_general_path(dtype, monkeypatch):
    d, n, nu = SC.CONTROL_CASE
    X, y, theta = SC.inputs(d, n, dtype)
    Xq = SC.query_points(X, dtype)
    first = _evaluate(X, y, theta, nu, Xq)
    monkeypatch.setenv("HBEGP_SMALL", "0")
    second = _evaluate(X, y, theta, nu, Xq)
    for key in first:  # the switch selects nothing at d = 33: the same launches, the same bits
        assert np.array_equal(np.asarray(first[key]), np.asarray(second[key])), key
    tol = SC.tol_of(dtype)
    d_o = check_against_oracle(f"control d={d} n={n} nu={nu} {_name(dtype)}", first, X, y, theta, nu, Xq, tol)
    print(f"SR control d={d} n={n} nu={nu} {_name(dtype)}: oracle " + " ".join(f"{k} {v:.2e}" for k, v in d_o.items()) + f" (bar {tol:g})")


# -------------------------------------------------------------------------------------------------------------------- B. fit
_FITS = {}


def _fit(case, maxeval=None):
    """The case's fit, run once per session: inputs, trace and everything read from the model (the handle is released)."""
    if (case, maxeval) in _FITS:
        return _FITS[(case, maxeval)]
    d, n, nu, dtype, fixed = case
    X, y, theta = SC.inputs(d, n, dtype)
    lo, hi = SC.fit_box(theta, dtype)
    starts = SC.fit_starts(d, n, lo, hi, dtype)
    key, maxeval = (case, maxeval), maxeval or SC.MAXEVAL[np.dtype(dtype)]
    fk = gpr.FittedKernel.new(X, y, theta, lo, hi, starts, nu=nu, maxeval=maxeval, trace=True, fixed_work=fixed)
    alpha, kinv = fk.arrays()
    Xq = SC.query_points(X, dtype)
    mean, var, _ = fk.predict(Xq)
    out = dict(X=X, y=y, theta0=theta, lo=lo, hi=hi, starts=starts, maxeval=maxeval, trace=fk.trace, lml=fk.lml, theta=fk.theta.copy(),
               n_evals=fk.n_evals, params=fk.device_params(), alpha=alpha, kinv=kinv, Xq=Xq, mean=mean, var=var)
    fk.release()
    _FITS[key] = out
    return out


def check_trace(what, tr, X, y, nu, lo, hi, dtype):
    """Every traced evaluation against O.objective in the element type through the Judge (tests/test_gpu_fit.py), the gradient
    per group on the scale of the whole gradient.  Returns (judge of the lml, judge of the gradient groups)."""
    f32 = SC.is_f32(dtype)
    tol = SC.tol_of(dtype)
    bounds = list(zip(lo, hi))
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    groups = SC.grad_groups(X.shape[1])
    jl, jg = PR.Judge(tol), PR.Judge(tol)
    for i in range(len(tr["lml"])):
        th = tr["theta"][i]
        assert np.all(th >= np.log(lo) - 1e-12) and np.all(th <= np.log(hi) + 1e-12), (what, i, th)
        f, g, res = O.objective(th, X, y, nu, bounds)
        if res is None:
            assert not f32, f"{what}: LAPACK f32 failed at evaluation {i} inside a box with cond(K) <= {SC.COND32_BOUND:.0f}"
            assert tr["lml"][i] == -math.inf, (what, i)
            continue
        assert math.isfinite(tr["lml"][i]), f"{what}: evaluation {i} failed on the device where the oracle gives {-f}"
        rf, kap = [], []

        def truth(kind, th=th, rf=rf):
            if not rf:
                rf.append(PR.referee_for(X64, y64, th, bounds, nu))
            return np.array([rf[0].lml()]) if kind == "lml" else rf[0].gradient()

        def kappa(kind, th=th, kap=kap):
            if not kap:
                kap.append(PR.sigma32(X64, y64, th, bounds, nu))
            return kap[0][kind]

        jl.check(f"{what}: lml of evaluation {i}", [tr["lml"][i]], [-f], lambda: truth("lml"), sigma_fn=(lambda: kappa("lml")) if f32 else None)
        scale = float(np.abs(g).max())
        for name, sl in groups:
            jg.check(f"{what}: gradient group {name} of evaluation {i}", tr["grad"][i][sl], -g[sl], lambda sl=sl: truth("grad")[sl], scale=scale,
                     sigma_fn=(lambda sl=sl: kappa("grad")[sl]) if f32 else None)
        if rf:
            rf[0].close()
    assert jl.n_nodigits == 0 and jg.n_nodigits == 0, (what, jl.summary(), jg.summary())
    return jl, jg


def check_capture(what, fit, nu, dtype):
    """fit.rs:116-125: the model is the first maximum of the trace -- its lml, its theta, its exp / clamp, and alpha / K^-1 of
    that evaluation (copied out of the ping-pong buffer that held it).  Returns the judge of the two arrays."""
    tr, lo, hi = fit["trace"], fit["lo"], fit["hi"]
    i_best = int(np.argmax(tr["lml"]))  # the first occurrence of the maximum, the trace being in (run, evaluation) order
    assert fit["lml"] == tr["lml"][i_best] == tr["lml"].max(), (what, fit["lml"], tr["lml"][i_best])
    # the model's theta is log(clamp(exp(theta))) of the captured evaluation's theta (fit.rs:155-164): exp's rounding moves the
    # log by an eps, the log's own rounding by |theta| eps -- the allowance of the exp / clamp below, in log space
    th_best = tr["theta"][i_best]
    assert (np.abs(fit["theta"] - th_best) <= (np.abs(th_best) + 2) * np.finfo(float).eps).all(), (what, fit["theta"] - th_best)
    bounds = list(zip(lo, hi))
    noise, amp, ell = fit["params"]
    w_noise, w_amp, w_ell = PR.clamped_params(fit["theta"], bounds)
    got, want = np.concatenate([[noise, amp], ell]), np.concatenate([[w_noise, w_amp], w_ell])
    assert (np.abs(got - want) <= (np.abs(fit["theta"]) + 2) * np.finfo(float).eps * want).all(), (what, got, want)
    X, y = fit["X"], fit["y"]
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    f, g, res = O.objective(tr["theta"][i_best], X, y, nu, bounds)
    assert res is not None, what
    assert np.all(np.isfinite(fit["alpha"])) and np.all(np.isfinite(fit["kinv"]))
    rf = PR.referee_for(X64, y64, tr["theta"][i_best], bounds, nu)
    kb = PR.sigma32(X64, y64, tr["theta"][i_best], bounds, nu) if SC.is_f32(dtype) else None
    jm = PR.Judge(SC.tol_of(dtype))
    jm.check(f"{what}: alpha of the fitted model", fit["alpha"], res["alpha"], lambda: sum(rf.alpha()), sigma_fn=(lambda: kb["alpha"]) if kb else None)
    jm.check(f"{what}: K^-1 of the fitted model", fit["kinv"], res["k_inv"], lambda: sum(rf.kinv()), sigma_fn=(lambda: kb["kinv"]) if kb else None)
    rf.close()
    assert jm.n_nodigits == 0, (what, jm.summary())
    return jm


def check_predict(what, fit, nu, dtype):
    """predict of the fitted model at five points against the oracle of the element type at device_params(), the referee where
    the plain bar fails (tests/test_gpu_fit.py)."""
    X, y, Xq = fit["X"], fit["y"], fit["Xq"]
    noise, amp, ell = fit["params"]
    assert np.all(np.isfinite(fit["mean"])) and np.all(fit["var"] >= 0)
    rp = O.extend(X, y, noise, amp, ell, nu)
    om, ov, _ = O.predict(Xq, X, rp["alpha"], rp["k_inv"], amp, ell, nu)
    rfp = R.Referee(X.astype(np.float64), y.astype(np.float64), noise, amp, ell, nu)
    jp = PR.Judge(SC.tol_of(dtype))
    jp.check(f"{what}: predict mean of the fitted model", fit["mean"], om, lambda: rfp.predict(Xq.astype(np.float64))[0])
    jp.check(f"{what}: predict variance of the fitted model", fit["var"], ov, lambda: rfp.predict(Xq.astype(np.float64))[1], scale=amp)
    rfp.close()
    assert jp.n_nodigits == 0, (what, jp.summary())
    return jp


def _check_fit(case, device_driven):
    d, n, nu, dtype, fixed = case
    what = "fit " + SC.fit_id(case)
    fit = _fit(case)
    tr, maxeval = fit["trace"], fit["maxeval"]
    n_runs = 1 + len(fit["starts"])
    assert set(tr["run"].tolist()) == set(range(n_runs)) and len(tr["lml"]) == fit["n_evals"] <= n_runs * maxeval
    assert np.all(np.diff(tr["run"]) >= 0)  # run by run
    jl, jg = check_trace(what, tr, fit["X"], fit["y"], nu, fit["lo"], fit["hi"], dtype)
    jm = check_capture(what, fit, nu, dtype)
    jp = check_predict(what, fit, nu, dtype)
    # the optimiser, both directions: fed the run's recorded evaluations, the host state machine (csrc/lbfgs_step.hpp) asks for
    # the points the device went on to evaluate, and wants no further point after the device's last one
    worst_step, lengths = replay_on_host_state_machine(tr, fit["theta0"], fit["starts"], np.log(fit["lo"]), np.log(fit["hi"]), maxeval, fixed)
    assert worst_step <= REPLAY_TOL, f"{what}: the device's and the host's iterates differ by {worst_step:.2e} of max(1, |theta|)"
    if fixed:
        assert lengths == [maxeval] * n_runs, (what, lengths)
    buf = captured_buffer(tr) if device_driven else None
    print(f"SR {what} p={d + 2} evaluations {lengths}: trace lml [{jl.summary()}]; trace gradient groups [{jg.summary()}]; model arrays "
          f"[{jm.summary()}]; predict [{jp.summary()}]; replay step {worst_step:.2e} (bar {REPLAY_TOL:g}); " +
          (f"captured buffer {buf[0]} (run {buf[1]}, evaluation {buf[2]})" if device_driven else "host-driven"))


@pytest.mark.parametrize("case", SC.FIT_CASES, ids=SC.fit_id)
def test_device_driven_fit(case):
    _check_fit(case, device_driven=True)


def test_past_32_features_the_host_drives_the_fit():
    _check_fit(SC.FIT_CONTROL, device_driven=False)


SEEDED_FACTOR = 16.0


def replay_sensitivity(tr, theta0, starts, lnlo, lnhi, maxeval):
    """What the replay itself does to one ulp: every run replayed on the host state machine with ONE coordinate of its start
    point moved up by one ulp (each coordinate in turn), fed the recorded (f, g) all the same.  Returns the worst
    |theta_seeded - theta_recorded| / max(1, |theta|) over the steps both have.  The host follows its own iterates while the
    curvature pairs take y from the recorded gradients, so near convergence (|s| ~ 1e-6) a difference of an ulp in x turns into
    a relative 1e-10 in s and from there into the next directions: over a run of 100+ evaluations at d = 25 it grows to 1e-7."""
    import ctypes as C

    from hbetune_rs_amd import _lib

    lib = _lib.load()
    p = len(theta0)
    lnlo, lnhi = np.ascontiguousarray(lnlo, dtype=np.float64), np.ascontiguousarray(lnhi, dtype=np.float64)
    worst = 0.0
    for r in sorted(set(tr["run"].tolist())):
        idx = np.nonzero(tr["run"] == r)[0]
        L = len(idx)
        th = tr["theta"][idx]
        f = np.ascontiguousarray(np.where(np.isfinite(tr["lml"][idx]), -tr["lml"][idx], np.inf))
        g = np.ascontiguousarray(-tr["grad"][idx])
        for j in range(p):
            x0 = np.array(theta0 if r == 0 else starts[r - 1], dtype=np.float64)
            x0[j] = np.nextafter(x0[j], np.inf)
            req, nreq = np.zeros((L, p)), C.c_int(0)
            assert lib.hbegp_debug_lbfgs_replay(p, _lib.dptr(x0), _lib.dptr(lnlo), _lib.dptr(lnhi), maxeval, 0, 0, L, _lib.dptr(f), _lib.dptr(g),
                                                _lib.dptr(req), C.byref(nreq)) == 0
            k = nreq.value
            worst = max(worst, float(np.max(np.abs(req[:k] - th[:k]) / np.maximum(1.0, np.abs(th[:k])))))
    return worst


@pytest.mark.parametrize("case", SC.LONG_FIT_CASES, ids=SC.fit_id)
def test_a_run_that_ends_by_its_own_decision_ends_where_the_host_ends(case):
    """With the grid's 30 / 20 evaluations only the d = 1 runs stop by the pgtol / ftol tests; every other run ends at maxeval.
    These fits have the library's default of 150 evaluations, inside which runs at p = 11, 19, 27 and 34 converge (found on the
    CPU with the oracle as the objective), so wl_advance's stop decisions are replayed at every width of the wave-wide state
    machine.  The arithmetic of the evaluations is the grid's business: here the capture and the optimiser alone.

    The step bar: 1e-9 was measured on runs of up to 40 evaluations.  Over 100+ evaluations the replay amplifies ulps by itself
    (replay_sensitivity: at d = 25 a start point moved by ONE ulp ends 1.5e-7 away from the recorded iterates, on the host alone, where
    the device is 1.4e-7 away; DESIGN.md section 27 has all six pairs).
    The device differs from the host by an ulp-level amount in each of the about five reductions of every iteration, not once, so
    it may be SEEDED_FACTOR = 16 times as far as the worst single seeded ulp (three iterations' worth of injections inside the
    amplifying stretch); a wrong decision moves an iterate by a whole step, 1e-3 and more.  The allowance is
    max(1e-9, 16 x seeded) and is computed from the host state machine alone."""
    what = f"long fit {SC.fit_id(case)}"
    fit = _fit(case, SC.LONG_MAXEVAL)
    tr = fit["trace"]
    assert np.all(np.diff(tr["run"]) >= 0) and len(tr["lml"]) == fit["n_evals"]
    jm = check_capture(what, fit, case[2], case[3])
    lnlo, lnhi = np.log(fit["lo"]), np.log(fit["hi"])
    worst_step, lengths = replay_on_host_state_machine(tr, fit["theta0"], fit["starts"], lnlo, lnhi, SC.LONG_MAXEVAL, False)
    seeded = replay_sensitivity(tr, fit["theta0"], fit["starts"], lnlo, lnhi, SC.LONG_MAXEVAL)
    allowed = max(REPLAY_TOL, SEEDED_FACTOR * seeded)
    print(f"SR {what} p={case[0] + 2} evaluations {lengths} of at most {SC.LONG_MAXEVAL}: replay step {worst_step:.2e}, one seeded ulp on the "
          f"host alone {seeded:.2e} (allowance {allowed:.2e}); model arrays [{jm.summary()}]")
    assert worst_step <= allowed, f"{what}: the device's and the host's iterates differ by {worst_step:.2e} of max(1, |theta|)"
    assert min(lengths) < SC.LONG_MAXEVAL, f"{what}: no run stopped by its own decision {lengths}: the case needs other data"


def test_both_ping_pong_buffers_are_captured_somewhere_in_the_grid():
    """make_model copies the model out of the buffer that holds the winning run's best evaluation: the grid must exercise both.
    (Fits another test of this session ran are reused; a fit is one launch.)"""
    seen = {SC.fit_id(case): captured_buffer(_fit(case)["trace"])[0] for case in SC.FIT_CASES}
    print("SR captured buffers: " + ", ".join(f"{k}: {v}" for k, v in seen.items()))
    assert set(seen.values()) == {0, 1}, seen
