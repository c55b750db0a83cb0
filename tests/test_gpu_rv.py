"""GPU: known per-row noise variances on the diagonal (the `_rv` entry points) against tests/rv_ref.py.

K = c Matern + diag(s2 + v).  The inputs are rv_ref.case's -- s2 = 0.05, c = 1.3, ell in [0.3, 1.3], v uniform in [0, 0.2] with every
seventh entry 0 -- which tests/test_rv_cpu.py checks against scikit-learn and whose cond(K) <= 1e4 it asserts, so LAPACK's digits
are not the limit of any comparison here.  Bars: parity_rules.TOL64 = 1e-8 and TOL32 = 1e-4, relative to max(1, scale of the
reference).  Every test calls a new symbol."""
import ctypes as C
import functools
import math
import os
import subprocess
import threading

import numpy as np
import pytest

import parity_rules as PRU
import paths_ref as PR
import rv_ref
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

SHAPES = rv_ref.GPU_SHAPES
NUS = rv_ref.NUS
DTYPES = (np.float64, np.float32)
# the box of the fits, around the case's own parameters (s2 = 0.05, c = 1.3, ell in [0.3, 1.3]; the optimiser bounds the noise in
# log space itself): tight enough that a run's evaluations stay well conditioned.  At its worst corner (lowest noise, largest
# amplitude, every length scale 1.3) cond(K) is 976 / 2,940 / 11,136 at n = 100 / 300 / 1024; _replay asserts cond(K) <= 1e4 on the
# reference's matrix of every traced evaluation, so that each can be replayed on LAPACK
FIT_LO = lambda d: np.array([0.045, 0.8] + [0.25] * d)  # noqa: E731
FIT_HI = lambda d: np.array([0.3, 1.5] + [1.3] * d)  # noqa: E731


def _tol(dtype):
    return PRU.TOL64 if np.dtype(dtype) == np.float64 else PRU.TOL32


def _name(dtype):
    return np.dtype(dtype).name


@functools.lru_cache(maxsize=None)
def _case(n, d):
    return rv_ref.case(n, d)


@functools.lru_cache(maxsize=None)
def _reference(n, d, nu, dtype_name):
    """rv_ref's evaluation of the case as the device sees it: the inputs rounded to the element type, v included."""
    X, y, v, theta = _case(n, d)
    dt = np.dtype(dtype_name)
    return rv_ref.evaluate(X.astype(dt).astype(np.float64), y.astype(dt).astype(np.float64), v.astype(dt).astype(np.float64), theta, nu)


def _evaluate(X, y, v, theta, nu, dtype, want_kinv=True):
    """One evaluation through hbegp_problem_create_rv_* (v None: the plain problem): lml, grad, alpha, K^-1, diag L."""
    prob = gpr.Problem(X.astype(dtype), y.astype(dtype), nu=nu, row_variance=v)
    try:
        lml, grad = prob.lml_with_gradient(theta)
        alpha, kinv, ldiag = prob.results(want_kinv=want_kinv)
    finally:
        prob.close()
    return lml, grad, alpha, kinv, ldiag


def _raw_model(handle, dtype, n, d, nu):
    return gpr.FittedKernel(handle, dtype, n, d, nu)


def _raw_extend_rv(X, y, rv, theta, nu, dtype):
    """hbegp_extend_rv_* called directly, so that rv may be NULL (the Python wrapper calls the plain symbol then)."""
    lib = _lib.load()
    X, y = _lib.as_c(X, dtype), _lib.as_c(y, dtype)
    n, d = X.shape
    h = C.c_void_p()
    fn = getattr(lib, "hbegp_extend_rv_" + ("f64" if np.dtype(dtype) == np.float64 else "f32"))
    _lib.check(fn(gpr.default_context()._h, _lib.aptr(X), _lib.aptr(y), _lib.dptr(rv), n, d, float(nu), _lib.dptr(_lib.as_c(theta, np.float64)),
                  None, None, C.byref(h)))
    return _raw_model(h, dtype, n, d, nu)


def _raw_fit_rv(symbol, X, y, rv, theta0, lo, hi, starts, nu, dtype, maxeval):
    """hbegp_fit_rv_* / hbegp_fit_loo_rv_* called directly (rv may be NULL): (model, theta_best, best)."""
    lib = _lib.load()
    X, y = _lib.as_c(X, dtype), _lib.as_c(y, dtype)
    n, d = X.shape
    p = d + 2
    starts_c = _lib.as_c(np.asarray(starts).reshape(-1, p), np.float64)
    opt = _lib.FitOptions()
    opt.maxeval = maxeval
    h = C.c_void_p()
    theta_best, best = np.zeros(p), C.c_double()
    fn = getattr(lib, symbol + ("_f64" if np.dtype(dtype) == np.float64 else "_f32"))
    _lib.check(fn(gpr.default_context()._h, _lib.aptr(X), _lib.aptr(y), _lib.dptr(rv), n, d, float(nu), _lib.dptr(_lib.as_c(theta0, np.float64)),
                  _lib.dptr(_lib.as_c(lo, np.float64)), _lib.dptr(_lib.as_c(hi, np.float64)), _lib.dptr(starts_c), len(starts_c), C.byref(opt),
                  _lib.dptr(theta_best), C.byref(best), C.byref(h)))
    return _raw_model(h, dtype, n, d, nu), theta_best, best.value


def _starts(d, k, seed):
    lo, hi = np.log(FIT_LO(d)), np.log(FIT_HI(d))
    return lo[None, :] + (hi - lo)[None, :] * np.random.default_rng(seed).random((k, d + 2))


def _model_outputs(fk, Xs):
    alpha, kinv = fk.arrays()
    mean, var, _ = fk.predict(Xs)
    return [np.array(fk.lml), fk.theta.copy(), alpha, kinv, mean, var]


def _same_bytes(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. one evaluation against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_one_evaluation_matches_the_reference(n, d, nu, dtype):
    X, y, v, theta = _case(n, d)
    ref = _reference(n, d, nu, _name(dtype))
    lml, grad, alpha, kinv, ldiag = _evaluate(X, y, v, theta, nu, dtype)
    tol = _tol(dtype)
    devs = dict(lml=PRU.dev(lml, ref["lml"]), grad=PRU.dev(grad, ref["grad"]), alpha=PRU.dev(alpha, ref["alpha"]),
                kinv=PRU.dev(kinv, ref["kinv"]), ldiag=PRU.dev(ldiag, ref["ldiag"]))
    print(f"n={n} d={d} nu={nu} {_name(dtype)}: " + ", ".join(f"{k} {x:.2e}" for k, x in devs.items()) + f" (bar {tol:g})")
    for k, x in devs.items():
        assert x <= tol, (k, x)


# ---- 2. v = 0 and rv = NULL give the plain call's bytes ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,d", [(100, 8), (200, 9), (1024, 8)])
def test_zero_variances_and_null_give_the_plain_bytes(n, d, dtype):
    X, y, _, theta = _case(n, d)
    X, y = X.astype(dtype), y.astype(dtype)
    Xs = np.random.default_rng(2).random((9, d)).astype(dtype)
    zeros = np.zeros(n)
    # extend
    plain = gpr.FittedKernel.extend(X, y, theta)
    want = _model_outputs(plain, Xs)
    assert plain.row_variance is None
    for rv in (zeros, None):
        fk = _raw_extend_rv(X, y, rv, theta, 2.5, dtype)
        assert _same_bytes(_model_outputs(fk, Xs), want), ("extend", rv is None)
        assert (fk.row_variance is None) == (rv is None)
        fk.release()
    plain.release()
    # fit and LOO fit: the same runs, the same captured evaluation, the same model
    lo, hi, starts = FIT_LO(d), FIT_HI(d), _starts(d, 2, 7)
    maxeval = 12 if n <= 200 else 6
    for symbol, new in (("hbegp_fit_rv", gpr.FittedKernel.new), ("hbegp_fit_loo_rv", gpr.FittedKernel.new_by_loo)):
        plain = new(X, y, theta, lo, hi, starts, maxeval=maxeval)
        want = _model_outputs(plain, Xs) + [plain.theta_best]
        for rv in (zeros, None):
            fk, theta_best, best = _raw_fit_rv(symbol, X, y, rv, theta, lo, hi, starts, 2.5, dtype, maxeval)
            assert _same_bytes(_model_outputs(fk, Xs) + [theta_best], want), (symbol, rv is None)
            if symbol == "hbegp_fit_loo_rv":
                assert best == plain.loo_best
            fk.release()
        plain.release()


# ---- 3. a constant v is a shift of the noise -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,d,nu", [(n, d, 2.5) for n, d in SHAPES] + [(200, 9, 0.5), (200, 9, 1.5), (200, 9, math.inf), (100, 8, 0.5)])
def test_constant_variance_is_a_noise_shift(n, d, nu, dtype):
    """The check that does not use the new reference: v = 0.07 everywhere at noise s2 is the plain evaluation at noise s2 + 0.07;
    only the noise entry of the gradient differs, by the factor s2 / (s2 + 0.07) (d/d ln s2 of the same matrix)."""
    X, y, _, theta = _case(n, d)
    shift = rv_ref.SHIFT
    got = _evaluate(X, y, np.full(n, shift), theta, nu, dtype)
    theta2 = theta.copy()
    theta2[0] = math.log(math.exp(theta[0]) + shift)
    want = _evaluate(X, y, None, theta2, nu, dtype)
    tol = _tol(dtype)
    grad_want = want[1].copy()
    grad_want[0] *= math.exp(theta[0]) / (math.exp(theta[0]) + shift)
    devs = [PRU.dev(got[0], want[0]), PRU.dev(got[1], grad_want), PRU.dev(got[2], want[2]), PRU.dev(got[3], want[3]), PRU.dev(got[4], want[4])]
    print(f"n={n} d={d} nu={nu} {_name(dtype)}: lml, grad, alpha, kinv, ldiag off by " + ", ".join(f"{x:.2e}" for x in devs) + f" (bar {tol:g})")
    assert max(devs) <= tol, devs
    Xs = np.random.default_rng(4).random((11, d)).astype(dtype)
    a = gpr.FittedKernel.extend(X.astype(dtype), y.astype(dtype), theta, nu=nu, row_variance=np.full(n, shift))
    b = gpr.FittedKernel.extend(X.astype(dtype), y.astype(dtype), theta2, nu=nu)
    ma, va, _ = a.predict(Xs)
    mb, vb, _ = b.predict(Xs)
    a.release(); b.release()
    assert PRU.dev(ma, mb) <= tol and PRU.dev(va, vb) <= tol


# ---- 4. fits -------------------------------------------------------------------------------------------------------------------
def _replay(tr, X, y, v, nu, dtype, loo, what, want_grad=True):
    dt = np.dtype(dtype)
    Xr, yr, vr = (a.astype(dt).astype(np.float64) for a in (X, y, v))
    tol, worst, worst_cond = _tol(dtype), [0.0, 0.0], 0.0
    assert len(tr["lml"]) > 0
    for i, th in enumerate(tr["theta"]):
        worst_cond = max(worst_cond, rv_ref.cond(rv_ref.kernel_matrix(Xr, vr, th, nu)))
        if loo:
            ref = rv_ref.loo(Xr, yr, vr, th, nu, want_grad=want_grad)
            val = ref["loo"]
        else:
            ref = rv_ref.evaluate(Xr, yr, vr, th, nu, want_grad=want_grad)
            val = ref["lml"]
        worst[0] = max(worst[0], PRU.dev(tr["lml"][i], val))
        if want_grad:
            worst[1] = max(worst[1], PRU.dev(tr["grad"][i], ref["grad"]))
    print(f"{what}: {len(tr['lml'])} traced evaluations, value off by {worst[0]:.2e}, gradient by {worst[1]:.2e} (bar {tol:g}), "
          f"largest cond(K) {worst_cond:.0f}")
    assert worst_cond <= rv_ref.COND_MAX, worst_cond
    assert worst[0] <= tol and worst[1] <= tol, worst


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,d", [(100, 8), (300, 9)])  # device-driven (one launch per run) and host-driven
def test_fit_trace_replays_on_the_reference_and_the_model_is_extend(n, d, dtype):
    X, y, v, theta = _case(n, d)
    Xd, yd = X.astype(dtype), y.astype(dtype)
    lo, hi = FIT_LO(d), FIT_HI(d)
    fk = gpr.FittedKernel.new(Xd, yd, theta, lo, hi, _starts(d, 2, 11), maxeval=40, trace=True, row_variance=v)
    assert len(np.unique(fk.trace["run"])) == 3 and fk.n_not_pd == 0
    _replay(fk.trace, X, y, v, 2.5, dtype, False, f"fit n={n} {_name(dtype)}")
    np.testing.assert_array_equal(fk.row_variance, v.astype(dtype).astype(np.float64))
    # The model is `extend`, bit for bit, at the theta the captured evaluation ran with: the trace's, as the optimiser passed it
    # (tests/test_gpu_fit.py has the same for the plain fit).  theta_best is log(clamp(exp(that theta))) (fit.rs:155-164): exp's
    # rounding moves the log by an eps and the log's own by |theta| eps, so theta_best may differ from the captured theta in the
    # last bit, and an evaluation at another theta is another matrix -- equality of bits at theta_best cannot be asked.  What holds
    # there: theta_best is the captured theta within that rounding (the optimiser keeps theta inside the box, so the clamp moves it by no more), and `extend` at it is the
    # model within the bar.
    best = int(np.argmax(fk.trace["lml"]))
    th_cap = fk.trace["theta"][best]
    assert fk.trace["lml"][best] == fk.lml
    assert np.all(np.abs(fk.theta_best - th_cap) <= (np.abs(th_cap) + 2) * np.finfo(float).eps), fk.theta_best - th_cap
    assert np.array_equal(fk.theta_best, fk.theta)
    ex = gpr.FittedKernel.extend(Xd, yd, th_cap, lo, hi, row_variance=v)
    if np.dtype(dtype) == np.float64:
        assert ex.lml == fk.lml
        assert _same_bytes(list(fk.arrays()), list(ex.arrays()))
    else:
        assert PRU.dev(ex.lml, fk.lml) <= PRU.TOL32
    at_best = gpr.FittedKernel.extend(Xd, yd, fk.theta_best, lo, hi, row_variance=v)
    _compare_models(at_best, fk, _tol(dtype), f"extend at theta_best vs the fitted model n={n} {_name(dtype)}")
    fk.release(); ex.release(); at_best.release()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_loo_fit_trace_replays_on_the_reference(dtype):
    n, d = 100, 8
    X, y, v, theta = _case(n, d)
    Xd, yd = X.astype(dtype), y.astype(dtype)
    lo, hi = FIT_LO(d), FIT_HI(d)
    fk = gpr.FittedKernel.new_by_loo(Xd, yd, theta, lo, hi, _starts(d, 2, 12), maxeval=40, trace=True, row_variance=v)
    _replay(fk.trace, X, y, v, 2.5, dtype, True, f"LOO fit n={n} {_name(dtype)}")
    assert fk.loo_best == fk.trace["lml"].max()
    ex = gpr.FittedKernel.extend(Xd, yd, fk.theta_best, row_variance=v)  # hbegp_fit_loo's model IS extend at theta_best
    assert _same_bytes(list(fk.arrays()), list(ex.arrays())) and ex.lml == fk.lml
    fk.release(); ex.release()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_fit_through_the_task_queue_replays_on_the_reference(dtype):
    """n = 1024: eight blocks, the task queue inside a fit, line-search trials in two phases (an lml-only trace leaves them on)."""
    n, d = 1024, 8
    X, y, v, theta = _case(n, d)
    fk = gpr.FittedKernel.new(X.astype(dtype), y.astype(dtype), theta, FIT_LO(d), FIT_HI(d), _starts(d, 1, 13), maxeval=12, trace="lml",
                              row_variance=v)
    _replay(fk.trace, X, y, v, 2.5, dtype, False, f"fit n={n} {_name(dtype)}", want_grad=False)
    fk.release()


# ---- 5. threads ----------------------------------------------------------------------------------------------------------------
def test_concurrent_small_fits_return_their_solo_bits():
    n, d = 100, 8
    X, y, v, theta = _case(n, d)
    lo, hi, starts = FIT_LO(d), FIT_HI(d), _starts(d, 2, 21)
    v2 = np.roll(v, 3) * 0.5
    Xs = np.random.default_rng(6).random((7, d))

    def job(kind):
        if kind == "plain":
            fk = gpr.FittedKernel.new(X, y, theta, lo, hi, starts, maxeval=30)
        else:
            rv = {"v": v, "v2": v2, "null": None}[kind]
            fk = _raw_fit_rv("hbegp_fit_rv", X, y, rv, theta, lo, hi, starts, 2.5, np.float64, 30)[0]
        out = _model_outputs(fk, Xs)
        fk.release()
        return out

    kinds = ["v", "v2", "null", "plain"]
    solo = {k: job(k) for k in kinds}
    assert _same_bytes(solo["null"], solo["plain"]) and not _same_bytes(solo["v"], solo["v2"]) and not _same_bytes(solo["v"], solo["plain"])
    for rep in range(3):
        got, errs = {}, []
        barrier = threading.Barrier(len(kinds))

        def run(k):
            try:
                barrier.wait()
                got[k] = job(k)
            except Exception as e:  # noqa: BLE001 -- reported below
                errs.append((k, repr(e)))

        threads = [threading.Thread(target=run, args=(k,)) for k in kinds]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errs, errs
        for k in kinds:
            assert _same_bytes(got[k], solo[k]), (rep, k)


# ---- 6. incremental extend -----------------------------------------------------------------------------------------------------
def _compare_models(a, b, tol, what):
    aa, ka = a.arrays()
    ab, kb = b.arrays()
    devs = [PRU.dev(a.lml, b.lml), PRU.dev(aa, ab), PRU.dev(ka, kb)]
    print(f"{what}: lml, alpha, K^-1 off by " + ", ".join(f"{x:.2e}" for x in devs) + f" (bar {tol:g})")
    assert max(devs) <= tol, (what, devs)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_incremental_extend_with_row_variances(dtype):
    n0, n, d = 256, 300, 9
    X, y, v, theta = _case(n, d)
    Xd, yd = X.astype(dtype), y.astype(dtype)
    tol = _tol(dtype)
    prior = gpr.FittedKernel.extend(Xd[:n0], yd[:n0], theta, row_variance=v[:n0])
    full = gpr.FittedKernel.extend(Xd, yd, theta, row_variance=v)
    inc = prior.extend_with(Xd, yd, row_variance=v)
    assert inc.incremental
    np.testing.assert_array_equal(inc.row_variance, v.astype(dtype).astype(np.float64))
    _compare_models(inc, full, tol, f"incremental vs full {_name(dtype)}")
    ref = rv_ref.evaluate(*(a.astype(dtype).astype(np.float64) for a in (X, y, v)), theta, 2.5, want_grad=False)
    ai, ki = inc.arrays()
    assert PRU.dev(inc.lml, ref["lml"]) <= tol and PRU.dev(ai, ref["alpha"]) <= tol and PRU.dev(ki, ref["kinv"]) <= tol
    # one changed v_i inside the prefix: the full path, and its bytes
    v2 = v.copy()
    v2[17] += 0.01
    res = prior.extend_with(Xd, yd, row_variance=v2)
    assert not res.incremental
    full2 = gpr.FittedKernel.extend(Xd, yd, theta, row_variance=v2)
    assert _same_bytes(list(res.arrays()) + [np.array(res.lml)], list(full2.arrays()) + [np.array(full2.lml)])
    # the plain call on a prior that carries v is refused, and says which call to use
    with pytest.raises(gpr.HbegpError) as e:
        prior.extend_with(Xd, yd)
    assert e.value.code == _lib.EINVAL and "hbegp_extend_from_rv" in str(e.value)
    # ... and so is its `_rv` form with rv = NULL, which is the plain call
    h, flag = C.c_void_p(0x5A5A), C.c_int(7)
    fn = getattr(_lib.load(), "hbegp_extend_from_rv_" + ("f64" if np.dtype(dtype) == np.float64 else "f32"))
    assert fn(gpr.default_context()._h, prior._h, _lib.aptr(Xd), _lib.aptr(yd), None, n, C.byref(h), C.byref(flag)) == _lib.EINVAL
    assert "hbegp_extend_from_rv" in _lib.last_error() and h.value == 0x5A5A and flag.value == 7
    # a prior without v counts as zeros: new rows with v extend it incrementally; a non-zero v in the prefix does not
    plain_prior = gpr.FittedKernel.extend(Xd[:n0], yd[:n0], theta)
    v3 = np.concatenate([np.zeros(n0), v[n0:]])
    inc3 = plain_prior.extend_with(Xd, yd, row_variance=v3)
    full3 = gpr.FittedKernel.extend(Xd, yd, theta, row_variance=v3)
    assert inc3.incremental
    _compare_models(inc3, full3, tol, f"plain prior + new rows with v {_name(dtype)}")
    res4 = plain_prior.extend_with(Xd, yd, row_variance=v)
    assert not res4.incremental
    for fk in (prior, full, inc, res, full2, plain_prior, inc3, full3, res4):
        fk.release()


def test_one_row_chain_with_row_variances():
    n, d = 258, 4
    X, y, v, theta = _case(n, d)
    fk = gpr.FittedKernel.extend(X[:256], y[:256], theta, row_variance=v[:256])
    for m in (257, 258):
        nxt = fk.extend_with(X[:m], y[:m], row_variance=v[:m])
        assert nxt.incremental and nxt.n == m
        fk.release()
        fk = nxt
    full = gpr.FittedKernel.extend(X, y, theta, row_variance=v)
    _compare_models(fk, full, PRU.TOL64, "chain 256 -> 257 -> 258")
    ref = rv_ref.evaluate(X, y, v, theta, 2.5, want_grad=False)
    assert PRU.dev(fk.lml, ref["lml"]) <= PRU.TOL64 and PRU.dev(fk.arrays()[0], ref["alpha"]) <= PRU.TOL64
    fk.release(); full.release()


# ---- 7. downstream of a model with v -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_downstream_of_a_model_with_row_variances(dtype):
    n, d, nu = 200, 9, 2.5
    X, y, v, theta = _case(n, d)
    Xd, yd = X.astype(dtype), y.astype(dtype)
    Xr, yr, vr = (a.astype(dtype).astype(np.float64) for a in (X, y, v))
    tol = _tol(dtype)
    fk = gpr.FittedKernel.extend(Xd, yd, theta, nu=nu, row_variance=v)
    ref = _reference(n, d, nu, _name(dtype))
    # the model's variances: the rounded values, widened
    got_v = fk.row_variance
    assert got_v.dtype == np.float64 and np.array_equal(got_v, v.astype(dtype).astype(np.float64))
    # predict: the latent function's mean and variance
    Xs = np.random.default_rng(8).random((150, d)).astype(dtype)
    mean, var, _ = fk.predict(Xs)
    rmean, rvar = rv_ref.predict(Xs.astype(np.float64), Xr, ref, theta, nu)
    assert PRU.dev(mean, rmean) <= tol and PRU.dev(var, rvar, scale=rv_ref.AMP) <= tol
    # leave-one-out: the variance is the noisy observation's, s2 + v_i included
    lmean, lvar, lpd, loo, lgrad = fk.loo(want_grad=True)
    rl = rv_ref.loo(Xr, yr, vr, theta, nu)
    devs = [PRU.dev(lmean, rl["mean"]), PRU.dev(lvar, rl["var"]), PRU.dev(lpd, rl["lpd"]), PRU.dev(loo, rl["loo"]), PRU.dev(lgrad, rl["grad"])]
    print(f"{_name(dtype)} LOO mean, var, lpd, loo, grad off by " + ", ".join(f"{x:.2e}" for x in devs) + f" (bar {tol:g})")
    assert max(devs) <= tol, devs
    assert np.all(lvar > (math.exp(theta[0]) + vr) * (1 - 1e-3))
    # sample paths: the noise draw of row i is sqrt(s2 + v_i) eps
    F, S = 400, 3
    rng = E.RNG(31)
    om0, ph = gpr.draw_spectral(nu, F, d, rng)
    w, eps = rng.standard_normal((S, F)), rng.standard_normal((S, n))
    om0, ph, w, eps = (np.asarray(a, dtype=dtype) for a in (om0, ph, w, eps))
    noise, amp, ell = fk.device_params()
    th_dev = np.log(np.concatenate([[noise, amp], ell]))
    xq = np.random.default_rng(9).uniform(-0.1, 1.1, (40, d)).astype(dtype)
    for e in (eps, None):
        paths = fk.sample_paths(om0, ph, w, e)
        rp = PR.Paths(Xr, yr, amp, ell, nu, noise, om0, ph, w, eps=None, solve=lambda r: np.zeros_like(r))
        rp.K = rv_ref.kernel_matrix(Xr, vr, th_dev, nu)
        rp.resid = rv_ref.paths_residual(Xr, yr, vr, th_dev, om0, ph, w, e)
        rp.v = np.linalg.solve(rp.K, rp.resid.T)
        f, df = paths.evaluate(xq)
        rf, rdf = rp.evaluate(xq)
        d_f, d_g = PRU.dev(f, rf), PRU.dev(df, rdf)
        print(f"{_name(dtype)} paths ({'with' if e is not None else 'without'} eps): f off by {d_f:.2e}, df by {d_g:.2e} (bar {tol:g})")
        assert d_f <= tol and d_g <= tol
        if e is None:
            # without a noise draw v does not enter that term: the bytes of a zero draw
            zero = fk.sample_paths(om0, ph, w, np.zeros((S, n), dtype=dtype))
            fz, dfz = zero.evaluate(xq)
            assert f.tobytes() == fz.tobytes() and df.tobytes() == dfz.tobytes()
            zero.release()
        else:
            # and with one, v is really in it: the homoscedastic residual is elsewhere
            rh = rv_ref.paths_residual(Xr, yr, None, th_dev, om0, ph, w, e)
            assert np.max(np.abs(rh - rp.resid)) > 1e-2
        paths.release()
    fk.release()


# ---- 8. pool hygiene -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,d", [(100, 8), (200, 9)])
def test_evaluation_ignores_what_its_pool_blocks_held(n, d, dtype):
    """v's block holds n entries of a recycled block: nothing is read beyond n, nothing depends on what the block held."""
    from test_gpu_pool_hygiene import _check

    X, y, v, theta = _case(n, d)

    def subject():
        lml, grad, alpha, kinv, ldiag = _evaluate(X, y, v, theta, 2.5, dtype)
        return [np.array(lml), grad, alpha, kinv, ldiag]

    _check(subject, 1, 1)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_bad_variances_are_refused_and_nothing_is_written(dtype):
    lib = _lib.load()
    n, d = 100, 8
    X, y, v, theta = _case(n, d)
    X, y = _lib.as_c(X, dtype), _lib.as_c(y, dtype)
    sfx = "f64" if np.dtype(dtype) == np.float64 else "f32"
    ctx = gpr.default_context()._h
    lo, hi = FIT_LO(d), FIT_HI(d)
    prior = gpr.FittedKernel.extend(X, y, theta, row_variance=v)
    bads = [(-1e-300, 3), (float("nan"), 0), (float("inf"), n - 1)] + ([(1e300, 5)] if sfx == "f32" else [])  # 1e300 is inf as a float
    for bad, at in bads:
        rv = v.copy()
        rv[at] = bad
        sentinel = 0x5A5A
        h = C.c_void_p(sentinel)
        tb, best, inc = np.full(d + 2, 7.0), C.c_double(7.0), C.c_int(7)
        opt = _lib.FitOptions()
        calls = {
            "problem_create": lambda: getattr(lib, f"hbegp_problem_create_rv_{sfx}")(ctx, _lib.aptr(X), _lib.aptr(y), _lib.dptr(rv), n, d, 2.5, 1, C.byref(h)),
            "extend": lambda: getattr(lib, f"hbegp_extend_rv_{sfx}")(ctx, _lib.aptr(X), _lib.aptr(y), _lib.dptr(rv), n, d, 2.5, _lib.dptr(theta), None, None, C.byref(h)),
            "extend_from": lambda: getattr(lib, f"hbegp_extend_from_rv_{sfx}")(ctx, prior._h, _lib.aptr(X), _lib.aptr(y), _lib.dptr(rv), n, C.byref(h), C.byref(inc)),
            "fit": lambda: getattr(lib, f"hbegp_fit_rv_{sfx}")(ctx, _lib.aptr(X), _lib.aptr(y), _lib.dptr(rv), n, d, 2.5, _lib.dptr(theta), _lib.dptr(lo), _lib.dptr(hi), None, 0, C.byref(opt), _lib.dptr(tb), C.byref(best), C.byref(h)),
            "fit_loo": lambda: getattr(lib, f"hbegp_fit_loo_rv_{sfx}")(ctx, _lib.aptr(X), _lib.aptr(y), _lib.dptr(rv), n, d, 2.5, _lib.dptr(theta), _lib.dptr(lo), _lib.dptr(hi), None, 0, C.byref(opt), _lib.dptr(tb), C.byref(best), C.byref(h)),
        }
        for name, call in calls.items():
            assert call() == _lib.EINVAL, (name, bad)
            assert f"rv[{at}]" in _lib.last_error(), (name, _lib.last_error())
            assert h.value == sentinel and np.all(tb == 7.0) and best.value == 7.0 and inc.value == 7, name
    prior.release()


# ---- the estimator -------------------------------------------------------------------------------------------------------------
def test_estimator_with_replicate_variances():
    x, y, f = rv_ref.estimator_data()
    xu, ym, yv, cnt = E.aggregate_replicates(x, y)
    assert xu.shape == (30, 2) and cnt.tolist() == [4] * 30
    model = E.EstimatorGPR.new(2).estimate(xu, ym, None, E.RNG.new_with_seed(1), y_variance=yv)
    fk, yn = model.fitted, model.y_norm
    want_v = yn.project_variance_into_normalized(ym, yv)
    np.testing.assert_array_equal(fk.row_variance, want_v)
    truth = yn.project_into_normalized(f(xu))
    mean, var, _ = fk.predict(xu)
    inside = rv_ref.rows_within_two_sigma(mean, var, want_v, truth)
    # the reference itself meets the criterion at the fitted theta for this seed (and the device agrees with it)
    ev = rv_ref.evaluate(xu, fk.y_train, want_v, fk.theta, fk.nu, want_grad=False)
    rmean, rvar = rv_ref.predict(xu, xu, ev, fk.theta, fk.nu)
    inside_ref = rv_ref.rows_within_two_sigma(rmean, rvar, want_v, truth)
    print(f"rows within two posterior-plus-v standard deviations of the noiseless function: device {inside}, reference {inside_ref} of 30")
    assert rv_ref.cond(ev["K"]) <= rv_ref.COND_MAX, rv_ref.cond(ev["K"])
    assert PRU.dev(mean, rmean) <= PRU.TOL64 and PRU.dev(var, rvar) <= PRU.TOL64
    assert inside_ref >= 27 and inside >= 27
    # extend with variances keeps them; without, the model has none
    more = E.EstimatorGPR.new(2).extend(xu, ym, model, y_variance=yv)
    np.testing.assert_array_equal(more.fitted.row_variance, want_v)
    assert E.EstimatorGPR.new(2).extend(xu, ym, model).fitted.row_variance is None


# ---- the C++ wrapper -----------------------------------------------------------------------------------------------------------
def test_cpp_wrapper_row_variance_arguments(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, lib_dir = str(tmp_path / "test_rv"), os.path.join(root, "hbetune_rs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "test_rv.cpp"),
                           "-L", lib_dir, "-lhbegp", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0 threw=2" in out.stdout
