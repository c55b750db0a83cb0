"""GPU: leave-one-out cross-validation -- hbegp_model_loo_*, hbegp_problem_eval_loo, hbegp_fit_loo_* and the estimator's opt-in
objective -- against the NumPy restatement (tests/loo_ref.py) and, independently of it, against real row deletion on the device.

Bars: parity_rules.TOL64 = 1e-8 and TOL32 = 1e-4, relative to max(1, scale of the reference); the variance relative to c + s2.
Thetas as in tests/test_gpu_paths.py: noise = 1e-2 amplitude (f64) and = amplitude (f32), so cond(K) <= n c / s2 + 1 <= 4.1e5."""
import ctypes as C
import functools
import math
import threading

import numpy as np
import pytest

import loo_ref as LR
import parity_rules as PRU
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

NUS = [0.5, 1.5, 2.5, math.inf]
D = 4
AMP = 1.3


def _tol(dtype):
    return PRU.TOL64 if np.dtype(dtype) == np.float64 else PRU.TOL32


def _data(n, dtype, seed=1, d=D):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    X, y = X.astype(dtype), y.astype(dtype)
    ratio = 1e-2 if np.dtype(dtype) == np.float64 else 1.0
    theta = np.log(np.concatenate([[ratio * AMP, AMP], np.linspace(0.3, 0.9, d)]))
    return X, y, theta


@functools.lru_cache(maxsize=8)
def _ref_at_test_theta(n, nu, dtype_name):
    X, y, theta = _data(n, np.dtype(dtype_name), seed=n)
    return LR.loo_at_theta(X, y, theta, nu)


def _check(what, got, ref, tol, c_plus_s2):
    """got = (mean, var, lpd, loo, grad) of the device."""
    mean, var, lpd, loo, grad = got
    devs = dict(mean=PRU.dev(mean, ref["mean"]), var=PRU.dev(var, ref["var"], scale=1.0) / c_plus_s2, lpd=PRU.dev(lpd, ref["lpd"]),
                loo=PRU.dev(loo, ref["loo"]), grad=PRU.dev(grad, ref["grad"]))
    print(f"{what}: " + ", ".join(f"{k} off by {v:.2e}" for k, v in devs.items()) +
          f" (loo {ref['loo']:.6g}, max |grad| {np.abs(ref['grad']).max():.3g}, two forms of m differ by "
          f"{np.abs(ref['m'] / ref['m_kinv'] - 1).max():.1e}; bar {tol:g})")
    for k, v in devs.items():
        assert v <= tol, (what, k, v)


def _kinds(n):
    return ["extend", "small_fit"] if n == 100 else ["extend"] if n <= 128 else ["extend", "extend_with"]


CASES = [(n, kind) for n in (1, 100, 129, 200, 4096) for kind in _kinds(n)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,kind", CASES)
@pytest.mark.parametrize("nu", NUS)
def test_model_loo_matches_restatement(nu, n, kind, dtype):
    """Every kind of model: extend (n <= 128: the single launch in the LDS; 129, 200: the launch path; 4096: the task queue),
    the incremental extend_with from a prior on a prefix of the rows, and a device-driven small fit (its captured factor)."""
    X, y, theta = _data(n, dtype, seed=n)
    if kind == "extend":
        fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    elif kind == "extend_with":
        n0 = 128 if n == 129 else n - 70
        prior = gpr.FittedKernel.extend(X[:n0], y[:n0], theta, nu=nu)
        fk = prior.extend_with(X, y)
        assert fk.incremental
        prior.release()
    else:
        lo = np.concatenate([[np.exp(theta[0]) / 4, AMP / 4], np.full(D, 0.1)])
        hi = np.concatenate([[np.exp(theta[0]) * 4, AMP * 4], np.full(D, 3.0)])
        fk = gpr.FittedKernel.new(X, y, theta, lo, hi, None, nu=nu, maxeval=12)
    noise, amp, ell = fk.device_params()
    if kind == "small_fit":
        ref = LR.loo(X, y, noise, amp, ell, nu)
    else:
        ref = _ref_at_test_theta(n, nu, np.dtype(dtype).name)
    got = fk.loo(want_grad=True)
    assert got[0].dtype == np.dtype(dtype) and got[4].dtype == np.float64
    _check(f"nu={nu} n={n} {kind} {np.dtype(dtype).name}", got, ref, _tol(dtype), amp + noise)
    # without the gradient: the same diagnostics; the same call: the same bits
    m2, v2, l2, loo2 = fk.loo()
    assert np.array_equal(m2, got[0]) and np.array_equal(v2, got[1]) and np.array_equal(l2, got[2]) and loo2 == got[3]
    again = fk.loo(want_grad=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nu", [0.5, 2.5, math.inf])
def test_model_loo_equals_real_deletion_on_the_device(nu, dtype):
    """No restatement: for eight rows i, extend on the data without row i at the same theta and predict at x_i."""
    n = 300
    X, y, theta = _data(n, dtype, seed=5)
    fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    mean, var, _, _ = fk.loo()
    s2, c = math.exp(theta[0]), math.exp(theta[1])
    tol = _tol(dtype)
    for i in (0, 1, 63, 127, 128, 200, 298, 299):
        keep = np.arange(n) != i
        fd = gpr.FittedKernel.extend(X[keep], y[keep], theta, nu=nu)
        pm, pv, _ = fd.predict(X[i:i + 1])
        fd.release()
        d_m = abs(float(pm[0]) - float(mean[i])) / max(1.0, abs(float(pm[0])))
        d_v = abs(float(pv[0]) + s2 - 1e-5 - float(var[i])) / (c + s2)
        print(f"nu={nu} {np.dtype(dtype).name} row {i}: mean off by {d_m:.2e}, var by {d_v:.2e} (bar {tol:g})")
        assert d_m <= tol and d_v <= tol, (i, d_m, d_v)
    fk.release()


def test_model_loo_refuses_the_other_element_type_and_all_null():
    X, y, theta = _data(50, np.float64)
    fk = gpr.FittedKernel.extend(X, y, theta)
    lib = _lib.load()
    loo = C.c_double()
    assert lib.hbegp_model_loo_f32(fk._h, None, None, None, C.byref(loo), None) == _lib.EINVAL
    assert "model holds f64 data" in _lib.last_error()
    assert lib.hbegp_model_loo_f64(fk._h, None, None, None, None, None) == _lib.EINVAL
    assert "every output is NULL" in _lib.last_error()
    assert lib.hbegp_model_loo_f64(fk._h, None, None, None, C.byref(loo), None) == _lib.OK  # loo alone
    assert loo.value == fk.loo()[3]
    fk.release()


# ---------------------------------------------------------------------------------------------------------------- the problem
BOX_LO = np.concatenate([[1e-4, 0.1], np.full(D, 0.05)])
BOX_HI = np.concatenate([[1e2, 10.0], np.full(D, 0.8)])


def _thetas(theta):
    clamped = theta.copy()
    clamped[2 + D - 1] = math.log(2.0)  # ell_D = 2 > its bound 0.8: evaluated at 0.8
    return [theta, theta + np.array([0.7, -0.3] + [0.2] * D), clamped]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 100, 300, 900])  # single launch (1, 100), launch path, task queue
@pytest.mark.parametrize("nu", [1.5, 2.5])
def test_problem_eval_loo_matches_restatement_and_leaves_the_slot_alone(nu, n, dtype):
    X, y, theta = _data(n, dtype, seed=n + 1)
    tol = _tol(dtype)
    prob = gpr.Problem(X, y, nu=nu)
    plain = gpr.Problem(X, y, nu=nu)
    for k, th in enumerate(_thetas(theta)):
        loo, grad = prob.loo_with_gradient(th, BOX_LO, BOX_HI)
        ref = LR.loo_at_theta(X, y, th, nu, BOX_LO, BOX_HI)
        d_l, d_g = PRU.dev(loo, ref["loo"]), PRU.dev(grad, ref["grad"])
        print(f"nu={nu} n={n} {np.dtype(dtype).name} theta {k}: loo off by {d_l:.2e}, grad by {d_g:.2e} (bar {tol:g})")
        assert d_l <= tol and d_g <= tol
        # the slot afterwards: what hbegp_problem_eval at that theta leaves behind, bit for bit
        want_lml, _ = plain.lml_with_gradient(th, BOX_LO, BOX_HI, want_grad=False)
        for a, b in zip(prob.results(), plain.results()):
            assert np.array_equal(a, b)
        # the same call gives the same bits; without the gradient the same value
        loo2, grad2 = prob.loo_with_gradient(th, BOX_LO, BOX_HI)
        assert loo2 == loo and np.array_equal(grad2, grad)
        assert prob.loo_with_gradient(th, BOX_LO, BOX_HI, want_grad=False)[0] == loo
        # a following evaluation is undisturbed
        lml_a, g_a = prob.lml_with_gradient(th, BOX_LO, BOX_HI)
        lml_b, g_b = plain.lml_with_gradient(th, BOX_LO, BOX_HI)
        assert lml_a == lml_b == want_lml and np.array_equal(g_a, g_b)
    prob.close()
    plain.close()


def test_problem_eval_loo_agrees_with_model_loo():
    X, y, theta = _data(300, np.float64, seed=3)
    prob = gpr.Problem(X, y)
    loo, grad = prob.loo_with_gradient(theta)
    prob.close()
    fk = gpr.FittedKernel.extend(X, y, theta)
    _, _, _, loo_m, grad_m = fk.loo(want_grad=True)
    fk.release()
    assert PRU.dev(loo, loo_m) <= PRU.TOL64 and PRU.dev(grad, grad_m) <= PRU.TOL64


def test_problem_eval_loo_not_positive_definite():
    # where hbegp_problem_eval fails (tests/test_gpu_parity.py): duplicate rows with vanishing noise on the single-launch path,
    # a NaN feature on the launch path
    lib = _lib.load()
    X4 = np.array([[0.1, 0.2], [0.1, 0.2], [0.5, 0.5], [0.9, 0.1]])
    y4 = np.array([1.0, 2.0, 3.0, 0.5])
    Xn, yn, theta_n = _data(300, np.float64, seed=2)
    Xn[17, 1] = np.nan
    for X, y, bad, good in ((X4, y4, np.array([math.log(1e-300), 0.0, 0.0, 0.0]), np.array([math.log(0.1), 0.0, 0.0, 0.0])),
                            (Xn, yn, theta_n, None)):
        prob = gpr.Problem(X, y)
        assert prob.lml_with_gradient(bad) is None
        loo, grad = C.c_double(1.0), np.ones(X.shape[1] + 2)
        rc = lib.hbegp_problem_eval_loo(prob._h, 0, 0, _lib.dptr(bad), None, None, C.byref(loo), _lib.dptr(grad))
        assert rc == _lib.NOT_PD and loo.value == -math.inf and (grad == 0).all()
        if good is not None:  # the slot is usable afterwards
            got = prob.loo_with_gradient(good)
            ref = LR.loo_at_theta(X, y, good, 2.5)
            assert PRU.dev(got[0], ref["loo"]) <= PRU.TOL64 and PRU.dev(got[1], ref["grad"]) <= PRU.TOL64
        prob.close()


def test_problem_eval_loo_same_bits_from_threads_on_different_slots():
    X, y, theta = _data(700, np.float64, seed=4)
    prob = gpr.Problem(X, y, n_slots=3)
    want = prob.loo_with_gradient(theta)
    out, errs = [None] * 3, []

    def work(slot):
        try:
            for _ in range(3):
                out[slot] = prob.loo_with_gradient(theta, slot=slot)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(s,)) for s in range(3)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for loo, grad in out:
        assert loo == want[0] and np.array_equal(grad, want[1])
    prob.close()


# ---------------------------------------------------------------------------------------------------------------- the fit
def _fit_box(dtype, d=D):
    """f64: the noise bound stays >= 1e-3 x the amplitude's upper bound, so cond(K) <= 1e3 n + 1 at every theta the optimiser can
    visit.  f32: the noise bound stays >= the amplitude's upper bound, cond(K) <= n + 1 -- the regime of every f32 case of this
    file (noise = amplitude) and of the f32 posterior tests: eps_f32 cond(K) has to stay below the 1e-4 bar, and at the f64 box's
    cond(K) <= 3e5 it is 2e-2 (measured there at n = 300: loo off by 1.8e-4, its gradient by 1.3e-2 of its scale)."""
    if np.dtype(dtype) == np.float64:
        lo = np.concatenate([[4e-3, 0.25], np.full(d, 0.1)])
        hi = np.concatenate([[4.0, 4.0], np.full(d, 3.0)])
    else:
        lo = np.concatenate([[4.0, 0.25], np.full(d, 0.1)])
        hi = np.concatenate([[400.0, 4.0], np.full(d, 3.0)])
    return lo, hi


@pytest.mark.parametrize("dtype,n", [(np.float64, 100), (np.float64, 300), (np.float64, 800), (np.float32, 300)])
def test_fit_loo(dtype, n):
    X, y, _ = _data(n, dtype, seed=n + 7)
    lo, hi = _fit_box(dtype)
    tol = _tol(dtype)
    theta0 = np.log(np.sqrt(lo * hi))
    # run 0 starts at an lml-fitted theta
    pre = gpr.FittedKernel.new(X, y, theta0, lo, hi, None, maxeval=25)
    start = pre.theta.copy()
    loo_start = pre.loo()[3]
    pre.release()
    starts = np.log(lo) + (np.log(hi) - np.log(lo)) * np.random.default_rng(n).uniform(0, 1, (2, D + 2))
    fk = gpr.FittedKernel.new_by_loo(X, y, start, lo, hi, starts, maxeval=20, trace=True)
    tr = fk.trace
    assert fk.n_evals == len(tr["lml"]) and set(tr["run"]) == {0, 1, 2}
    # every traced evaluation through the restatement
    worst_l = worst_g = 0.0
    for th, loo, grad in zip(tr["theta"], tr["lml"], tr["grad"]):
        ref = LR.loo_at_theta(X, y, th, 2.5, lo, hi)
        worst_l, worst_g = max(worst_l, PRU.dev(loo, ref["loo"])), max(worst_g, PRU.dev(grad, ref["grad"]))
    print(f"fit_loo n={n} {np.dtype(dtype).name}: {len(tr['lml'])} evaluations, loo off by {worst_l:.2e}, grad by {worst_g:.2e} (bar {tol:g}); "
          f"loo {loo_start:.6g} at the lml optimum -> {fk.loo_best:.6g}")
    assert worst_l <= tol and worst_g <= tol
    # the capture rule: the arg-max of the trace (ties to the lowest (run, eval): the trace is in that order), clamped
    i = int(np.argmax(tr["lml"]))
    assert fk.loo_best == tr["lml"][i]
    # (fit.rs:155-164 with the C library's exp / log, which math's are; NumPy's vectorised ones may differ in the last bit)
    want_theta = np.array([math.log(min(max(math.exp(t), a), b)) for t, a, b in zip(tr["theta"][i], lo, hi)])
    assert np.array_equal(fk.theta_best, want_theta) and np.array_equal(fk.theta, want_theta)
    # exact, by the capture rule: evaluation 0 of run 0 IS the lml-fitted theta
    assert np.array_equal(tr["theta"][0], start) and fk.loo_best >= tr["lml"][0]
    assert PRU.dev(tr["lml"][0], loo_start) <= tol
    # the model is extend at theta_best, bit for bit
    ext = gpr.FittedKernel.extend(X, y, fk.theta_best)
    for a, b in zip(fk.arrays(), ext.arrays()):
        assert np.array_equal(a, b)
    xs = np.random.default_rng(1).uniform(0, 1, (20, D)).astype(dtype)
    for a, b in zip(fk.predict(xs)[:2], ext.predict(xs)[:2]):
        assert np.array_equal(a, b)
    assert fk.lml == ext.lml
    assert PRU.dev(fk.loo()[3], fk.loo_best) <= tol
    # the same call twice: the same bits
    fk2 = gpr.FittedKernel.new_by_loo(X, y, start, lo, hi, starts, maxeval=20, trace=True)
    assert np.array_equal(fk2.theta_best, fk.theta_best) and fk2.loo_best == fk.loo_best
    assert np.array_equal(fk2.trace["lml"], tr["lml"]) and np.array_equal(fk2.trace["grad"], tr["grad"])
    for a, b in zip(fk.arrays(), fk2.arrays()):
        assert np.array_equal(a, b)
    for f in (fk, fk2, ext):
        f.release()


def test_fit_loo_honours_maxeval_and_fixed_work():
    X, y, _ = _data(200, np.float64, seed=9)
    lo, hi = _fit_box(np.float64)
    theta0 = np.log(np.sqrt(lo * hi))
    fk = gpr.FittedKernel.new_by_loo(X, y, theta0, lo, hi, None, maxeval=7, fixed_work=True)
    assert fk.n_evals == 7
    fk.release()
    fk = gpr.FittedKernel.new_by_loo(X, y, theta0, lo, hi, None, maxeval=3)
    assert 1 <= fk.n_evals <= 3
    fk.release()


# ---------------------------------------------------------------------------------------------------------------- the estimator
def test_estimator_objective_and_loo_a():
    n, d = 150, 3
    rng = np.random.default_rng(11)
    x = rng.uniform(0, 1, (n, d))
    y = 40.0 + 25.0 * ((x - 0.4) ** 2).sum(axis=1) + rng.standard_normal(n)
    est = lambda: E.EstimatorGPR.new(d).noise_bounds(1e-3, 1e1).length_scale_bounds([(0.05, 5.0)] * d)  # noqa: E731
    with pytest.raises(ValueError):
        est().objective("aic")
    # the default path returns the bits it returns without the builder
    m_default = est().estimate(x, y, None, E.RNG(3))
    m_lml = est().objective("lml").estimate(x, y, None, E.RNG(3))
    assert np.array_equal(m_default.fitted.theta, m_lml.fitted.theta)
    for a, b in zip(m_default.fitted.arrays(), m_lml.fitted.arrays()):
        assert np.array_equal(a, b)
    assert not hasattr(m_default.fitted, "loo_best")
    m_loo = est().objective("loo").estimate(x, y, None, E.RNG(3))
    assert hasattr(m_loo.fitted, "loo_best")
    loo_of = lambda m: m.fitted.loo()[3]  # noqa: E731
    print(f"estimator: loo {loo_of(m_lml):.6g} (lml objective) vs {loo_of(m_loo):.6g} (loo objective)")
    assert PRU.dev(loo_of(m_loo), m_loo.fitted.loo_best) <= PRU.TOL64
    # loo_a in original units against the restatement projected through YNormalize
    for m in (m_lml, m_loo):
        y_train, y_norm = E.YNormalize.new_project_into_normalized(y, "linear", None)
        noise, amp, ell = m.fitted.device_params()
        ref = LR.loo(x, y_train, noise, amp, ell, 2.5, want_grad=False)
        mean, std, resid = m.loo_a()
        want_mean = y_norm.project_mean_from_normalized(ref["mean"], ref["var"])
        want_std = y_norm.project_std_from_normalized(ref["mean"], ref["var"])
        want_resid = (y_train - ref["mean"]) / np.sqrt(ref["var"])
        assert PRU.dev(mean, want_mean) <= PRU.TOL64 and PRU.dev(std, want_std) <= PRU.TOL64
        assert PRU.dev(resid, want_resid) <= PRU.TOL64
        assert np.abs(resid).max() < 6.0  # a sane model of its own data
    for m in (m_default, m_lml, m_loo):
        m.fitted.release()
