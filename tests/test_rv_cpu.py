"""CPU: the reference of the row-variance model (tests/rv_ref.py) against scikit-learn and against leave-one-out by deletion, the
estimator's replicate aggregation and variance projection, and the `_rv` entry points' signatures and refusals that need no device.

The GPU file (tests/test_gpu_rv.py) compares the engine with rv_ref at these very parameters; cond(K) <= 1e4 is asserted here for
every case it uses, so that LAPACK's own digits (~cond(K) eps = 2e-12) are never the limit of a 1e-8 comparison."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import rv_ref
from hbetune_rs_amd import _lib
from hbetune_rs_amd.estimator import YNormalize, aggregate_replicates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sklearn_model(X, y, v, theta, nu):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel

    p = np.exp(theta)
    base = RBF(length_scale=p[2:]) if math.isinf(nu) else Matern(length_scale=p[2:], nu=nu)
    kernel = ConstantKernel(p[1]) * base + WhiteKernel(p[0])
    return GaussianProcessRegressor(kernel=kernel, alpha=v, optimizer=None).fit(X, y)


@pytest.mark.parametrize("n,d,nu", rv_ref.CPU_SHAPES)
def test_reference_matches_sklearn_with_alpha_array(n, d, nu):
    X, y, v, theta = rv_ref.case(n, d)
    assert np.all(v[::7] == 0.0) and v.max() <= 0.2 and v.min() >= 0.0
    ev = rv_ref.evaluate(X, y, v, theta, nu)
    assert rv_ref.cond(ev["K"]) <= rv_ref.COND_MAX
    gp = _sklearn_model(X, y, v, theta, nu)
    # sklearn's theta: [ln c, ln ell_k, ln s2]; ours: [ln s2, ln c, ln ell_k]
    sk_theta = np.concatenate([theta[1:], theta[:1]])
    lml, grad = gp.log_marginal_likelihood(sk_theta, eval_gradient=True)
    grad = np.concatenate([grad[-1:], grad[:-1]])
    assert abs(lml - ev["lml"]) <= 1e-12 * max(1.0, abs(lml))
    assert np.max(np.abs(grad - ev["grad"])) <= 1e-12 * max(1.0, np.max(np.abs(grad)))
    Xs = np.random.default_rng(5).random((17, d))
    mean, std = gp.predict(Xs, return_std=True)
    rmean, rvar = rv_ref.predict(Xs, X, ev, theta, nu)
    assert np.max(np.abs(mean - rmean)) <= 1e-12 * max(1.0, np.max(np.abs(mean)))
    # sklearn's variance is that of a new observation under the White kernel: minus s2 it is the latent function's (ours, which
    # carries predict.rs's 1e-5 instead)
    assert np.max(np.abs((std * std - math.exp(theta[0])) - (rvar - 1e-5))) <= 1e-12 * max(1.0, math.exp(theta[1]))


def test_gpu_cases_are_well_conditioned():
    """Every (n, d) of tests/test_gpu_rv.py at every nu it uses: cond(K) <= 1e4."""
    worst = 0.0
    for n, d in rv_ref.GPU_SHAPES + rv_ref.GPU_EXTRA_SHAPES:
        X, y, v, theta = rv_ref.case(n, d)
        for nu in rv_ref.NUS:
            worst = max(worst, rv_ref.cond(rv_ref.kernel_matrix(X, v, theta, nu)))
    assert worst <= rv_ref.COND_MAX


def test_closed_form_loo_equals_deletion():
    n, d, nu = 40, 3, 2.5
    X, y, v, theta = rv_ref.case(n, d)
    cf = rv_ref.loo(X, y, v, theta, nu)
    mean, var = rv_ref.loo_by_deletion(X, y, v, theta, nu)
    assert np.max(np.abs(cf["mean"] - mean)) <= 1e-10
    assert np.max(np.abs(cf["var"] - var)) <= 1e-10
    # the variance is the noisy observation's: above the row's own noise s2 + v_i
    assert np.all(var > math.exp(theta[0]) + v)
    # and the closed-form gradient is the derivative of the closed-form loo (v held fixed)
    h = 1e-6
    for j in range(len(theta)):
        e = np.zeros(len(theta))
        e[j] = h
        fd = (rv_ref.loo(X, y, v, theta + e, nu, want_grad=False)["loo"] - rv_ref.loo(X, y, v, theta - e, nu, want_grad=False)["loo"]) / (2 * h)
        assert abs(fd - cf["grad"][j]) <= 1e-6 * max(1.0, abs(fd))


def test_lml_gradient_is_the_derivative_with_v_fixed():
    X, y, v, theta = rv_ref.case(60, 3)
    ev = rv_ref.evaluate(X, y, v, theta, 1.5)
    h = 1e-6
    for j in range(len(theta)):
        e = np.zeros(len(theta))
        e[j] = h
        fd = (rv_ref.evaluate(X, y, v, theta + e, 1.5, False)["lml"] - rv_ref.evaluate(X, y, v, theta - e, 1.5, False)["lml"]) / (2 * h)
        assert abs(fd - ev["grad"][j]) <= 1e-6 * max(1.0, abs(fd))


def test_aggregate_replicates_groups_of_1_2_and_5():
    rng = np.random.default_rng(3)
    xa, xb, xc = np.array([0.1, 0.2]), np.array([0.5, 0.5]), np.array([0.9, 0.1])
    ya, yb, yc = rng.normal(1.0, 0.3, 5), rng.normal(2.0, 0.3, 2), np.array([3.25])
    # interleaved, first appearances in the order b, c, a
    rows = [(xb, yb[0]), (xc, yc[0]), (xa, ya[0]), (xa, ya[1]), (xb, yb[1]), (xa, ya[2]), (xa, ya[3]), (xa, ya[4])]
    x = np.array([r[0] for r in rows])
    y = np.array([r[1] for r in rows])
    xu, mean, var, count = aggregate_replicates(x, y)
    assert xu.tolist() == [xb.tolist(), xc.tolist(), xa.tolist()] and count.tolist() == [2, 1, 5]
    np.testing.assert_allclose(mean, [yb.mean(), yc[0], ya.mean()], rtol=0, atol=1e-15)
    pooled = (((ya - ya.mean()) ** 2).sum() + ((yb - yb.mean()) ** 2).sum()) / (4 + 1)
    np.testing.assert_allclose(var, [yb.var(ddof=1) / 2, pooled, ya.var(ddof=1) / 5], rtol=1e-14, atol=0)


def test_aggregate_replicates_without_a_replicated_row():
    x = np.array([[0.0], [1.0], [2.0]])
    y = np.array([5.0, 6.0, 7.0], dtype=np.float32)
    xu, mean, var, count = aggregate_replicates(x, y)
    assert xu.tolist() == x.tolist() and mean.tolist() == y.tolist() and mean.dtype == np.float32
    assert var.tolist() == [0.0, 0.0, 0.0] and count.tolist() == [1, 1, 1]


def test_variance_projection_linear_is_exact_and_logarithmic_is_first_order():
    rng = np.random.default_rng(11)
    y = rng.uniform(2.0, 9.0, 12)
    yv = rng.uniform(0.01, 0.2, 12)
    _, lin = YNormalize.new_project_into_normalized(y, "linear")
    assert np.array_equal(lin.project_variance_into_normalized(y, yv), yv / float(lin.amplitude) ** 2)
    # exact: the projection is affine, so the variance of projected draws scales by its slope squared
    a, b = lin.project_into_normalized(np.array([0.0, 1.0]))
    np.testing.assert_allclose(lin.project_variance_into_normalized(y, yv), yv * (b - a) ** 2, rtol=1e-14)
    _, lg = YNormalize.new_project_into_normalized(y, "logarithmic")
    h = 1e-6
    slope = (lg.project_into_normalized(y + h) - lg.project_into_normalized(y - h)) / (2 * h)
    np.testing.assert_allclose(lg.project_variance_into_normalized(y, yv), slope ** 2 * yv, rtol=1e-8)


def test_reference_meets_the_estimator_criterion_for_the_fixed_seed():
    """The GPU file's estimator test asks that the posterior mean at the training rows lies within two posterior-plus-v standard
    deviations of the noiseless function for at least 27 of 30 rows.  Here the reference, its hyper-parameters fitted by scipy's
    L-BFGS-B from the estimator's own start and box, meets that for the seed the GPU test uses."""
    from scipy.optimize import minimize

    from hbetune_rs_amd.estimator import EstimatorGPR

    x, y, f = rv_ref.estimator_data()
    xu, ym, yv, cnt = aggregate_replicates(x, y)
    assert xu.shape == (30, 2) and cnt.tolist() == [4] * 30 and np.all(yv > 0)
    yt, yn = YNormalize.new_project_into_normalized(ym, "linear")
    v = yn.project_variance_into_normalized(ym, yv)
    theta0, lo, hi = EstimatorGPR.new(2)._theta_and_bounds(None, yt)

    def objective(th):
        try:
            ev = rv_ref.evaluate(xu, yt, v, th, 2.5)
        except np.linalg.LinAlgError:
            return 1e10, np.zeros(len(th))
        return -ev["lml"], -ev["grad"]

    rng = np.random.default_rng(0)
    starts = [theta0] + [np.log(lo) + (np.log(hi) - np.log(lo)) * rng.random(len(lo)) for _ in range(2)]
    fits = [minimize(objective, s0, jac=True, method="L-BFGS-B", bounds=list(zip(np.log(lo), np.log(hi)))) for s0 in starts]
    theta = min(fits, key=lambda r: r.fun).x
    ev = rv_ref.evaluate(xu, yt, v, theta, 2.5, want_grad=False)
    mean, var = rv_ref.predict(xu, xu, ev, theta, 2.5)
    assert rv_ref.rows_within_two_sigma(mean, var, v, yn.project_into_normalized(f(xu))) >= 27


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------
RV_SYMBOLS = ["hbegp_problem_create_rv", "hbegp_fit_rv", "hbegp_fit_loo_rv", "hbegp_extend_rv", "hbegp_extend_from_rv"]


def test_rv_symbols_are_declared_exported_and_mirror_their_plain_counterparts():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hbegp.h")).read()
    for base in RV_SYMBOLS:
        for sfx in ("f64", "f32"):
            name, plain = f"{base}_{sfx}", f"{base[:-3]}_{sfx}"
            assert re.search(rf"\bint {name}\s*\(", header) and hasattr(lib, name)
            res, args = _lib.SIGNATURES[name]
            pres, pargs = _lib.SIGNATURES[plain]
            # the plain signature with `const double* rv` behind y -- for both element types
            k = 4 if base == "hbegp_extend_from_rv" else 3
            assert res is pres and list(args) == list(pargs[:k]) + [C.POINTER(C.c_double)] + list(pargs[k:])
    assert _lib.SIGNATURES["hbegp_model_row_variance"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_double)])
    assert hasattr(lib, "hbegp_model_row_variance")
    assert lib.hbegp_version() == 200 and C.sizeof(_lib.FitOptions) == 8 + 4 * 4 + 7 * 8


def test_rv_refusals_without_a_device():
    """The order of the plain entry points (tests/test_abi_cpu.py): the options' size, then the arguments with the context first --
    a NULL context is reported before a bad rv is looked at."""
    lib = _lib.load()
    x = np.zeros(4)
    bad_rv = np.array([0.0, -1.0, 0.0, 0.0])
    opt = _lib.FitOptions()
    out = C.c_void_p(0x1234)
    rc = lib.hbegp_fit_rv_f64(None, _lib.dptr(x), _lib.dptr(x), _lib.dptr(bad_rv), 4, 1, 2.5, _lib.dptr(x), _lib.dptr(x), _lib.dptr(x), None,
                              0, C.byref(opt), None, None, C.byref(out))
    assert rc == _lib.EINVAL and "ctx is NULL" in _lib.last_error() and out.value == 0x1234
    bad = _lib.FitOptions()
    bad.struct_size = 0
    rc = lib.hbegp_fit_loo_rv_f32(None, _lib.fptr(x.astype(np.float32)), _lib.fptr(x.astype(np.float32)), _lib.dptr(bad_rv), 4, 1, 2.5,
                                  _lib.dptr(x), _lib.dptr(x), _lib.dptr(x), None, 0, C.byref(bad), None, None, None)
    assert rc == _lib.EINVAL and "struct_size" in _lib.last_error()
    rc = lib.hbegp_extend_rv_f64(None, _lib.dptr(x), _lib.dptr(x), _lib.dptr(bad_rv), 4, 1, 2.5, _lib.dptr(x), None, None, C.byref(out))
    assert rc == _lib.EINVAL and "ctx is NULL" in _lib.last_error() and out.value == 0x1234
    rc = lib.hbegp_problem_create_rv_f64(None, _lib.dptr(x), _lib.dptr(x), _lib.dptr(bad_rv), 4, 1, 2.5, 1, C.byref(out))
    assert rc == _lib.EINVAL and "ctx is NULL" in _lib.last_error() and out.value == 0x1234
    rc = lib.hbegp_extend_from_rv_f64(None, None, _lib.dptr(x), _lib.dptr(x), _lib.dptr(bad_rv), 4, C.byref(out), None)
    assert rc == _lib.EINVAL and "NULL" in _lib.last_error() and out.value == 0x1234
    assert lib.hbegp_model_row_variance(None, None) == _lib.EINVAL and "NULL model" in _lib.last_error()
