"""CPU checks of the posterior-gradient feature (hbegp_predict_grad_*, hbegp_maximize_ei_*): the symbols and their
signatures, argument checks that refuse before any device call, and the formulas themselves -- the NumPy restatement of
d mean / dx* and d var / dx* (tests/predict_grad_ref.py, both forms of the variance gradient) against central differences of the oracle's predict for every
Matern order, and the EI-gradient algebra against central differences of estimator.expected_improvement."""
import ctypes as C
import math

import numpy as np
import pytest

import predict_grad_ref as PG
from hbetune_rs_amd import _lib
from hbetune_rs_amd import estimator as E
from oracle import gpr_oracle as O

NEW = ("hbegp_predict_grad_f64", "hbegp_predict_grad_f32", "hbegp_maximize_ei_f64", "hbegp_maximize_ei_f32")


def test_gradient_symbols_are_exported_with_signatures():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def _einval(rc, what):
    assert rc == _lib.EINVAL
    assert what in _lib.last_error(), _lib.last_error()


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    x = np.zeros(4)
    out = np.zeros(4)
    d = _lib.dptr
    xf, outf = np.zeros(4, np.float32), np.zeros(4, np.float32)
    f = _lib.fptr
    _einval(lib.hbegp_predict_grad_f64(None, d(x), 1, d(out), d(out), d(out), d(out), None), "NULL model")
    _einval(lib.hbegp_predict_grad_f32(None, f(xf), 1, f(outf), f(outf), f(outf), f(outf), None), "NULL model")
    _einval(lib.hbegp_predict_grad_f64(None, d(x), -1, d(out), d(out), d(out), d(out), None), "m must be >= 0")
    _einval(lib.hbegp_predict_grad_f32(None, f(xf), -3, f(outf), None, f(outf), None, None), "m must be >= 0")
    lo, hi = np.zeros(2), np.ones(2)
    _einval(lib.hbegp_maximize_ei_f64(None, d(x), 0, d(lo), d(hi), 0.0, 10, d(out), d(out), None), "S must be >= 1")
    _einval(lib.hbegp_maximize_ei_f32(None, f(xf), 0, d(lo), d(hi), 0.0, 10, f(outf), d(out), None), "S must be >= 1")
    _einval(lib.hbegp_maximize_ei_f64(None, d(x), 2, d(lo), d(hi), 0.0, 10, d(out), d(out), None), "NULL model")
    # lo > hi: the box is checked against the model's d, so without a model the call stops at the model (the GPU test
    # tests/test_gpu_predict_grad.py::test_wrong_arguments checks the lo > hi message on a real model)
    _einval(lib.hbegp_maximize_ei_f64(None, d(x), 2, d(hi), d(lo), 0.0, 10, d(out), d(out), None), "NULL model")


def _problem(nu, n=30, d=3, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    amp, noise = 1.7, 1e-2
    ell = np.array([0.3, 0.5, 0.8][:d])
    res = O.lml_with_gradient(X, y, noise, amp, ell, nu)
    # query points away from the training points (nu = 1/2 has a kink at r = 0)
    Xs = rng.uniform(0, 1, (40, d))
    dist = np.sqrt((((Xs / ell)[:, None, :] - (X / ell)[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
    Xs = Xs[dist > 0.05][:12]
    return X, res["alpha"], res["k_inv"], amp, ell, Xs, noise


@pytest.mark.parametrize("nu", [0.5, 1.5, 2.5, math.inf])
def test_restatement_matches_central_differences_of_the_oracle(nu):
    X, alpha, kinv, amp, ell, Xs, noise = _problem(nu)
    m, d = Xs.shape
    dmean = PG.dmean_ref(Xs, X, alpha, amp, ell, nu)
    dvar = PG.dvar_ref(Xs, X, amp, ell, nu, noise)
    assert PG.row_dev(PG.dvar_ref_kinv(Xs, X, kinv, amp, ell, nu), dvar) < 1e-9  # the two forms agree at this cond(K)
    fd_mean, fd_var = np.zeros((m, d)), np.zeros((m, d))
    for k in range(d):
        h = 1e-5 * ell[k]
        xp, xm = Xs.copy(), Xs.copy()
        xp[:, k] += h
        xm[:, k] -= h
        mp, vp, _ = O.predict(xp, X, alpha, kinv, amp, ell, nu)
        mm, vm, _ = O.predict(xm, X, alpha, kinv, amp, ell, nu)
        fd_mean[:, k] = (mp - mm) / (2 * h)
        fd_var[:, k] = (vp - vm) / (2 * h)
    _, var, _ = O.predict(Xs, X, alpha, kinv, amp, ell, nu)
    assert (var > 1e-6).all()  # no clamped variance at these points
    assert PG.row_dev(dmean, fd_mean) < 1e-6, PG.row_dev(dmean, fd_mean)
    assert PG.row_dev(dvar, fd_var) < 1e-6, PG.row_dev(dvar, fd_var)


@pytest.mark.parametrize("nu", [0.5, 1.5, 2.5, math.inf])
def test_restatement_at_a_training_point_is_finite(nu):
    X, alpha, kinv, amp, ell, _, noise = _problem(nu)
    dmean = PG.dmean_ref(X[:3], X, alpha, amp, ell, nu)
    dvar = PG.dvar_ref(X[:3], X, amp, ell, nu, noise)
    assert np.isfinite(dmean).all() and np.isfinite(dvar).all()


def _ei_fd(mean_fn, var_fn, x, fmin, h=1e-6):
    g = np.zeros_like(x)
    for k in range(len(x)):
        xp, xm = x.copy(), x.copy()
        xp[k] += h
        xm[k] -= h
        ep = E.expected_improvement(mean_fn(xp), math.sqrt(var_fn(xp)), fmin)
        em = E.expected_improvement(mean_fn(xm), math.sqrt(var_fn(xm)), fmin)
        g[k] = (ep - em) / (2 * h)
    return g


def test_ei_gradient_algebra_against_central_differences():
    # smooth mean / variance fields with known gradients
    mean_fn = lambda x: 0.3 + math.sin(2 * x[0]) * x[1]  # noqa: E731
    dmean_fn = lambda x: np.array([2 * math.cos(2 * x[0]) * x[1], math.sin(2 * x[0])])  # noqa: E731
    var_fn = lambda x: 0.05 + 0.2 * x[0] ** 2 + 0.1 * math.cos(x[1])  # noqa: E731
    dvar_fn = lambda x: np.array([0.4 * x[0], -0.1 * math.sin(x[1])])  # noqa: E731
    rng = np.random.default_rng(3)
    for fmin in (-0.2, 0.3, 0.9):
        for _ in range(10):
            x = rng.uniform(-1, 1, 2)
            ei, g = E.expected_improvement_with_gradient(mean_fn(x), var_fn(x), dmean_fn(x), dvar_fn(x), fmin)
            assert ei == E.expected_improvement(mean_fn(x), math.sqrt(var_fn(x)), fmin)
            fd = _ei_fd(mean_fn, var_fn, x, fmin)
            assert np.abs(g - fd).max() <= 1e-7 * max(1.0, np.abs(fd).max()), (g, fd)


def test_ei_gradient_in_the_zero_variance_branch():
    mean_fn = lambda x: 0.3 + x[0] - 2 * x[1]  # noqa: E731
    dm = np.array([1.0, -2.0])
    zero = lambda x: 0.0  # noqa: E731
    x = np.array([0.1, 0.2])
    for fmin, want in ((1.0, -dm), (-1.0, np.zeros(2))):  # mean < fmin: EI = fmin - mean, gradient -dmean; else 0
        ei, g = E.expected_improvement_with_gradient(mean_fn(x), 0.0, dm, np.array([0.7, 0.1]), fmin)
        assert ei == max(fmin - mean_fn(x), 0.0)
        assert np.array_equal(g, want)
        assert np.allclose(_ei_fd(mean_fn, zero, x, fmin), want, rtol=0, atol=1e-8)


def test_python_signatures_match_the_header_arity():
    # the ctypes argument lists follow include/hbegp.h: 8 arguments for the gradient predict, 10 for the maximiser
    for name in NEW:
        _, args = _lib.SIGNATURES[name]
        assert len(args) == (8 if "predict" in name else 10), name
        assert args[0] is C.c_void_p
