"""CPU: the restatement of leave-one-out cross-validation (tests/loo_ref.py) against genuine one-row-deleted refits and against
central differences, and the argument checks of the new entry points (no GPU needed: they refuse before any device call).

The refits go through oracle.gpr_oracle.extend / predict.  Their bookkeeping: predict() returns the LATENT variance
c + 1e-5 - k*^T K^-1 k* (predict.rs:25-37: no noise s2, plus min_noise = 1e-5), the leave-one-out variance is the observation's,
so var_i = predict's variance + s2 - 1e-5."""
import ctypes as C
import math

import numpy as np
import pytest

import loo_ref as LR
from hbetune_rs_amd import _lib
from oracle import gpr_oracle as O

NUS = [0.5, 1.5, 2.5, math.inf]


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    return X, y


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("n", [60, 200])
def test_restatement_equals_real_row_deletion(nu, n):
    X, y = _data(n, 3, n)
    s2, c, ell = 0.02, 1.3, np.array([0.3, 0.6, 0.9])
    r = LR.loo(X, y, s2, c, ell, nu, want_grad=False)
    worst_mu = worst_var = 0.0
    for i in range(n):
        keep = np.arange(n) != i
        fit = O.extend(X[keep], y[keep], s2, c, ell, nu)
        mean, var, _ = O.predict(X[i:i + 1], X[keep], fit["alpha"], fit["k_inv"], c, ell, nu)
        worst_mu = max(worst_mu, abs(mean[0] - r["mean"][i]))
        worst_var = max(worst_var, abs(var[0] + s2 - O.MIN_NOISE - r["var"][i]))
    print(f"nu={nu} n={n}: mean off by {worst_mu:.2e}, var by {worst_var:.2e}")
    # cond(K) <= n c / s2 + 1 ~ 1.3e4: LAPACK's refits carry ~1e-12 of it
    assert worst_mu <= 1e-10 and worst_var <= 1e-10
    # the two forms of m_i, and lpd as the Gaussian log density of y_i under (mu_i, var_i)
    assert np.abs(r["m"] / r["m_kinv"] - 1).max() <= 1e-12
    dens = -0.5 * np.log(2 * math.pi * r["var"]) - (y - r["mean"]) ** 2 / (2 * r["var"])
    assert np.abs(dens - r["lpd"]).max() <= 1e-12 * max(1.0, np.abs(dens).max())
    assert r["loo"] == pytest.approx(dens.sum(), rel=1e-13)


@pytest.mark.parametrize("nu", NUS)
def test_gradient_forms_agree_and_match_central_differences(nu):
    n, d = 60, 3
    X, y = _data(n, d, 7)
    theta = np.log(np.array([0.02, 1.3, 0.3, 0.6, 0.9]))
    r = LR.loo_at_theta(X, y, theta, nu, by_the_book=True)
    scale = max(1.0, np.abs(r["grad_book"]).max())
    assert np.abs(r["grad"] - r["grad_book"]).max() <= 1e-11 * scale  # the identity: one n^3 product instead of p
    # central differences with h = 1e-4: truncation ~ h^2 |loo'''| / 6 ~ 1e-8 of the scale, rounding ~ 1e-16 |loo| / h ~ 1e-10
    h = 1e-4
    fd = np.zeros_like(theta)
    for j in range(len(theta)):
        e = np.zeros_like(theta)
        e[j] = h
        fd[j] = (LR.loo_at_theta(X, y, theta + e, nu, want_grad=False)["loo"]
                 - LR.loo_at_theta(X, y, theta - e, nu, want_grad=False)["loo"]) / (2 * h)
    print(f"nu={nu}: gradient {r['grad']}, off central differences by {np.abs(fd - r['grad']).max():.2e}")
    assert np.abs(fd - r["grad"]).max() <= 1e-6 * scale


def test_clamped_length_scale_is_evaluated_at_its_bound():
    X, y = _data(40, 2, 3)
    lo, hi = np.array([1e-5, 0.1, 0.05, 0.05]), np.array([1e5, 10.0, 2.0, 0.5])
    theta = np.log(np.array([0.05, 1.0, 0.4, 0.9]))  # ell_2 above its bound
    a = LR.loo_at_theta(X, y, theta, 2.5, lo, hi)
    v = np.exp(theta)  # (the unclamped parameters exactly as loo_at_theta forms them)
    b = LR.loo(X, y, v[0], v[1], np.array([v[2], 0.5]), 2.5)
    assert a["loo"] == b["loo"] and np.array_equal(a["grad"], b["grad"])


# ---------------------------------------------------------------------------------------------------------------- the C ABI
NEW_SYMBOLS = ["hbegp_model_loo_f64", "hbegp_model_loo_f32", "hbegp_problem_eval_loo", "hbegp_fit_loo_f64", "hbegp_fit_loo_f32",
               "hbegp_debug_loo_phases"]


def test_new_symbols_are_exported_and_version_is_unchanged():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.hbegp_version() == 200


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_model_loo_refuses_null_model_and_all_null_outputs(sfx):
    lib = _lib.load()
    fn = getattr(lib, f"hbegp_model_loo_{sfx}")
    loo = C.c_double()
    assert fn(None, None, None, None, C.byref(loo), None) == _lib.EINVAL
    assert "NULL model" in _lib.last_error()
    grad = np.zeros(4)
    assert fn(None, None, None, None, None, _lib.dptr(grad)) == _lib.EINVAL
    assert "NULL model" in _lib.last_error()
    assert fn(None, None, None, None, None, None) == _lib.EINVAL
    assert "every output is NULL" in _lib.last_error()


def test_problem_eval_loo_refuses_null_arguments():
    lib = _lib.load()
    theta = np.zeros(3)
    loo = C.c_double()
    assert lib.hbegp_problem_eval_loo(None, 0, 0, _lib.dptr(theta), None, None, C.byref(loo), None) == _lib.EINVAL
    assert "NULL problem" in _lib.last_error()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_fit_loo_checks_its_arguments_like_fit(sfx):
    lib = _lib.load()
    fn = getattr(lib, f"hbegp_fit_loo_{sfx}")
    x = np.zeros(4, dtype=np.float64 if sfx == "f64" else np.float32)
    t = np.zeros(4)
    bad = _lib.FitOptions()
    bad.struct_size = 0
    rc = fn(None, _lib.aptr(x), _lib.aptr(x), 4, 1, 2.5, _lib.dptr(t), _lib.dptr(t), _lib.dptr(t), None, 0, C.byref(bad), None, None, None)
    assert rc == _lib.EINVAL and "struct_size" in _lib.last_error()
    ok = _lib.FitOptions()
    rc = fn(None, _lib.aptr(x), _lib.aptr(x), 4, 1, 2.5, _lib.dptr(t), _lib.dptr(t), _lib.dptr(t), None, 0, C.byref(ok), None, None, None)
    assert rc == _lib.EINVAL and "ctx is NULL" in _lib.last_error()


def test_loo_phase_hook_runs_without_a_device():
    lib = _lib.load()
    ph = np.full(4, -1.0)
    assert lib.hbegp_debug_loo_phases(0, _lib.dptr(ph)) == 0
    assert (ph == 0).all()
