"""CPU: the restatement of leave-group-out cross-validation (tests/lgo_ref.py) against genuine group-deleted refits, its two
gradient forms against each other and against central differences, its two limits (singletons = leave-one-out, one group = the
log marginal likelihood), estimator.replicate_groups, and the argument checks of the new entry points (no GPU needed).

The refits go through oracle.gpr_oracle.extend on the rows outside the group; the group's predictive distribution is then
N(k* alpha, K** + s2 I - k* K^-1 k*^T) from the oracle's kernel matrices, and lpd_g its log density at y_I."""
import ctypes as C
import math

import numpy as np
import pytest

import lgo_ref as GR
import loo_ref as LR
from hbetune_rs_amd import _lib
from hbetune_rs_amd import estimator as E
from oracle import gpr_oracle as O

NUS = [0.5, 1.5, 2.5, math.inf]
D = 4
S2, AMP, ELL = 1e-2, 1.3, np.array([0.3, 0.5, 0.7, 0.9])


def _data(n, d=D, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    return X, y


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


@pytest.mark.parametrize("nu", NUS)
def test_restatement_equals_real_group_deletion(nu):
    n = 200
    X, y = _data(n, seed=n)
    groups = GR.group_mix(n)
    r = GR.lgo(X, y, S2, AMP, ELL, nu, groups, want_grad=False)
    sizes = sorted(len(I) for I in r["members"])
    assert sizes[-7:] == [1, 1, 2, 5, 17, 33, 64] and len(r["members"]) == 7 + n - 123
    worst_mu = worst_lpd = 0.0
    for g, I in enumerate(r["members"]):
        keep = np.setdiff1d(np.arange(n), I)
        fit = O.extend(X[keep], y[keep], S2, AMP, ELL, nu)
        Ks = O.product_kernel(X[I], X[keep], AMP, ELL, nu)
        mu = Ks @ fit["alpha"]
        cov = O.product_kernel(X[I], X[I], AMP, ELL, nu) + S2 * np.eye(len(I)) - Ks @ fit["k_inv"] @ Ks.T
        Lc = np.linalg.cholesky(0.5 * (cov + cov.T))
        z = np.linalg.solve(Lc, y[I] - mu)
        lpd = -0.5 * float(z @ z) - float(np.log(np.diag(Lc)).sum()) - 0.5 * len(I) * math.log(2 * math.pi)
        worst_mu = max(worst_mu, _rel(r["mean"][I], mu))
        worst_lpd = max(worst_lpd, _rel(r["lpd"][g], lpd))
        assert _rel(r["var"][I], np.diag(cov)) <= 1e-9
    print(f"nu={nu}: mean off by {worst_mu:.2e}, lpd by {worst_lpd:.2e} (bar 1e-9)")
    assert worst_mu <= 1e-9 and worst_lpd <= 1e-9


@pytest.mark.parametrize("nu", NUS)
def test_gradient_two_forms_and_central_differences(nu):
    n = 200
    X, y = _data(n, seed=n)
    groups = GR.group_mix(n)
    theta = np.log(np.concatenate([[S2, AMP], ELL]))
    r = GR.lgo_at_theta(X, y, theta, nu, groups, by_the_book=True)
    scale = max(1.0, np.abs(r["grad_book"]).max())
    d_forms = np.abs(r["grad"] - r["grad_book"]).max() / scale
    h, fd = 1e-5, np.zeros(len(theta))
    for j in range(len(theta)):
        e = np.zeros(len(theta))
        e[j] = h
        fd[j] = (GR.lgo_at_theta(X, y, theta + e, nu, groups, want_grad=False)["lgo"] -
                 GR.lgo_at_theta(X, y, theta - e, nu, groups, want_grad=False)["lgo"]) / (2 * h)
    d_fd = np.abs(r["grad"] - fd).max() / np.abs(fd).max()
    print(f"nu={nu}: the two forms differ by {d_forms:.2e} (bar 1e-10), central differences by {d_fd:.2e} (bar 1e-6)")
    assert d_forms <= 1e-10 and d_fd <= 1e-6


@pytest.mark.parametrize("nu", NUS)
def test_singletons_are_leave_one_out_and_one_group_is_the_lml(nu):
    X, y = _data(200, seed=3)
    a = GR.lgo(X, y, S2, AMP, ELL, nu, None)
    b = LR.loo(X, y, S2, AMP, ELL, nu)
    for k, kb in (("mean", "mean"), ("var", "var"), ("lpd", "lpd"), ("lgo", "loo"), ("grad", "grad")):
        assert _rel(a[k], b[kb]) <= 1e-12, k
    assert _rel(GR.lgo(X, y, S2, AMP, ELL, nu, np.arange(200)[::-1].copy())["mean"], b["mean"]) <= 1e-12
    X, y = _data(64, seed=4)
    one = GR.lgo(X, y, S2, AMP, ELL, nu, np.full(64, 9))
    ref = O.lml_with_gradient(X, y, S2, AMP, ELL, nu)
    assert len(one["lpd"]) == 1
    assert _rel(one["lgo"], ref["lml"]) <= 1e-10 and _rel(one["grad"], ref["grad"]) <= 1e-10
    assert np.abs(one["mean"]).max() <= 1e-9  # nothing is left to predict from: the prior mean


def test_replicate_groups():
    rng = np.random.default_rng(0)
    base = rng.uniform(0, 1, (5, 3))
    x = np.concatenate([base[[0, 1, 0, 2, 1, 0]], np.repeat(base[3:4], 130, axis=0), base[[4, 2]]])
    g = E.replicate_groups(x)
    assert g.dtype == np.int32 and g.shape == (len(x),)
    assert g[:6].tolist() == [0, 1, 0, 2, 1, 0]
    assert sorted(set(g.tolist())) == list(range(g.max() + 1))  # dense
    big = g[6:136]
    assert len(set(big.tolist())) == 3 and np.bincount(big - big.min()).tolist() == [64, 64, 2]
    assert (np.diff(big) >= 0).all()  # split in row order
    assert g[136] not in set(g[:136].tolist()) and g[137] == 2
    assert E.replicate_groups(x, max_size=200)[6:136].min() == E.replicate_groups(x, max_size=200)[6:136].max()
    for lab in set(g.tolist()):  # equal labels: equal rows
        rows = x[g == lab]
        assert (rows == rows[0]).all()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
NEW_SYMBOLS = ["hbegp_model_lgo_f64", "hbegp_model_lgo_f32", "hbegp_problem_eval_lgo", "hbegp_fit_lgo_f64", "hbegp_fit_lgo_f32",
               "hbegp_debug_lgo_phases"]


def test_new_symbols_are_exported_and_registered():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.hbegp_version() == 200


def test_argument_checks_refuse_before_any_device_call():
    lib = _lib.load()
    out = C.c_double()
    assert lib.hbegp_model_lgo_f64(None, None, None, None, None, None, None, None) == _lib.EINVAL
    assert "every output is NULL" in _lib.last_error()
    assert lib.hbegp_model_lgo_f64(None, None, None, None, None, None, C.byref(out), None) == _lib.EINVAL
    assert "NULL model" in _lib.last_error()
    assert lib.hbegp_problem_eval_lgo(None, 0, 0, None, None, None, None, C.byref(out), None) == _lib.EINVAL
    assert "NULL problem" in _lib.last_error()
    ph = np.full(4, -1.0)
    assert lib.hbegp_debug_lgo_phases(0, _lib.dptr(ph)) == 0
    assert (ph == 0).all()
