"""GPU: leave-group-out cross-validation -- hbegp_model_lgo_*, hbegp_problem_eval_lgo, hbegp_fit_lgo_* and the estimator's opt-in
objective -- against the NumPy restatement (tests/lgo_ref.py), against its two limits on the device (singletons = leave-one-out,
one group = the log marginal likelihood) and, independently of the restatement, against real group deletion on the device.

Bars as in tests/test_gpu_loo.py: parity_rules.TOL64 = 1e-8 and TOL32 = 1e-4, relative to max(1, scale of the reference); the
variance relative to c + s2.  Thetas as there: noise = 1e-2 amplitude (f64) and = amplitude (f32)."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import lgo_ref as GR
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


def _groups(n):
    """The partition each size is tested with: 1 and 64 one group (64: the cap, M_II = K^-1 whole), 100 runs of 1 .. 9 rows, 129 the
    pair {127, 128} across the block edge among runs of three, 200 the CPU test's mix, other sizes one scattered group of 64, runs of
    five and singletons."""
    if n in (1, 64):
        return np.full(n, 5, dtype=np.int32)
    if n == 100:
        return np.repeat(np.arange(40), np.arange(40) % 9 + 1)[:n].astype(np.int32)
    if n == 129:
        g = (np.arange(n) // 3).astype(np.int32)
        g[126] = 1000
        g[127] = g[128] = -1
        return g
    if n == 200:
        return GR.group_mix(n)
    perm = np.random.default_rng(n).permutation(n)
    g = np.empty(n, dtype=np.int32)
    g[perm[:64]] = -7
    rest = perm[64:]
    k = len(rest) // 2
    g[rest[:k]] = 10 + np.arange(k) // 5
    g[rest[k:]] = 100000 + np.arange(len(rest) - k)
    return g


@functools.lru_cache(maxsize=8)
def _ref_at_test_theta(n, nu, dtype_name):
    X, y, theta = _data(n, np.dtype(dtype_name), seed=n)
    return GR.lgo_at_theta(X, y, theta, nu, _groups(n))


def _check(what, got, ref, tol, c_plus_s2):
    """got = (mean, var, lpd, lgo, grad) of the device."""
    mean, var, lpd, lgo, grad = got
    assert len(lpd) == len(ref["lpd"])
    devs = dict(mean=PRU.dev(mean, ref["mean"]), var=PRU.dev(var, ref["var"], scale=1.0) / c_plus_s2, lpd=PRU.dev(lpd, ref["lpd"]),
                lgo=PRU.dev(lgo, ref["lgo"]), grad=PRU.dev(grad, ref["grad"]))
    print(f"{what}: " + ", ".join(f"{k} off by {v:.2e}" for k, v in devs.items()) +
          f" (lgo {ref['lgo']:.6g}, max |grad| {np.abs(ref['grad']).max():.3g}, {len(lpd)} groups; bar {tol:g})")
    for k, v in devs.items():
        assert v <= tol, (what, k, v)


CASES = [(n, kind) for n in (1, 64, 100, 129, 200) for kind in (["extend"] if n <= 128 else ["extend", "extend_with"])]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,kind", CASES)
@pytest.mark.parametrize("nu", NUS)
def test_model_lgo_matches_restatement(nu, n, kind, dtype):
    X, y, theta = _data(n, dtype, seed=n)
    if kind == "extend":
        fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    else:
        n0 = 128 if n == 129 else n - 70
        prior = gpr.FittedKernel.extend(X[:n0], y[:n0], theta, nu=nu)
        fk = prior.extend_with(X, y)
        assert fk.incremental
        prior.release()
    noise, amp, _ = fk.device_params()
    ref = _ref_at_test_theta(n, nu, np.dtype(dtype).name)
    g = _groups(n)
    got = fk.lgo(g, want_grad=True)
    assert got[0].dtype == np.dtype(dtype) and got[2].dtype == np.dtype(dtype) and got[4].dtype == np.float64
    _check(f"nu={nu} n={n} {kind} {np.dtype(dtype).name}", got, ref, _tol(dtype), amp + noise)
    # without the gradient: the same diagnostics; the same call: the same bits
    m2, v2, l2, lgo2 = fk.lgo(g)
    assert np.array_equal(m2, got[0]) and np.array_equal(v2, got[1]) and np.array_equal(l2, got[2]) and lgo2 == got[3]
    again = fk.lgo(g, want_grad=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_model_lgo_where_the_gram_sums_split_into_row_chunks(dtype):
    """n = 1100: the Gram sums of the group of 64 rows take five chunks of 256 rows, those of the runs of five two chunks of 1024,
    the singletons' one.  The diagnostics alone (the gradient's kernels do not see the chunks)."""
    n = 1100
    X, y, theta = _data(n, dtype, seed=n)
    g = _groups(n)
    v = np.exp(theta)
    ref = GR.lgo(X, y, v[0], v[1], v[2:], 2.5, g, want_grad=False)
    fk = gpr.FittedKernel.extend(X, y, theta)
    mean, var, lpd, lgo = fk.lgo(g)
    fk.release()
    tol = _tol(dtype)
    devs = dict(mean=PRU.dev(mean, ref["mean"]), var=PRU.dev(var, ref["var"], scale=1.0) / (v[0] + v[1]), lpd=PRU.dev(lpd, ref["lpd"]),
                lgo=PRU.dev(lgo, ref["lgo"]))
    print(f"n={n} {np.dtype(dtype).name}: " + ", ".join(f"{k} off by {d:.2e}" for k, d in devs.items()) + f" (bar {tol:g})")
    for k, d in devs.items():
        assert d <= tol, k


# ---------------------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [100, 200])
def test_singletons_are_leave_one_out_on_the_device(n, dtype):
    X, y, theta = _data(n, dtype, seed=n + 2)
    fk = gpr.FittedKernel.extend(X, y, theta)
    tol = _tol(dtype)
    loo = fk.loo(want_grad=True)
    by_null = fk.lgo(None, want_grad=True)
    by_label = fk.lgo(np.arange(n)[::-1] * 3 - 50, want_grad=True)  # n distinct labels: the dense ids are the row indices
    assert all(np.array_equal(a, b) for a, b in zip(by_null, by_label))
    noise, amp, _ = fk.device_params()
    for name, a, b, scale in (("mean", by_null[0], loo[0], None), ("var", by_null[1], loo[1], amp + noise), ("lpd", by_null[2], loo[2], None),
                              ("lgo", by_null[3], loo[3], None), ("grad", by_null[4], loo[4], None)):
        dv = PRU.dev(a, b) if scale is None else PRU.dev(a, b, scale=1.0) / scale
        print(f"n={n} {np.dtype(dtype).name} singletons against model_loo: {name} off by {dv:.2e} (bar {tol:g})")
        assert dv <= tol, name
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nu", [0.5, 2.5])
def test_one_group_of_all_rows_is_the_lml_on_the_device(nu, dtype):
    X, y, theta = _data(64, dtype, seed=8)
    prob = gpr.Problem(X, y, nu=nu)
    lml, grad = prob.lml_with_gradient(theta)
    prob.close()
    fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    _, _, lpd, lgo, g = fk.lgo(np.zeros(64, dtype=np.int64), want_grad=True)
    fk.release()
    tol = _tol(dtype)
    print(f"nu={nu} {np.dtype(dtype).name}: one group of 64 against the lml: off by {PRU.dev(lgo, lml):.2e}, grad by {PRU.dev(g, grad):.2e}")
    assert len(lpd) == 1 and PRU.dev(lgo, lml) <= tol and PRU.dev(g, grad) <= tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_relabelling_the_groups_changes_no_row(dtype):
    n = 200
    X, y, theta = _data(n, dtype, seed=n)
    fk = gpr.FittedKernel.extend(X, y, theta)
    g = _groups(n)
    a = fk.lgo(g, want_grad=True)
    # the same partition under other integers, negative ones too
    uniq = np.unique(g)
    new = dict(zip(uniq.tolist(), (np.random.default_rng(0).permutation(len(uniq)) * 11 - 400).tolist()))
    g2 = np.array([new[v] for v in g.tolist()], dtype=np.int64)
    b = fk.lgo(g2, want_grad=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    tol = _tol(dtype)
    assert PRU.dev(b[2], a[2]) <= tol and PRU.dev(b[3], a[3]) <= tol and PRU.dev(b[4], a[4]) <= tol
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nu", [0.5, 2.5, math.inf])
def test_model_lgo_equals_real_group_deletion_on_the_device(nu, dtype):
    """No restatement: extend on the data without the group's rows at the same theta, the joint posterior at them."""
    n = 300
    X, y, theta = _data(n, dtype, seed=5)
    perm = np.random.default_rng(6).permutation(n)
    g = 1000 + np.arange(n)
    members = [np.sort(perm[:2]), np.sort(perm[2:11]), np.sort(perm[11:75])]
    for k, I in enumerate(members):
        g[I] = k
    order = {int(v): i for i, v in enumerate(dict.fromkeys(g.tolist()))}  # dense ids: order of first appearance
    fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    mean, var, lpd, _ = fk.lgo(g)
    fk.release()
    s2, c = math.exp(theta[0]), math.exp(theta[1])
    tol = _tol(dtype)
    for k, I in enumerate(members):
        keep = np.setdiff1d(np.arange(n), I)
        fd = gpr.FittedKernel.extend(X[keep], y[keep], theta, nu=nu)
        pm, cov = fd.predict_cov(X[I])
        fd.release()
        cov = cov.astype(np.float64) + (s2 - 1e-5) * np.eye(len(I))
        Lc = np.linalg.cholesky(0.5 * (cov + cov.T))
        z = np.linalg.solve(Lc, y[I].astype(np.float64) - pm)
        want_lpd = -0.5 * float(z @ z) - float(np.log(np.diag(Lc)).sum()) - 0.5 * len(I) * math.log(2 * math.pi)
        d_m = PRU.dev(mean[I], pm)
        d_v = PRU.dev(var[I], np.diag(cov), scale=1.0) / (c + s2)
        d_l = PRU.dev(lpd[order[k]], want_lpd)
        print(f"nu={nu} {np.dtype(dtype).name} group of {len(I)}: mean off by {d_m:.2e}, var by {d_v:.2e}, lpd by {d_l:.2e} (bar {tol:g})")
        assert d_m <= tol and d_v <= tol and d_l <= tol, (len(I), d_m, d_v, d_l)


def test_model_lgo_refusals():
    X, y, theta = _data(130, np.float64)
    fk = gpr.FittedKernel.extend(X, y, theta)
    lib = _lib.load()
    lgo = C.c_double()
    g = np.zeros(130, dtype=np.int32)
    g[65:] = 1 + np.arange(65)
    ip = g.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.hbegp_model_lgo_f64(fk._h, ip, None, None, None, None, C.byref(lgo), None) == _lib.EINVAL
    assert "group 0 holds 65 rows" in _lib.last_error()
    g[64] = 1  # 64 rows: the cap itself is fine
    assert lib.hbegp_model_lgo_f64(fk._h, ip, None, None, None, None, C.byref(lgo), None) == _lib.OK
    assert lib.hbegp_model_lgo_f32(fk._h, ip, None, None, None, None, C.byref(lgo), None) == _lib.EINVAL
    assert "model holds f64 data" in _lib.last_error()
    assert lib.hbegp_model_lgo_f64(fk._h, ip, None, None, None, None, None, None) == _lib.EINVAL
    assert "every output is NULL" in _lib.last_error()
    with pytest.raises(ValueError):
        fk.lgo(np.zeros(129, dtype=np.int32))
    with pytest.raises(ValueError):
        fk.lgo(np.zeros(130))
    # the problem and the fit refuse the same partition
    prob = gpr.Problem(X, y)
    g[64] = 0
    with pytest.raises(Exception, match="holds 65 rows"):
        prob.lgo_with_gradient(theta, g)
    prob.close()
    lo, hi = _fit_box(np.float64)
    with pytest.raises(Exception, match="holds 65 rows"):
        gpr.FittedKernel.new_by_lgo(X, y, np.log(np.sqrt(lo * hi)), lo, hi, None, maxeval=3, groups=g)
    fk.release()


# ---------------------------------------------------------------------------------------------------------------- the problem
BOX_LO = np.concatenate([[1e-4, 0.1], np.full(D, 0.05)])
BOX_HI = np.concatenate([[1e2, 10.0], np.full(D, 0.8)])


def _thetas(theta):
    inside = theta.copy()
    inside[2:] -= 0.7  # every length scale inside its bounds: nothing is clamped
    clamped = theta.copy()
    clamped[2 + D - 1] = math.log(2.0)  # ell_D = 2 > its bound 0.8: evaluated at 0.8
    return [inside, clamped]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,nu", [(1, 2.5), (100, 2.5), (300, 1.5), (300, 2.5), (900, 2.5)])  # single launch, launch path, task queue
def test_problem_eval_lgo_matches_restatement_and_leaves_the_slot_alone(n, nu, dtype):
    X, y, theta = _data(n, dtype, seed=n + 1)
    g = _groups(n)
    tol = _tol(dtype)
    prob = gpr.Problem(X, y, nu=nu)
    plain = gpr.Problem(X, y, nu=nu)
    for k, th in enumerate(_thetas(theta)):
        lgo, grad = prob.lgo_with_gradient(th, g, BOX_LO, BOX_HI)
        ref = GR.lgo_at_theta(X, y, th, nu, g, BOX_LO, BOX_HI)
        d_l, d_g = PRU.dev(lgo, ref["lgo"]), PRU.dev(grad, ref["grad"])
        print(f"nu={nu} n={n} {np.dtype(dtype).name} theta {k}: lgo off by {d_l:.2e}, grad by {d_g:.2e} (bar {tol:g})")
        assert d_l <= tol and d_g <= tol
        # the slot afterwards: what hbegp_problem_eval at that theta leaves behind, bit for bit
        want_lml, _ = plain.lml_with_gradient(th, BOX_LO, BOX_HI, want_grad=False)
        for a, b in zip(prob.results(), plain.results()):
            assert np.array_equal(a, b)
        # the same call gives the same bits; without the gradient the same value
        lgo2, grad2 = prob.lgo_with_gradient(th, g, BOX_LO, BOX_HI)
        assert lgo2 == lgo and np.array_equal(grad2, grad)
        assert prob.lgo_with_gradient(th, g, BOX_LO, BOX_HI, want_grad=False)[0] == lgo
        # a following evaluation is undisturbed
        lml_a, g_a = prob.lml_with_gradient(th, BOX_LO, BOX_HI)
        lml_b, g_b = plain.lml_with_gradient(th, BOX_LO, BOX_HI)
        assert lml_a == lml_b == want_lml and np.array_equal(g_a, g_b)
    prob.close()
    plain.close()


def test_problem_eval_lgo_agrees_with_model_lgo():
    X, y, theta = _data(300, np.float64, seed=3)
    g = _groups(300)
    prob = gpr.Problem(X, y)
    lgo, grad = prob.lgo_with_gradient(theta, g)
    prob.close()
    fk = gpr.FittedKernel.extend(X, y, theta)
    _, _, _, lgo_m, grad_m = fk.lgo(g, want_grad=True)
    fk.release()
    assert PRU.dev(lgo, lgo_m) <= PRU.TOL64 and PRU.dev(grad, grad_m) <= PRU.TOL64


@pytest.mark.parametrize("n", [100, 300])
def test_problem_eval_lgo_nan_in_y_is_not_positive_definite(n):
    """A numerical outcome: NOT_PD, -inf and a zero gradient; the slot works afterwards."""
    lib = _lib.load()
    X, y, theta = _data(n, np.float64, seed=2)
    g = _groups(n)
    yn = y.copy()
    yn[17] = np.nan
    prob = gpr.Problem(X, yn)
    lgo, grad = C.c_double(1.0), np.ones(D + 2)
    rc = lib.hbegp_problem_eval_lgo(prob._h, 0, 0, _lib.dptr(theta), None, None, g.ctypes.data_as(C.POINTER(C.c_int)), C.byref(lgo),
                                    _lib.dptr(grad))
    assert rc == _lib.NOT_PD and lgo.value == -math.inf and (grad == 0).all()
    assert prob.lgo_with_gradient(theta, g) is None
    prob.close()
    good = gpr.Problem(X, y)
    got = good.lgo_with_gradient(theta, g)
    ref = GR.lgo_at_theta(X, y, theta, 2.5, g)
    assert PRU.dev(got[0], ref["lgo"]) <= PRU.TOL64 and PRU.dev(got[1], ref["grad"]) <= PRU.TOL64
    good.close()


def test_problem_eval_lgo_same_bits_from_threads_on_different_slots():
    X, y, theta = _data(700, np.float64, seed=4)
    g = _groups(700)
    prob = gpr.Problem(X, y, n_slots=3)
    want = prob.lgo_with_gradient(theta, g)
    out, errs = [None] * 3, []

    def work(slot):
        try:
            for _ in range(3):
                out[slot] = prob.lgo_with_gradient(theta, g, slot=slot)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(s,)) for s in range(3)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for lgo, grad in out:
        assert lgo == want[0] and np.array_equal(grad, want[1])
    prob.close()


# ---------------------------------------------------------------------------------------------------------------- the fit
def _fit_box(dtype, d=D):
    """tests/test_gpu_loo.py's box: f64 noise >= 1e-3 x the amplitude's upper bound, f32 noise >= the amplitude's upper bound."""
    if np.dtype(dtype) == np.float64:
        lo = np.concatenate([[4e-3, 0.25], np.full(d, 0.1)])
        hi = np.concatenate([[4.0, 4.0], np.full(d, 3.0)])
    else:
        lo = np.concatenate([[4.0, 0.25], np.full(d, 0.1)])
        hi = np.concatenate([[400.0, 4.0], np.full(d, 3.0)])
    return lo, hi


@pytest.mark.parametrize("dtype,n", [(np.float64, 100), (np.float64, 300), (np.float64, 800), (np.float32, 300)])
def test_fit_lgo(dtype, n):
    X, y, _ = _data(n, dtype, seed=n + 7)
    g = _groups(n)
    lo, hi = _fit_box(dtype)
    tol = _tol(dtype)
    theta0 = np.log(np.sqrt(lo * hi))
    maxeval = 8 if n <= 300 else 5
    starts = np.log(lo) + (np.log(hi) - np.log(lo)) * np.random.default_rng(n).uniform(0, 1, (1, D + 2))
    fk = gpr.FittedKernel.new_by_lgo(X, y, theta0, lo, hi, starts, maxeval=maxeval, trace=True, groups=g)
    tr = fk.trace
    assert fk.n_evals == len(tr["lml"]) and set(tr["run"]) == {0, 1} and fk.n_evals <= 2 * maxeval
    worst_l = worst_g = 0.0
    for th, lgo, grad in zip(tr["theta"], tr["lml"], tr["grad"]):
        ref = GR.lgo_at_theta(X, y, th, 2.5, g, lo, hi)
        worst_l, worst_g = max(worst_l, PRU.dev(lgo, ref["lgo"])), max(worst_g, PRU.dev(grad, ref["grad"]))
    print(f"fit_lgo n={n} {np.dtype(dtype).name}: {len(tr['lml'])} evaluations, lgo off by {worst_l:.2e}, grad by {worst_g:.2e} (bar {tol:g}); "
          f"lgo {tr['lml'][0]:.6g} -> {fk.lgo_best:.6g}")
    assert worst_l <= tol and worst_g <= tol
    # the capture rule: the arg-max of the trace (ties to the lowest (run, eval): the trace is in that order), clamped
    i = int(np.argmax(tr["lml"]))
    assert fk.lgo_best == tr["lml"][i]
    want_theta = np.array([math.log(min(max(math.exp(t), a), b)) for t, a, b in zip(tr["theta"][i], lo, hi)])
    assert np.array_equal(fk.theta_best, want_theta) and np.array_equal(fk.theta, want_theta)
    assert np.array_equal(tr["theta"][0], theta0)
    # the model is extend at theta_best, bit for bit
    ext = gpr.FittedKernel.extend(X, y, fk.theta_best)
    for a, b in zip(fk.arrays(), ext.arrays()):
        assert np.array_equal(a, b)
    assert fk.lml == ext.lml
    assert PRU.dev(fk.lgo(g)[3], fk.lgo_best) <= tol
    # row variances go through: zeros give the bits of none
    fz = gpr.FittedKernel.new_by_lgo(X, y, theta0, lo, hi, starts, maxeval=maxeval, trace=True, groups=g, row_variance=np.zeros(n))
    assert np.array_equal(fz.theta_best, fk.theta_best) and fz.lgo_best == fk.lgo_best
    assert np.array_equal(fz.trace["lml"], tr["lml"]) and np.array_equal(fz.trace["grad"], tr["grad"])
    for a, b in zip(fk.arrays(), fz.arrays()):
        assert np.array_equal(a, b)
    for f in (fk, fz, ext):
        f.release()


def test_fit_lgo_honours_maxeval_and_fixed_work_and_row_variance():
    X, y, _ = _data(200, np.float64, seed=9)
    g = _groups(200)
    lo, hi = _fit_box(np.float64)
    theta0 = np.log(np.sqrt(lo * hi))
    fk = gpr.FittedKernel.new_by_lgo(X, y, theta0, lo, hi, None, maxeval=7, fixed_work=True, groups=g)
    assert fk.n_evals == 7
    fk.release()
    fk = gpr.FittedKernel.new_by_lgo(X, y, theta0, lo, hi, None, maxeval=3, groups=g, trace=True)
    assert 1 <= fk.n_evals <= 3
    # a row variance that is not zero changes the objective as the restatement says
    rv = np.linspace(0.0, 0.05, 200)
    fr = gpr.FittedKernel.new_by_lgo(X, y, theta0, lo, hi, None, maxeval=3, groups=g, trace=True, row_variance=rv)
    v = np.exp(fr.trace["theta"][0])
    ref = GR.lgo(X, y, v[0], v[1], v[2:], 2.5, g, rv=rv)
    assert PRU.dev(fr.trace["lml"][0], ref["lgo"]) <= PRU.TOL64 and PRU.dev(fr.trace["grad"][0], ref["grad"]) <= PRU.TOL64
    assert fr.trace["lml"][0] != fk.trace["lml"][0]
    fk.release()
    fr.release()


# ---------------------------------------------------------------------------------------------------------------- what it is for
def test_replicates_leave_one_out_is_more_confident_than_leave_group_out():
    """40 points x 3 replicates with independent noise of standard deviation 0.3 on a unit-scale function.  At one fixed theta, a
    row predicted with its replicates in the training set has a higher log density than predicted without them in expectation; the
    sums over the rows of this data set are compared per row at the theta new_by_loo finds."""
    rng = np.random.default_rng(12)
    base = rng.uniform(0, 1, (40, 2))
    x = np.repeat(base, 3, axis=0)
    y = np.sin(4 * x[:, 0]) * np.cos(3 * x[:, 1]) + 0.3 * rng.standard_normal(120)
    g = E.replicate_groups(x)
    assert g.max() == 39 and (np.bincount(g) == 3).all()
    lo = np.array([1e-3, 0.05, 0.05, 0.05])
    hi = np.array([10.0, 10.0, 5.0, 5.0])
    theta0 = np.log(np.array([0.1, 1.0, 0.5, 0.5]))
    f_loo = gpr.FittedKernel.new_by_loo(x, y, theta0, lo, hi, None, maxeval=40)
    f_lgo = gpr.FittedKernel.new_by_lgo(x, y, theta0, lo, hi, None, maxeval=40, groups=g)
    loo_row = f_loo.loo()[3] / 120
    lgo_row = f_loo.lgo(g)[3] / 120
    print(f"replicates: at the loo fit's theta loo / row = {loo_row:.4f}, lgo / row = {lgo_row:.4f}; fitted noise {math.exp(f_loo.theta[0]):.4g} "
          f"(loo objective) and {math.exp(f_lgo.theta[0]):.4g} (lgo objective); the data's is {0.3 ** 2:.4g}")
    assert lgo_row < loo_row
    f_loo.release()
    f_lgo.release()


def test_estimator_objective_lgo_and_lgo_a():
    n, d = 90, 3
    rng = np.random.default_rng(11)
    x = np.repeat(rng.uniform(0, 1, (n // 3, d)), 3, axis=0)
    y = 40.0 + 25.0 * ((x - 0.4) ** 2).sum(axis=1) + rng.standard_normal(n)
    g = E.replicate_groups(x)
    est = lambda: E.EstimatorGPR.new(d).noise_bounds(1e-3, 1e1).length_scale_bounds([(0.05, 5.0)] * d)  # noqa: E731
    m_default = est().estimate(x, y, None, E.RNG(3))
    m_groups_unused = est().estimate(x, y, None, E.RNG(3), groups=g)  # the default objective does not read them
    assert np.array_equal(m_default.fitted.theta, m_groups_unused.fitted.theta) and not hasattr(m_default.fitted, "lgo_best")
    m_lgo = est().objective("lgo").estimate(x, y, None, E.RNG(3), groups=g)
    assert PRU.dev(m_lgo.fitted.lgo(g)[3], m_lgo.fitted.lgo_best) <= PRU.TOL64
    y_train, y_norm = E.YNormalize.new_project_into_normalized(y, "linear", None)
    noise, amp, ell = m_lgo.fitted.device_params()
    ref = GR.lgo(x, y_train, noise, amp, ell, 2.5, g, want_grad=False)
    mean, std, resid = m_lgo.lgo_a(g)
    assert PRU.dev(mean, y_norm.project_mean_from_normalized(ref["mean"], ref["var"])) <= PRU.TOL64
    assert PRU.dev(std, y_norm.project_std_from_normalized(ref["mean"], ref["var"])) <= PRU.TOL64
    assert PRU.dev(resid, (y_train - ref["mean"]) / np.sqrt(ref["var"])) <= PRU.TOL64
    for m in (m_default, m_groups_unused, m_lgo):
        m.fitted.release()


# ---------------------------------------------------------------------------------------------------------------- pool hygiene
_CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lgo_pool_child.py")


def _child(tmp_path, name, settings):
    out = str(tmp_path / f"{name}.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("HBEGP_POOL_FRESH", "HBEGP_POOL_POISON")}
    subprocess.run([sys.executable, _CHILD, out] + settings, env=env, check=True, timeout=120)
    return np.load(out)


def test_model_lgo_does_not_depend_on_recycled_pool_blocks(tmp_path):
    """One model_lgo with a gradient at n = 200 in child processes: the reference in a process whose every block is fresh, then in
    another process on blocks poisoned with finite garbage, with NaN, and with no switch at all -- which recycles exactly the blocks
    the poisoned calls gave back.  The same bytes every time: the poisoned calls drew at least the call's three blocks (the small
    arrays, Y, C: 2 n_p^2 doubles) and did not read what they held, and the blocks went back cleared."""
    ref = _child(tmp_path, "fresh", ["fresh"])
    assert ref["fresh_blocks"] == 0
    got = _child(tmp_path, "recycled", ["poison1", "poison2", "plain"])
    assert got["plain_blocks"] == 0
    for mode in ("poison1", "poison2", "plain"):
        if mode != "plain":
            assert got[mode + "_blocks"] >= 3 and got[mode + "_bytes"] >= 2 * 256 * 256 * 8, (mode, got[mode + "_blocks"], got[mode + "_bytes"])
        for k in ("mean", "var", "lpd", "lgo", "grad"):
            assert ref["fresh_" + k].tobytes() == got[f"{mode}_{k}"].tobytes(), (mode, k)
