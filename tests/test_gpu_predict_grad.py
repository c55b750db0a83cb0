"""GPU: posterior gradients at the query points (hbegp_predict_grad_*) and the batched EI maximiser (hbegp_maximize_ei_*).

Parity against the NumPy restatement (tests/predict_grad_ref.py): dmean on the model's own alpha (hbegp_model_get), dvar in
the library's form -2 (L^-1 dk) . (L^-1 k*) with the host's Cholesky factor; the explicit K^-1 form on the model's own K^-1 is
printed beside it (it loses digits as cond(K) grows).  Consistency with central differences of the device's own predict, the
edge cases of include/hbegp.h, the maximiser's contract and threads."""
import math
import threading

import numpy as np
import pytest

import predict_grad_ref as PG
from hbetune_rs_amd import _lib, gpr, synth
from hbetune_rs_amd import estimator as E
from oracle import gpr_oracle as O

pytestmark = pytest.mark.gpu

NUS = [0.5, 1.5, 2.5, math.inf]


def _data(n, d, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    return X.astype(dtype), y.astype(dtype)


def _model(n, d, nu, dtype, seed=1, noise_over_amp=1e-2):
    X, y = _data(n, d, seed, dtype)
    amp = 1.3
    ell = np.linspace(0.3, 0.9, d)
    theta = np.log(np.concatenate([[noise_over_amp * amp, amp], ell]))
    fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    # K = c Phi + s2 I with Phi PSD, Phi_ii = 1: lambda_max <= n c + s2, lambda_min >= s2
    cond_bound = (n * fk.amplitude + fk.noise) / fk.noise
    return fk, X, cond_bound


def _candidates(m, d, seed):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (m, d))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [200, 4096])
@pytest.mark.parametrize("nu", NUS)
def test_parity_with_the_restatement(nu, n, dtype):
    d = 4
    # f32: a larger noise keeps cond(K) where the f32 factor carries the 1e-4 bar for the variance gradient (measured at n = 4096:
    # up to 2.8e-4 per row at cond(K) <= 2e4, and 1.07e-4 for the squared exponential at cond(K) <= 4.1e3)
    f32_noise = 2.0 if math.isinf(nu) else 1.0
    fk, X, cond_bound = _model(n, d, nu, dtype, noise_over_amp=1e-2 if dtype == np.float64 else f32_noise)
    assert cond_bound <= 1e8
    alpha, kinv = fk.arrays()
    bar = 1e-8 if dtype == np.float64 else 1e-4
    for m in (1, 5, 40, 300):
        Xs = _candidates(m, d, 10 + m).astype(dtype)
        mean, var, dmean, dvar, _ = fk.predict_with_gradient(Xs)
        assert dmean.dtype == dtype and dmean.shape == (m, d) and dvar.shape == (m, d)
        rm = PG.dmean_ref(Xs, X, alpha, fk.amplitude, fk.length_scale, nu)
        rv = PG.dvar_ref(Xs, X, fk.amplitude, fk.length_scale, nu, fk.noise, var=var)
        dev_m, dev_v = PG.row_dev(dmean, rm), PG.row_dev(dvar, rv)
        dev_k = PG.row_dev(dvar, PG.dvar_ref_kinv(Xs, X, kinv, fk.amplitude, fk.length_scale, nu, var=var))
        print(f"nu={nu} n={n} {np.dtype(dtype).name} m={m}: dmean {dev_m:.2e} dvar {dev_v:.2e} (K^-1 form {dev_k:.2e}; "
              f"cond(K) <= {cond_bound:.1e})")
        assert dev_m <= bar and dev_v <= bar, (m, dev_m, dev_v)
    fk.release()


def test_fitted_m_size_model():
    w = synth.make_workload("M")
    X, y = w["X"], w["y"]
    starts = synth.restart_points("M", w["lo"], w["hi"], 2)
    fk = gpr.FittedKernel.new(X, y, w["theta0"], w["lo"], w["hi"], starts)
    alpha, kinv = fk.arrays()
    Xs = synth.candidates("M", 300, w["d"])
    mean, var, dmean, dvar, _ = fk.predict_with_gradient(Xs)
    dev_m = PG.row_dev(dmean, PG.dmean_ref(Xs, X, alpha, fk.amplitude, fk.length_scale, fk.nu))
    dev_v = PG.row_dev(dvar, PG.dvar_ref(Xs, X, fk.amplitude, fk.length_scale, fk.nu, fk.noise, var=var))
    dev_k = PG.row_dev(dvar, PG.dvar_ref_kinv(Xs, X, kinv, fk.amplitude, fk.length_scale, fk.nu, var=var))
    K = O.product_kernel(X, X, fk.amplitude, fk.length_scale, fk.nu)
    K[np.diag_indices(len(X))] += fk.noise
    ev = np.linalg.eigvalsh(K)
    print(f"M: cond(K) = {ev[-1] / ev[0]:.2e}; dmean {dev_m:.2e}, dvar vs the L^-1 form {dev_v:.2e}, "
          f"vs the explicit K^-1 form (not asserted) {dev_k:.2e}")
    assert dev_m <= 1e-8
    # at cond(K) = 6.7e11 the device's L^-1 and the host's differ in their trailing digits (L^-1 grows like sqrt(cond(K))):
    # measured 1.7e-6 between the two L^-1 forms, against ~2 (the whole scale) for the explicit K^-1 form
    assert dev_v <= 1e-5
    fk.release()


@pytest.mark.parametrize("nu", NUS)
def test_consistent_with_central_differences_of_predict(nu):
    d = 3
    fk, X, _ = _model(300, d, nu, np.float64, seed=4)
    Xs = _candidates(60, d, 5)
    ell = fk.length_scale
    dist = np.sqrt((((Xs / ell)[:, None, :] - (X / ell)[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
    Xs = Xs[dist > 0.05][:20]
    m = len(Xs)
    assert m > 8
    mean, var, dmean, dvar, nw = fk.predict_with_gradient(Xs)
    pm, pv, pw = fk.predict(Xs)  # batched path (m > 8)
    assert np.allclose(mean, pm, rtol=1e-12, atol=0) and np.allclose(var, pv, rtol=1e-12, atol=0) and nw == pw
    fd_m, fd_v = np.zeros((m, d)), np.zeros((m, d))
    for k in range(d):
        h = 1e-5 * ell[k]
        xp, xm = Xs.copy(), Xs.copy()
        xp[:, k] += h
        xm[:, k] -= h
        mp, vp, _ = fk.predict(xp)
        mm, vm, _ = fk.predict(xm)
        fd_m[:, k] = (mp - mm) / (2 * h)
        fd_v[:, k] = (vp - vm) / (2 * h)
    assert (var > 0).all()
    print(f"nu={nu}: |grad - central differences| / row scale: mean {PG.row_dev(dmean, fd_m):.2e}, var {PG.row_dev(dvar, fd_v):.2e}")
    assert PG.row_dev(dmean, fd_m) <= 1e-6
    assert PG.row_dev(dvar, fd_v) <= 1e-6
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nu", NUS)
def test_query_at_a_training_point_is_finite(nu, dtype):
    fk, X, _ = _model(150, 3, nu, dtype, noise_over_amp=1e-2 if dtype == np.float64 else 1.0)
    alpha, _ = fk.arrays(want_kinv=False)
    Xs = X[:12].copy()
    mean, var, dmean, dvar, _ = fk.predict_with_gradient(Xs)
    assert np.isfinite(dmean).all() and np.isfinite(dvar).all()
    rm = PG.dmean_ref(Xs, X, alpha, fk.amplitude, fk.length_scale, nu)
    rv = PG.dvar_ref(Xs, X, fk.amplitude, fk.length_scale, nu, fk.noise, var=var)
    bar = 1e-8 if dtype == np.float64 else 1e-4
    assert PG.row_dev(dmean, rm) <= bar and PG.row_dev(dvar, rv) <= bar
    fk.release()


def test_clamped_variance_has_zero_gradient():
    # f32, amplitude 1e4, noise 1e-8 of it: at the training points c + 1e-5 - |L^-1 k*|^2 is rounding of size eps32 * c,
    # well beyond 1e-5, so about half of those variances come out negative and are clamped
    g = np.stack(np.meshgrid(np.linspace(0, 1, 8), np.linspace(0, 1, 8)), axis=-1).reshape(-1, 2)
    X = g.astype(np.float32)
    y = np.sin(3 * g).sum(axis=1).astype(np.float32) * 100
    theta = np.log([1e-4, 1e4, 0.05, 0.05])
    fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
    mean, var, dmean, dvar, n_warn = fk.predict_with_gradient(X)
    clamped = var == 0
    print(f"clamped variances: {int(clamped.sum())} of {len(var)}, n_warn {n_warn}")
    assert clamped.any()
    assert (dvar[clamped] == 0).all()
    assert np.isfinite(dvar).all()
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_row_stays_in_its_row_and_m_zero(dtype):
    fk, X, _ = _model(300, 3, 2.5, dtype)
    Xs = _candidates(20, 3, 7).astype(dtype)
    ref = fk.predict_with_gradient(Xs)
    Xs[6, 1] = np.nan
    mean, var, dmean, dvar, _ = fk.predict_with_gradient(Xs)
    assert np.isnan(mean[6]) and np.isnan(var[6]) and np.isnan(dmean[6]).all() and np.isnan(dvar[6]).all()
    keep = np.arange(20) != 6
    for got, want in zip((mean, var, dmean, dvar), ref[:4]):
        assert np.array_equal(got[keep], want[keep])
    mean, var, dmean, dvar, n_warn = fk.predict_with_gradient(np.zeros((0, 3), dtype=dtype))
    assert mean.shape == (0,) and dmean.shape == (0, 3) and n_warn == 0
    fk.release()


def test_mean_only_and_bitwise_repeatable():
    fk, X, _ = _model(700, 5, 1.5, np.float64)
    Xs = _candidates(130, 5, 8)
    a = fk.predict_with_gradient(Xs)
    b = fk.predict_with_gradient(Xs)
    for u, v in zip(a[:4], b[:4]):
        assert u.tobytes() == v.tobytes()
    mean, var, dmean, dvar, _ = fk.predict_with_gradient(Xs, want_variance=False)
    assert var is None and dvar is None
    assert mean.tobytes() == a[0].tobytes() and dmean.tobytes() == a[2].tobytes()
    fk.release()


def test_wrong_arguments():
    lib = _lib.load()
    fk, X, _ = _model(100, 2, 2.5, np.float64)
    Xs = _candidates(3, 2, 1)
    out, g = np.zeros(3), np.zeros((3, 2))
    d = _lib.dptr

    def einval(rc, what):
        assert rc == _lib.EINVAL and what in _lib.last_error(), _lib.last_error()

    einval(lib.hbegp_predict_grad_f64(fk._h, d(Xs), 3, d(out), d(out), d(g), None, None), "together")
    einval(lib.hbegp_predict_grad_f64(fk._h, d(Xs), 3, d(out), None, d(g), d(g), None), "together")
    einval(lib.hbegp_predict_grad_f64(fk._h, d(Xs), -1, d(out), None, d(g), None, None), "m must be")
    Xf = Xs.astype(np.float32)
    einval(lib.hbegp_predict_grad_f32(fk._h, _lib.fptr(Xf), 3, _lib.fptr(Xf), None, _lib.fptr(Xf), None, None), "f64 data")
    lo, hi = np.zeros(2), np.ones(2)
    starts = np.array([[0.2, 0.3], [0.5, 0.5]])
    xo, eo = np.zeros((2, 2)), np.zeros(2)
    einval(lib.hbegp_maximize_ei_f64(fk._h, d(starts), 2, d(hi), d(lo), 0.0, 10, d(xo), d(eo), None), "lo[0] > hi[0]")
    einval(lib.hbegp_maximize_ei_f64(fk._h, d(starts + 0.6), 2, d(lo), d(hi), 0.0, 10, d(xo), d(eo), None), "outside the box")
    einval(lib.hbegp_maximize_ei_f64(fk._h, d(starts), 0, d(lo), d(hi), 0.0, 10, d(xo), d(eo), None), "S must be")
    einval(lib.hbegp_maximize_ei_f64(fk._h, d(starts), 2, d(lo), d(hi), 0.0, 0, d(xo), d(eo), None), "maxeval")
    einval(lib.hbegp_maximize_ei_f64(fk._h, d(starts), 2, d(lo), d(hi), math.nan, 10, d(xo), d(eo), None), "fmin")
    fk.release()


def _fitted_estimator_model(d, n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = ((X - 0.37) ** 2).sum(axis=1)
    model = E.EstimatorGPR.new(d).estimate(X, y, None, E.RNG.new_with_seed(seed))
    return model, X, y


def _projected_gradient(x, g, lo, hi):
    pg = g.copy()
    pg[(x <= lo) & (g < 0)] = 0  # minimising -EI: gradient of -EI is -g; at lo a step down is blocked when -g > 0
    pg[(x >= hi) & (g > 0)] = 0
    return pg


@pytest.mark.parametrize("d,grid", [(1, 20001), (2, 401)])
def test_maximizer_reaches_the_grid_maximum(d, grid):
    model, X, y = _fitted_estimator_model(d, 5 if d == 1 else 10, 11 + d)
    bounds = [(0.0, 1.0)] * d
    lo, hi = np.zeros(d), np.ones(d)
    fmin = float(y.min())
    lattice = (np.arange(16) + 0.5) / 16 if d == 1 else (np.arange(4) + 0.5) / 4
    starts = np.stack(np.meshgrid(*[lattice] * d, indexing="ij"), axis=-1).reshape(-1, d)
    x, ei, nevals = model.maximize_ei(starts, bounds, fmin, maxeval=150)
    assert x.shape == (16, d) and ei.shape == (16,) and (nevals >= 1).all() and (nevals <= 150).all()
    assert ((x >= lo) & (x <= hi)).all()
    _, ei_start = model.predict_mean_ei_a(starts, fmin)
    assert (ei >= ei_start).all()
    _, ei_at = model.predict_mean_ei_a(x, fmin)
    assert np.allclose(ei, ei_at, rtol=1e-10, atol=1e-300), np.abs(ei - ei_at).max()
    axes = [np.linspace(0, 1, grid)] * d
    G = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, d)
    ei_grid = np.concatenate([model.predict_mean_ei_a(G[i:i + 40000], fmin)[1] for i in range(0, len(G), 40000)])
    print(f"d={d}: best EI {ei.max():.10e}, grid max {ei_grid.max():.10e}, evaluations per run {nevals.min()}..{nevals.max()}")
    assert ei.max() >= ei_grid.max() * (1 - 1e-6)
    # runs that stopped early: projected gradient of EI at their point within the optimiser's tolerance
    _, ei2, dei = model.predict_mean_ei_grad_a(x, fmin)
    early = nevals < 150
    pg = np.array([np.abs(_projected_gradient(x[i], dei[i], lo, hi)).max() for i in range(16)])
    print("projected |dEI| of the early runs:", pg[early])
    assert (pg[early] <= 1e-5 * np.maximum(1.0, ei[early])).all(), pg[early]
    # deterministic
    x2, ei2, nevals2 = model.maximize_ei(starts, bounds, fmin, maxeval=150)
    assert x2.tobytes() == x.tobytes() and ei2.tobytes() == ei.tobytes() and np.array_equal(nevals, nevals2)


def test_maximizer_f32_stays_in_the_box():
    rng = np.random.default_rng(2)
    X = rng.uniform(0, 1, (60, 2)).astype(np.float32)
    y = (((X - 0.3) ** 2).sum(axis=1)).astype(np.float32)
    model = E.EstimatorGPR.new(2).estimate(X, y, None, E.RNG.new_with_seed(2))
    lo, hi = np.array([0.1, 0.1]), np.array([0.9, 0.7])
    starts = rng.uniform(0.1, 0.7, (8, 2)).astype(np.float32)
    x, ei, nevals = model.maximize_ei(starts, list(zip(lo, hi)), float(y.min()), maxeval=60)
    assert x.dtype == np.float32
    assert ((x.astype(np.float64) >= lo) & (x.astype(np.float64) <= hi)).all()
    _, ei_start = model.predict_mean_ei_a(starts, float(y.min()))
    assert (ei >= ei_start.astype(np.float64) * (1 - 1e-6)).all()


def test_gradient_estimator_chain_rule():
    for projection in ("linear", "logarithmic"):
        rng = np.random.default_rng(9)
        X = rng.uniform(0, 1, (50, 2))
        y = 1.0 + ((X - 0.4) ** 2).sum(axis=1)
        model = E.EstimatorGPR.new(2).y_projection(projection).estimate(X, y, None, E.RNG.new_with_seed(9))
        Xs = rng.uniform(0, 1, (12, 2))
        mean, g = model.predict_mean_grad_a(Xs)
        assert np.allclose(mean, model.predict_mean_a(Xs), rtol=1e-12)
        for k in range(2):
            h = 1e-5 * model.fitted.length_scale[k]
            xp, xm = Xs.copy(), Xs.copy()
            xp[:, k] += h
            xm[:, k] -= h
            fd = (model.predict_mean_a(xp) - model.predict_mean_a(xm)) / (2 * h)
            assert np.abs(g[:, k] - fd).max() <= 1e-6 * np.abs(fd).max(), (projection, np.abs(g[:, k] - fd).max())
        _, ei, dei = model.predict_mean_ei_grad_a(Xs, float(y.min()))
        _, ei_ref = model.predict_mean_ei_a(Xs, float(y.min()))
        assert np.allclose(ei, ei_ref, rtol=1e-10, atol=1e-300)
        assert dei.shape == (12, 2)


def test_threads_return_the_single_thread_bits():
    fks = [_model(500, 4, 2.5, np.float64)[0] for _ in range(5)]
    Xs = [_candidates(40 + 30 * i, 4, 20 + i) for i in range(4)]
    ref = [fks[0].predict_with_gradient(x) for x in Xs]
    for shared in (True, False):
        got = [None] * 4

        def run(i):
            fk = fks[0] if shared else fks[1 + i]
            for _ in range(3):
                got[i] = fk.predict_with_gradient(Xs[i])

        ts = [threading.Thread(target=run, args=(i,)) for i in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for i in range(4):
            for u, v in zip(got[i][:4], ref[i][:4]):
                assert u.tobytes() == v.tobytes(), (shared, i)
    for fk in fks:
        fk.release()
