"""GPU: the log-space constrained expected improvement (hbegp_log_constrained_ei_* / hbegp_maximize_log_constrained_ei_*).

The device's lcei, lei, lpof and grad replayed through the NumPy / scipy restatement (tests/lcei_ref.py) on the engine's own
predict_grad outputs of the 1 + C models; best, mean and var bit for bit; the scalar function swept over every z of the 60-digit
table's points through fmin and a limit; the dead zone where hbegp_constrained_ei_* returns exactly 0 with a zero gradient;
consistency with the logarithm of cEI; clamped variances; bits across batch sizes, positions, gradient on / off, threads and the
constraints' order; the maximiser with the dead-zone search of tests/lcei_cases.py; the estimator's layer; the pool's poisons; the
phase clock; the C++ mirror.  The models are tests/test_gpu_cei.py's.

Bars: 1e-8 (f64) / 1e-4 (f32) times max(1, |reference value|) for lcei, lei and lpof, entry by entry (a -inf reference has to be
met exactly); for the gradient times max(1, sum_k(|d lcei / d mu_k| |dmean_k| + |d lcei / d sigma_k| |dsigma_k|) of the
restatement) as well, row by row.  Measured deviations: DESIGN section 24."""
import ctypes as C
import json
import math
import os
import subprocess
import threading

import numpy as np
import pytest

import lcei_cases as S
import lcei_ref as R
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E
from test_gpu_cei import D, _candidates, _fmin, _limits, _models, _posteriors, _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _release(fks):
    for fk in fks:
        fk.release()


def _compare(dtype, got, mu, vr, dmu, dvr, fmin, limits):
    """The device's (lcei, lei, lpof, grad) against the restatement's on the same posteriors: worst deviation / bar of the values
    and of the gradient.  Asserts both."""
    rv, rlei, rlpof, rg, scale = R.lcei_grad_x(mu, vr, dmu, dvr, fmin, limits)
    val, grad, lei, lpof = got
    worst = 0.0
    for name, a, b in (("lcei", val, rv), ("lei", lei, rlei), ("lpof", lpof, rlpof)):
        fin = np.isfinite(b)
        assert (a[~fin] == b[~fin]).all(), (name, a[~fin], b[~fin])  # a -inf is met exactly
        dev = np.abs(a[fin] - b[fin]) / R.value_bar(dtype, b[fin])
        if dev.size:
            worst = max(worst, float(dev.max()))
    gdev = np.abs(grad.astype(np.float64) - rg).max(axis=1) / R.grad_bar(dtype, rv, scale)
    assert np.isfinite(gdev).all()
    assert worst <= 1.0 and gdev.max() <= 1.0, (worst, float(gdev.max()))
    return worst, float(gdev.max())


def _replay(fks, Xs, fmin, limits, dtype, d=D):
    m, K = len(Xs), len(fks)
    val, best, grad, lei, lpof, mean, var = gpr.log_constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True, want_details=True)
    assert val.dtype == np.float64 and val.shape == (m,) and grad.dtype == dtype and grad.shape == (m, d)
    assert lei.dtype == np.float64 and lpof.dtype == np.float64 and mean.shape == (m, K) and var.shape == (m, K)
    pg, mu, vr, dmu, dvr = _posteriors(fks, Xs)
    for k in range(K):
        assert mean[:, k].tobytes() == pg[k][0].tobytes() and var[:, k].tobytes() == pg[k][1].tobytes()
    worst, gworst = _compare(dtype, (val, grad, lei, lpof), mu, vr, dmu, dvr, fmin, limits)
    print(f"  C={K - 1} m={m} d={d} fmin={fmin:.3g}: lcei in [{val.min():.4g}, {val.max():.4g}], deviation / bar: values {worst:.1e}, "
          f"grad {gworst:.1e}")
    assert (val == lei + lpof).all() and (lpof <= 0.0).all()
    if K == 1:
        assert val.tobytes() == lei.tobytes() and not lpof.any()
    if math.isinf(fmin):
        assert not lei.any() and val.tobytes() == lpof.tobytes()
    assert best == R.argmax_last(val)
    # the plain-space call on the same rows: the same posteriors bit for bit
    cdet = gpr.constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True, want_details=True)
    assert cdet[5].tobytes() == mean.tobytes() and cdet[6].tobytes() == var.tobytes()
    # without a gradient: the same bits
    val2, best2, lei2, lpof2, mean2, var2 = gpr.log_constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_details=True)
    assert val2.tobytes() == val.tobytes() and best2 == best and lei2.tobytes() == lei.tobytes() and lpof2.tobytes() == lpof.tobytes()
    cdet2 = gpr.constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_details=True)
    assert mean2.tobytes() == cdet2[4].tobytes() and var2.tobytes() == cdet2[5].tobytes()
    return worst, gworst


@pytest.mark.parametrize("n_con", [0, 1, 3, 8])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_lcei_replays_through_the_restatement(dtype, n_con):
    fks = _models(n_con, dtype)
    pool = _candidates(300, 11, dtype)
    limits, fmin = _limits(fks), _fmin(fks)
    worst = [0.0, 0.0]
    for m in (1, 5, 40, 300):  # 5: one workgroup of four waves plus one
        for fm in (fmin, math.inf):
            if n_con == 0 and math.isinf(fm):
                with pytest.raises(_lib.HbegpError, match="nothing to compute"):
                    gpr.log_constrained_ei(fks[0], [], pool[:m], fm, limits)
                continue
            r = _replay(fks, pool[:m], fm, limits, dtype)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"{np.dtype(dtype).name} C={n_con}: worst deviation / bar: values {worst[0]:.1e}, grad {worst[1]:.1e}")
    _release(fks)


@pytest.mark.parametrize("d", [1, 17, 64])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_replay_at_other_feature_counts(dtype, d):
    fks = _models(2, dtype, d=d)
    Xs = _candidates(5, 12, dtype, d=d)
    limits, fmin = _limits(fks), _fmin(fks)
    for fm in (fmin, math.inf):
        r = _replay(fks, Xs, fm, limits, dtype, d=d)
        print(f"{np.dtype(dtype).name} d={d} fmin={fm:.3g}: deviation / bar: values {r[0]:.1e}, grad {r[1]:.1e}")
    _release(fks)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_threshold_sweep_of_the_scalar_function(dtype):
    """One fixed candidate, m = 1, C = 1: fmin = mu_0 + z sigma_0 and limit = mu_1 + z sigma_1 for every z of the table, so the
    device evaluates its scalar function on both terms at (nearly) that z; the restatement is taken at the z the fp64 quotient
    realises.  The posteriors do not depend on the thresholds: they are read once."""
    with open(os.path.join(ROOT, "tests", "golden", "logei_table.json")) as f:
        zs = [float.fromhex(r["z"]) for r in json.load(f)["rows"]]
    fks = _models(1, dtype)
    x = _candidates(300, 11, dtype)[37:38]
    pg, mu, vr, dmu, dvr = _posteriors(fks, x)
    sd = np.sqrt(vr)
    assert (sd > 1e-3).all()
    worst, at = [0.0, 0.0], [0.0, 0.0]
    for z in zs:
        fmin, limits = float(mu[0, 0] + z * sd[0, 0]), np.array([mu[0, 1] + z * sd[0, 1]])
        val, best, grad, lei, lpof, mean, var = gpr.log_constrained_ei(fks[0], fks[1:], x, fmin, limits, want_grad=True, want_details=True)
        assert mean.tobytes() == np.array([[pg[0][0][0], pg[1][0][0]]], dtype=dtype).tobytes() and best == 0
        r = _compare(dtype, (val, grad, lei, lpof), mu, vr, dmu, dvr, fmin, limits)
        for i in range(2):
            if r[i] > worst[i]:
                worst[i], at[i] = r[i], z
    print(f"{np.dtype(dtype).name}: {len(zs)} thresholds: worst deviation / bar: values {worst[0]:.1e} at z = {at[0]:.6g}, "
          f"grad {worst[1]:.1e} at z = {at[1]:.6g}")
    _release(fks)


@pytest.mark.parametrize("n_con", [0, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dead_zone(dtype, n_con):
    """fmin_normalized = -1e3 and every limit -1e3 on the parity test's candidates: hbegp_constrained_ei_* returns exactly 0 and an
    all-zero gradient (the precondition), the log call finite values within the bar and a gradient whose every row is finite and
    nonzero."""
    fks = _models(n_con, dtype)
    Xs = _candidates(40, 11, dtype)
    fmin, limits = -1e3, np.full(n_con, -1e3)
    cval, _, cgrad = gpr.constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True)
    assert (cval == 0.0).all() and not cgrad.any()
    val, best, grad, lei, lpof, _, _ = gpr.log_constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True, want_details=True)
    _, mu, vr, dmu, dvr = _posteriors(fks, Xs)
    r = _compare(dtype, (val, grad, lei, lpof), mu, vr, dmu, dvr, fmin, limits)
    print(f"{np.dtype(dtype).name} C={n_con}: lcei in [{val.min():.4g}, {val.max():.4g}], |grad| rows in [{np.abs(grad).max(axis=1).min():.3g}, "
          f"{np.abs(grad).max(axis=1).max():.3g}], deviation / bar: values {r[0]:.1e}, grad {r[1]:.1e}")
    assert np.isfinite(val).all() and (val < -1000).all() and np.isfinite(grad).all() and grad.any(axis=1).all()
    assert best == R.argmax_last(val)
    _release(fks)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_consistent_with_the_logarithm_of_cei(dtype):
    fks = _models(3, dtype)
    Xs = _candidates(300, 11, dtype)
    limits, fmin = _limits(fks), _fmin(fks)
    n = 0
    for fm in (fmin, math.inf):
        cval, _ = gpr.constrained_ei(fks[0], fks[1:], Xs, fm, limits)
        val, _ = gpr.log_constrained_ei(fks[0], fks[1:], Xs, fm, limits)
        ok = cval >= 1e-280
        dev = np.abs(val[ok] - np.log(cval[ok])) / R.value_bar(dtype, np.log(cval[ok]))
        n += int(ok.sum())
        print(f"{np.dtype(dtype).name} fmin={fm:.3g}: {int(ok.sum())} of 300 rows with cei >= 1e-280, |lcei - log cei| / bar {dev.max():.1e}")
        assert ok.sum() > 100 and dev.max() <= 1.0
    _release(fks)


def test_clamped_variance_counts_as_sigma_zero():
    """The f32 amplitude-1e4 model of tests/test_gpu_predict_grad.py at its own training rows: about half of the variances are
    clamped to 0.  Every value is finite or -inf exactly as the indicator rule says, every gradient component is finite, nothing
    is NaN; the restatement on the same posteriors agrees."""
    g = np.stack(np.meshgrid(np.linspace(0, 1, 8), np.linspace(0, 1, 8)), axis=-1).reshape(-1, 2)
    dtype, scale, theta = np.float32, 100.0, np.log([1e-4, 1e4, 0.05, 0.05])
    X = g.astype(dtype)
    ys = [(np.sin(3 * g).sum(axis=1) * scale).astype(dtype), (np.cos(2 * g).sum(axis=1) * scale).astype(dtype),
          ((g ** 2).sum(axis=1) * scale).astype(dtype)]
    fks = [gpr.FittedKernel.extend(X, y, theta, nu=2.5) for y in ys]
    fmin, limits = 0.4 * scale, np.array([0.9, 0.8]) * scale
    for fm in (fmin, math.inf):
        val, best, grad, lei, lpof, mean, var = gpr.log_constrained_ei(fks[0], fks[1:], X, fm, limits, want_grad=True, want_details=True)
        zero = var == 0
        assert zero.sum() > 0
        assert not np.isnan(val).any() and not np.isnan(lei).any() and not np.isnan(lpof).any() and np.isfinite(grad).all()
        mu64, lim = mean.astype(np.float64), np.concatenate([[fm], limits])
        want_inf = (zero & ~(lim[None, :] > mu64)).any(axis=1)  # a sigma = 0 term at or beyond its threshold
        if math.isinf(fm):
            want_inf = (zero[:, 1:] & ~(limits[None, :] > mu64[:, 1:])).any(axis=1)
        assert ((val == -math.inf) == want_inf).all() and np.isfinite(val[~want_inf]).all()
        only = zero[:, 1:].all(axis=1)
        assert np.isin(lpof[only], (0.0, -math.inf)).all()  # every sigma_k = 0: a sum of log indicators
        _, mu, vr, dmu, dvr = _posteriors(fks, X)
        _compare(dtype, (val, grad, lei, lpof), mu, vr, dmu, dvr, fm, limits)
        assert best == R.argmax_last(val)
        print(f"fmin={fm:.3g}: {int(zero.sum())} clamped variances among 3 x 64, {int(want_inf.sum())} rows at -inf")
    _release(fks)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_row(dtype):
    fks = _models(2, dtype)
    limits, fmin = _limits(fks), _fmin(fks)
    Xs = _candidates(40, 31, dtype)
    clean = gpr.log_constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True, want_details=True)
    bad = Xs.copy()
    bad[13, 2] = math.nan
    val, best, grad, lei, lpof, _, _ = gpr.log_constrained_ei(fks[0], fks[1:], bad, fmin, limits, want_grad=True, want_details=True)
    keep = np.arange(40) != 13
    assert math.isnan(val[13]) and math.isnan(lei[13]) and math.isnan(lpof[13]) and np.isnan(grad[13]).all()
    assert val[keep].tobytes() == clean[0][keep].tobytes() and grad[keep].tobytes() == clean[2][keep].tobytes()
    assert lei[keep].tobytes() == clean[3][keep].tobytes() and lpof[keep].tobytes() == clean[4][keep].tobytes()
    assert best == R.argmax_last(val) and best != 13
    val0, best0 = gpr.log_constrained_ei(fks[0], fks[1:], np.zeros((0, D), dtype), fmin, limits)
    assert val0.shape == (0,) and best0 == -1
    _release(fks)


def test_bits_positions_gradient_threads_and_constraint_order():
    dtype = np.float64
    fks = _models(3, dtype)
    limits, fmin = _limits(fks), _fmin(fks)
    pool = _candidates(300, 21, dtype)
    obj, cons = fks[0], fks[1:]
    full = gpr.log_constrained_ei(obj, cons, pool, fmin, limits, want_grad=True, want_details=True)
    again = gpr.log_constrained_ei(obj, cons, pool, fmin, limits, want_grad=True, want_details=True)
    assert _same(full, again)
    nograd = gpr.log_constrained_ei(obj, cons, pool, fmin, limits)
    assert nograd[0].tobytes() == full[0].tobytes() and nograd[1] == full[1]
    for j in (0, 17, 299):
        for want_grad in (False, True):
            alone = gpr.log_constrained_ei(obj, cons, pool[j:j + 1], fmin, limits, want_grad=want_grad)
            assert alone[0][0] == full[0][j] and alone[1] == 0
            if want_grad:
                assert alone[2].tobytes() == full[2][j].tobytes()
    moved = gpr.log_constrained_ei(obj, cons, np.vstack([pool[40:60], pool[17:18], pool[:5]]), fmin, limits, want_grad=True, want_details=True)
    assert moved[0][20] == full[0][17] and moved[2][20].tobytes() == full[2][17].tobytes()
    assert moved[3][20] == full[3][17] and moved[4][20] == full[4][17]
    assert moved[0][:20].tobytes() == full[0][40:60].tobytes()
    # the constraints in the opposite order: the same quantity by other additions
    rev = gpr.log_constrained_ei(obj, cons[::-1], pool, fmin, limits[::-1], want_grad=True)
    _, mu, vr, dmu, dvr = _posteriors(fks, pool)
    rv, _, _, _, scale = R.lcei_grad_x(mu, vr, dmu, dvr, fmin, limits)
    assert (np.abs(rev[0] - full[0]) <= R.value_bar(dtype, rv)).all()
    assert (np.abs(rev[2] - full[2]).max(axis=1) <= R.grad_bar(dtype, rv, scale)).all()
    got = [None, None]

    def run_same(i):
        for _ in range(5):
            got[i] = gpr.log_constrained_ei(obj, cons, pool, fmin, limits, want_grad=True, want_details=True)

    def run_opposite(i):
        for _ in range(5):
            if i == 0:
                got[0] = gpr.log_constrained_ei(obj, cons, pool, fmin, limits, want_grad=True, want_details=True)
            else:
                got[1] = gpr.log_constrained_ei(obj, cons[::-1], pool, fmin, limits[::-1], want_grad=True)

    for target, what in ((run_same, "in the same order"), (run_opposite, "in opposite orders")):
        got[:] = [None, None]
        ts = [threading.Thread(target=target, args=(i,), daemon=True) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in ts), f"two concurrent log-cEI calls naming the constraints {what} did not return"
        assert _same(full, got[0])
        assert _same(full, got[1]) if target is run_same else _same(rev, got[1])
    _release(fks)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_maximiser(dtype):
    fks = _models(2, dtype)
    limits, fmin = _limits(fks), _fmin(fks)
    bounds = [(0.0, 1.0)] * D
    cand = np.random.default_rng(41).uniform(0, 1, (2000, D)).astype(dtype)
    for n_con in (2, 0):  # n_con = 0: log EI and its maximiser
        for fm in (fmin, math.inf) if n_con else (fmin,):
            cons, lim = fks[1:1 + n_con], limits[:n_con]
            cval, cbest = gpr.log_constrained_ei(fks[0], cons, cand, fm, lim)
            order = np.argsort(cval, kind="stable")
            starts = np.vstack([cand[order[-3:]], cand[:3]])  # the three best of the random candidates and three arbitrary ones
            s_val, _ = gpr.log_constrained_ei(fks[0], cons, starts, fm, lim)
            x, val, nevals = gpr.maximize_log_constrained_ei(fks[0], cons, starts, bounds, fm, lim, maxeval=60)
            assert x.dtype == dtype and x.shape == (6, D) and (x >= 0).all() and (x <= 1).all()
            assert (val >= s_val).all(), (val, s_val)
            assert (nevals >= 1).all() and (nevals <= 60).all()
            again, _ = gpr.log_constrained_ei(fks[0], cons, x, fm, lim)
            assert again.tobytes() == val.tobytes()
            print(f"{np.dtype(dtype).name} C={n_con} fmin={fm:.3g}: starts {s_val}, maximised {val}, evaluations {nevals}")
    lo, hi = np.zeros(D), np.ones(D)
    x, val, nevals = fks[0].maximize_log_ei(cand[:2], lo, hi, fmin, maxeval=20)
    assert val.tobytes() == fks[0].log_ei(x, fmin)[0].tobytes() and (nevals <= 20).all()
    _release(fks)


def test_dead_zone_search():
    """tests/lcei_cases.py (shown to work with the reference alone in tests/test_lcei_cpu.py): fmin = +inf, one low-noise
    constraint, six starts whose plain-space pof is exactly 0.  hbegp_maximize_constrained_ei_* returns its starts (the
    precondition); the log maximiser ends every run at a strictly larger lcei than its start, and at least one where
    hbegp_constrained_ei_* reports pof >= 0.5."""
    dtype = np.float64
    X = S.training_rows()
    tho, thc = S.thetas()
    obj = gpr.FittedKernel.extend(X, S.objective_targets(X), tho, nu=S.NU)
    con = gpr.FittedKernel.extend(X, S.constraint_targets(X), thc, nu=S.NU)
    starts, lim = S.starts().astype(dtype), [S.LIMIT]
    pof0, _, g0 = gpr.constrained_ei(obj, [con], starts, math.inf, lim, want_grad=True)
    assert (pof0 == 0.0).all() and not g0.any()
    px, pv, _ = gpr.maximize_constrained_ei(obj, [con], starts, S.BOUNDS, math.inf, lim, maxeval=S.MAXEVAL)
    assert px.tobytes() == starts.tobytes() and not pv.any()  # plain space does not move
    s_val, _ = gpr.log_constrained_ei(obj, [con], starts, math.inf, lim)
    x, val, nevals = gpr.maximize_log_constrained_ei(obj, [con], starts, S.BOUNDS, math.inf, lim, maxeval=S.MAXEVAL)
    again, _ = gpr.log_constrained_ei(obj, [con], x, math.inf, lim)
    end_pof, _ = gpr.constrained_ei(obj, [con], x, math.inf, lim)
    for i in range(len(starts)):
        print(f"run {i}: start x_0 = {starts[i, 0]:.3f} lcei = {s_val[i]:10.2f} -> lcei = {val[i]:9.3f} pof = {end_pof[i]:.4f} "
              f"at x = {x[i]} after {nevals[i]} evaluations")
    assert again.tobytes() == val.tobytes() and (nevals <= S.MAXEVAL).all() and (nevals >= 1).all()
    assert np.isfinite(s_val).all() and (val > s_val).all()
    assert (end_pof >= 0.5).sum() >= 1
    _release([obj, con])


def test_estimator_layer():
    """tests/test_gpu_cei.py::test_acquire_by_constrained_ei's three surrogates: log_constrained_ei_a is the logarithm of
    constrained_ei_a within the bar and ranks the same row first; acquire_by_log_constrained_ei picks distinct rows starting with
    it; with limits no row can meet, acquire_by_constrained_ei sees ties at exactly 0 while the log ranking still orders the
    rows; SurrogateModelGPR.maximize_log_ei reproduces FittedKernel.log_ei."""
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 1, (120, 3))
    y = ((X - 0.3) ** 2).sum(axis=1) + 0.5 + 0.02 * rng.standard_normal(120) ** 2
    g1 = ((X - 0.7) ** 2).sum(axis=1) + 0.5 + 0.02 * rng.standard_normal(120) ** 2
    g2 = X.sum(axis=1) + 1.0 + 0.02 * rng.standard_normal(120) ** 2
    model, c1, c2 = (E.EstimatorGPR.new(3).estimate(X, t, None, E.RNG.new_with_seed(4 + i)) for i, t in enumerate((y, g1, g2)))
    limits = [float(np.median(g1)), float(np.quantile(g2, 0.7))]
    fmin = E.feasible_fmin(y, np.stack([g1, g2], axis=1), limits)
    cand = np.random.default_rng(9).uniform(0, 1, (200, 3))
    cval, cbest = E.constrained_ei_a(model, [c1, c2], cand, fmin, limits)
    val, best = E.log_constrained_ei_a(model, [c1, c2], cand, fmin, limits)
    ok = cval >= 1e-280
    assert ok.sum() > 50 and (np.abs(val[ok] - np.log(cval[ok])) <= R.value_bar(model.dtype, np.log(cval[ok]))).all()
    assert best == R.argmax_last(val) and best == cbest
    idx, means, vals, fmins = E.acquire_by_log_constrained_ei(cand, model, [c1, c2], 3, limits, fmin=fmin)
    pidx, _, pvals, pfmins = E.acquire_by_constrained_ei(cand, model, [c1, c2], 3, limits, fmin=fmin)
    assert len(set(idx.tolist())) == 3 and idx[0] == best and vals[0] == val[best] and means.shape == (3, 3)
    assert idx[0] == pidx[0] and fmins[0] == pfmins[0] and (np.diff(fmins) <= 0).all()
    print(f"log picks {idx.tolist()} lcei {vals}; plain picks {pidx.tolist()} cei {pvals}")
    far = [float(g1.min()) - 50.0, float(g2.min()) - 50.0]  # limits far below anything either constraint model predicts
    zval, _ = E.constrained_ei_a(model, [c1, c2], cand, math.inf, far)
    lval, lbest = E.log_constrained_ei_a(model, [c1, c2], cand, math.inf, far)
    assert not zval.any() and np.isfinite(lval).all() and len(np.unique(lval)) > 100 and lbest == R.argmax_last(lval)
    lidx, _, lvals, _ = E.acquire_by_log_constrained_ei(cand, model, [c1, c2], 2, far, fmin=math.inf)
    assert lidx[0] == lbest and lvals[0] == lval[lbest] and len(set(lidx.tolist())) == 2
    x, v, ne = E.maximize_log_constrained_ei(model, [c1, c2], cand[[best, 0]], [(0.0, 1.0)] * 3, fmin, limits, maxeval=30)
    assert v[0] >= val[best] and v[1] >= val[0] and (ne <= 30).all()
    x, v, ne = model.maximize_log_ei(cand[:2], [(0.0, 1.0)] * 3, fmin, maxeval=20)
    assert v.tobytes() == model.fitted.log_ei(x, model._fmin_normalized(fmin))[0].tobytes() and (ne <= 20).all()


@pytest.mark.parametrize("poison_case", [(100, 4, 2.5), (300, 5, 2.5)], ids=lambda c: "n%d-d%d-nu%s" % c)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pool_hygiene_of_the_two_new_calls(dtype, poison_case):
    """tests/test_gpu_pool_hygiene.py's method: the bytes of a run on fresh blocks under HBEGP_POOL_POISON = 1 and 2."""
    import test_gpu_pool_hygiene as H

    def evaluate(fk, case, m, dt):
        cons = [H._model(case, dt, k=1), H._model(case, dt, k=2)]
        limits = [float(np.median(c.y_train)) for c in cons]
        fmin = float(np.quantile(np.asarray(fk.y_train, dtype=np.float64), 0.2))
        Xs = H._candidates(m, fk.d, 26 + m, dt)
        out = list(gpr.log_constrained_ei(fk, cons, Xs, fmin, limits, want_grad=True, want_details=True))
        out += list(gpr.maximize_log_constrained_ei(fk, cons, Xs[:4], [(-0.5, 1.5)] * fk.d, fmin, limits, maxeval=8))
        for c in cons:
            c.release()
        return out

    H._check(lambda: H._on_model(evaluate, poison_case, 70, dtype), 15, 6 * H._mat_bytes(poison_case[0], dtype))


def test_debug_lcei_phases():
    lib = _lib.load()
    fks = _models(2, np.float64)
    limits, fmin = _limits(fks), _fmin(fks)
    Xs = _candidates(300, 5, np.float64)
    ph, cph, cph2 = np.full(2, -1.0), np.full(2, -1.0), np.full(2, -2.0)
    assert lib.hbegp_debug_cei_phases(1, None) == _lib.OK  # a timed cEI call first: its record has to survive
    gpr.constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True)
    assert lib.hbegp_debug_cei_phases(0, _lib.dptr(cph)) == _lib.OK
    assert lib.hbegp_debug_lcei_phases(1, None) == _lib.OK
    timed = gpr.log_constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True)
    assert lib.hbegp_debug_lcei_phases(0, _lib.dptr(ph)) == _lib.OK
    assert lib.hbegp_debug_cei_phases(0, _lib.dptr(cph2)) == _lib.OK
    print(f"phases: the predicts {ph[0]:.3f} ms, the log kernel and the arg-max {ph[1]:.3f} ms (cEI's: {cph[0]:.3f}, {cph[1]:.3f})")
    assert np.isfinite(ph).all() and (ph > 0).all()
    assert cph2.tobytes() == cph.tobytes()  # the other kind's record is left alone
    untimed = gpr.log_constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True)
    assert _same(timed, untimed)  # timing changes no bit
    _release(fks)


def test_cpp_mirror_lcei(tmp_path):
    exe = str(tmp_path / "test_lcei")
    lib_dir = os.path.join(ROOT, "hbetune_rs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_lcei.cpp"),
                           "-L", lib_dir, "-lhbegp", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0 threw=1" in out.stdout
