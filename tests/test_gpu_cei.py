"""GPU: the constrained expected improvement (hbegp_constrained_ei_* / hbegp_maximize_constrained_ei_*).

The device's cei, ei, pof and grad replayed through the NumPy restatement (tests/cei_ref.py) on the engine's own predict_grad outputs
of the 1 + C models; best, mean and var against predict / predict_grad bit for bit; bits across batch sizes, positions, gradient on
/ off, threads and the constraints' order; clamped variances, NaN rows, m = 0, argument checks; the maximiser; the estimator's
acquire_by_constrained_ei; the C++ mirror; the phase clock.  (Models on different devices are refused too; one device cannot show
it.)

Bars: 1e-8 (f64) / 1e-4 (f32) times max(1, max_j(|fmin - mu_0j| + sigma_0j)) (times 1 for fmin = +inf); for the gradient times
max(1, the largest sum_k(|d cei / d mu_k| |dmean_k| + |d cei / d sigma_k| |dsigma_k|) of the restatement) as well.  Measured
deviations: DESIGN section 22."""
import ctypes as C
import math
import os
import subprocess
import threading

import numpy as np
import pytest

import cei_ref as R
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 4
# f32: a noise of the amplitude's size keeps cond(K) <= n + 1 (tests/test_gpu_kg.py)
F32_NOISE = 1.0
NUS = (1.5, 0.5, math.inf, 2.5)  # model k has nu = NUS[k % 4]
NS = (100, 60, 300, 150, 200, 90, 120, 250, 75)  # model k has n = NS[k]: 100 for the objective, 60 .. 300 for the constraints
N_NEAR = 24  # candidates next to shared training rows: small sigma, so F is next to 0 or 1 there


def _rows(d=D, seed=1):
    """The 300 rows every model takes its first n from."""
    return np.random.default_rng(seed).uniform(0, 1, (300, d))


def _model(k, dtype, d=D, seed=1, n=None):
    """tests/test_gpu_ehvi.py::_model over nine response functions: model k on the first NS[k] of the shared rows, at a fixed
    theta (no fit)."""
    n = NS[k] if n is None else n
    X = _rows(d, seed)[:n]
    rng = np.random.default_rng(seed + 100 * (k + 1))
    if k == 0:
        y = np.sin(3 * X).sum(axis=1) / math.sqrt(d) * 2
    else:
        y = np.cos((1.5 + 0.5 * k) * X + 0.7 * k).sum(axis=1) / math.sqrt(d) * 2 + ((X - 0.1 * k) ** 2).sum(axis=1) / d
    y = y + 0.1 * rng.standard_normal(n)
    X, y = X.astype(dtype), y.astype(dtype)
    amp = 1.3 if k == 0 else 0.6 + 0.1 * k
    noise_over_amp = 1e-2 if dtype == np.float64 else F32_NOISE
    ell = np.linspace(0.3, 0.9, d) if k % 2 == 0 else np.linspace(0.8, 0.4, d)
    theta = np.log(np.concatenate([[noise_over_amp * amp, amp], ell]))
    return gpr.FittedKernel.extend(X, y, theta, nu=NUS[k % 4])


def _models(n_con, dtype, d=D, seed=1):
    return [_model(k, dtype, d, seed) for k in range(1 + n_con)]


def _candidates(m, seed, dtype, d=D):
    """m rows: the first N_NEAR next to training rows that every model holds (a small sigma in every model), the others uniform
    over a box a little larger than the data's."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.1, 1.1, (m, d))
    near = min(m, N_NEAR)
    c[:near] = _rows(d)[:near] + 0.002 * rng.standard_normal((near, d))
    return c[rng.permutation(m)].astype(dtype)


def _limits(fks):
    """One limit per constraint: the median of its training targets, moved a little per constraint -- across the candidates the
    constraint then almost surely holds, almost surely fails, or is even."""
    return np.array([float(np.median(fk.y_train)) + 0.05 * (k % 3 - 1) for k, fk in enumerate(fks[1:])])


def _fmin(fks):
    return float(np.quantile(np.asarray(fks[0].y_train, dtype=np.float64), 0.2))


def _posteriors(fks, Xs):
    pg = [fk.predict_with_gradient(Xs) for fk in fks]
    mu, vr, dmu, dvr = (np.stack([p[i] for p in pg], axis=1).astype(np.float64) for i in range(4))
    return pg, mu, vr, dmu, dvr


def _replay(fks, Xs, fmin, limits, dtype, d=D):
    """Device cei / ei / pof / grad against the restatement on the engine's own predict_grad outputs; best, mean, var bit for bit.
    Returns (worst deviation of the values / their bar, of grad / its bar, the restatement's per-model factors)."""
    m, K = len(Xs), len(fks)
    val, best, grad, ei, pof, mean, var = gpr.constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True, want_details=True)
    assert val.dtype == np.float64 and val.shape == (m,) and grad.dtype == dtype and grad.shape == (m, d)
    assert ei.dtype == np.float64 and pof.dtype == np.float64 and mean.shape == (m, K) and var.shape == (m, K)
    pg, mu, vr, dmu, dvr = _posteriors(fks, Xs)
    for k in range(K):
        assert mean[:, k].tobytes() == pg[k][0].tobytes() and var[:, k].tobytes() == pg[k][1].tobytes()
    rv, rei, rpof, rg, scale = R.cei_grad_x(mu, vr, dmu, dvr, fmin, limits)
    bar = R.value_bar(dtype, mu[:, 0], vr[:, 0], fmin)
    gbar = R.grad_bar(dtype, mu[:, 0], vr[:, 0], fmin, scale)
    pbar = 1e-8 if dtype == np.float64 else 1e-4  # pof is a probability
    dev = max(float(np.abs(val - rv).max()), float(np.abs(ei - rei).max()))
    pdev = float(np.abs(pof - rpof).max())
    gdev = float(np.abs(grad.astype(np.float64) - rg).max())
    print(f"  C={K - 1} m={m} d={d} fmin={fmin:.3g}: cei max {val.max():.3e} deviation {dev:.1e} (bar {bar:.1e}), pof deviation {pdev:.1e} "
          f"(bar {pbar:.1e}), grad deviation {gdev:.1e} (bar {gbar:.1e})")
    assert dev <= bar, (m, K, dev, bar)
    assert pdev <= pbar, (m, K, pdev, pbar)
    assert gdev <= gbar, (m, K, gdev, gbar)
    assert (val >= 0.0).all() and (pof >= 0.0).all() and (pof <= 1.0).all() and (ei >= 0.0).all()
    if math.isinf(fmin):
        assert (ei == 1.0).all() and val.tobytes() == pof.tobytes()
    assert best == R.argmax_last(val)
    # without a gradient: the same bits, and the batched predict's posterior
    val2, best2, ei2, pof2, mean2, var2 = gpr.constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_details=True)
    assert val2.tobytes() == val.tobytes() and best2 == best and ei2.tobytes() == ei.tobytes() and pof2.tobytes() == pof.tobytes()
    assert mean2.tobytes() == mean.tobytes() and var2.tobytes() == var.tobytes()
    if m > 16:  # predict's batched path: the same launches
        for k in range(K):
            pm, pv, _ = fks[k].predict(Xs)
            assert mean2[:, k].tobytes() == pm.tobytes() and var2[:, k].tobytes() == pv.tobytes()
    return max(dev / bar, pdev / pbar), gdev / gbar, R.parts(mu, vr, fmin, limits)[0]


@pytest.mark.parametrize("n_con", [0, 1, 3, 8])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_cei_replays_through_the_restatement(dtype, n_con):
    fks = _models(n_con, dtype)
    pool = _candidates(300, 11, dtype)
    limits, fmin = _limits(fks), _fmin(fks)
    worst = [0.0, 0.0]
    for m in (1, 5, 40, 300):  # 5: one workgroup of four waves plus one
        for fm in (fmin, math.inf):
            if n_con == 0 and math.isinf(fm):
                with pytest.raises(_lib.HbegpError, match="nothing to compute"):
                    gpr.constrained_ei(fks[0], [], pool[:m], fm, limits)
                continue
            r = _replay(fks, pool[:m], fm, limits, dtype)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
            if m == 300 and dtype == np.float64 and not math.isinf(fm):
                for k in range(1, 1 + n_con):  # the candidates hold rows with F next to 0, next to 1/2 and next to 1
                    F = r[2][:, k]
                    assert F.min() < 0.05 and F.max() > 0.95 and ((F > 0.25) & (F < 0.75)).any(), (k, F.min(), F.max())
    print(f"{np.dtype(dtype).name} C={n_con}: worst deviation / bar: values {worst[0]:.1e}, grad {worst[1]:.1e}")
    for fk in fks:
        fk.release()


@pytest.mark.parametrize("d", [1, 17, 64])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_replay_at_other_feature_counts(dtype, d):
    fks = _models(2, dtype, d=d)
    Xs = _candidates(5, 12, dtype, d=d)
    limits, fmin = _limits(fks), _fmin(fks)
    for fm in (fmin, math.inf):
        r = _replay(fks, Xs, fm, limits, dtype, d=d)
        print(f"{np.dtype(dtype).name} d={d} fmin={fm:.3g}: deviation / bar: values {r[0]:.1e}, grad {r[1]:.1e}")
    for fk in fks:
        fk.release()


def _same(a, b):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b))


def test_bits_positions_gradient_threads_and_constraint_order():
    dtype = np.float64
    fks = _models(3, dtype)
    limits, fmin = _limits(fks), _fmin(fks)
    pool = _candidates(300, 21, dtype)
    obj, cons = fks[0], fks[1:]
    full = gpr.constrained_ei(obj, cons, pool, fmin, limits, want_grad=True, want_details=True)
    again = gpr.constrained_ei(obj, cons, pool, fmin, limits, want_grad=True, want_details=True)
    assert _same(full, again)
    nograd = gpr.constrained_ei(obj, cons, pool, fmin, limits)
    assert nograd[0].tobytes() == full[0].tobytes() and nograd[1] == full[1]
    for j in (0, 17, 299):
        for want_grad in (False, True):
            alone = gpr.constrained_ei(obj, cons, pool[j:j + 1], fmin, limits, want_grad=want_grad)
            assert alone[0][0] == full[0][j] and alone[1] == 0
            if want_grad:
                assert alone[2].tobytes() == full[2][j].tobytes()
    moved = gpr.constrained_ei(obj, cons, np.vstack([pool[40:60], pool[17:18], pool[:5]]), fmin, limits, want_grad=True, want_details=True)
    assert moved[0][20] == full[0][17] and moved[2][20].tobytes() == full[2][17].tobytes()
    assert moved[3][20] == full[3][17] and moved[4][20] == full[4][17]
    assert moved[0][:20].tobytes() == full[0][40:60].tobytes()
    # the constraints in the opposite order: the same quantity by other products
    rev = gpr.constrained_ei(obj, cons[::-1], pool, fmin, limits[::-1], want_grad=True)
    _, mu, vr, dmu, dvr = _posteriors(fks, pool)
    scale = R.cei_grad_x(mu, vr, dmu, dvr, fmin, limits)[4]
    bar = R.value_bar(dtype, mu[:, 0], vr[:, 0], fmin)
    assert np.abs(rev[0] - full[0]).max() <= bar
    assert np.abs(rev[2] - full[2]).max() <= R.grad_bar(dtype, mu[:, 0], vr[:, 0], fmin, scale)
    # two threads on the same models in the same order: the same bits
    got = [None, None]

    def run_same(i):
        for _ in range(5):
            got[i] = gpr.constrained_ei(obj, cons, pool, fmin, limits, want_grad=True, want_details=True)

    def run_opposite(i):
        for _ in range(5):
            if i == 0:
                got[0] = gpr.constrained_ei(obj, cons, pool, fmin, limits, want_grad=True, want_details=True)
            else:
                got[1] = gpr.constrained_ei(obj, cons[::-1], pool, fmin, limits[::-1], want_grad=True)

    for target, what in ((run_same, "in the same order"), (run_opposite, "in opposite orders")):
        got[:] = [None, None]
        ts = [threading.Thread(target=target, args=(i,), daemon=True) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in ts), f"two concurrent cEI calls naming the constraints {what} did not return"
        assert _same(full, got[0])
        assert _same(full, got[1]) if target is run_same else _same(rev, got[1])
    for fk in fks:
        fk.release()


def test_clamped_variance_counts_as_sigma_zero():
    g = np.stack(np.meshgrid(np.linspace(0, 1, 8), np.linspace(0, 1, 8)), axis=-1).reshape(-1, 2)
    n_clamped = {}
    # a low-noise f64 model at its own training rows, and the f32 model of tests/test_gpu_predict_grad.py whose variances there are
    # rounding of size eps32 * c, far beyond 1e-5: about half of them come out negative and are clamped
    for dtype, scale, theta in ((np.float64, 1.0, np.log([1e-9, 1.0, 0.05, 0.05])), (np.float32, 100.0, np.log([1e-4, 1e4, 0.05, 0.05]))):
        X = g.astype(dtype)
        ys = [(np.sin(3 * g).sum(axis=1) * scale).astype(dtype), (np.cos(2 * g).sum(axis=1) * scale).astype(dtype),
              ((g ** 2).sum(axis=1) * scale).astype(dtype)]
        fks = [gpr.FittedKernel.extend(X, y, theta, nu=2.5) for y in ys]
        fmin, limits = 0.4 * scale, np.array([0.9, 0.8]) * scale
        for fm in (fmin, math.inf):
            val, best, grad, ei, pof, mean, var = gpr.constrained_ei(fks[0], fks[1:], X, fm, limits, want_grad=True, want_details=True)
            n_clamped[np.dtype(dtype).name] = int((var == 0).sum())
            assert np.isfinite(val).all() and np.isfinite(grad).all() and (val >= 0).all()
            _, mu, vr, dmu, dvr = _posteriors(fks, X)
            rv, rei, rpof, rg, sc = R.cei_grad_x(mu, vr, dmu, dvr, fm, limits)  # the restatement takes dsigma = 0 where sigma is 0
            bar = R.value_bar(dtype, mu[:, 0], vr[:, 0], fm)
            assert np.abs(val - rv).max() <= bar and np.abs(ei - rei).max() <= bar
            assert np.abs(pof - rpof).max() <= (1e-8 if dtype == np.float64 else 1e-4)
            assert np.abs(grad - rg).max() <= R.grad_bar(dtype, mu[:, 0], vr[:, 0], fm, sc)
            zero = var == 0
            assert (np.isin(pof[zero[:, 1:].all(axis=1)], (0.0, 1.0))).all()  # every sigma_k = 0: a product of indicators
        for fk in fks:
            fk.release()
    print(f"clamped variances among 3 x 64 rows: {n_clamped}")
    assert n_clamped["float32"] > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_row_and_no_rows(dtype):
    fks = _models(2, dtype)
    limits, fmin = _limits(fks), _fmin(fks)
    Xs = _candidates(40, 31, dtype)
    clean = gpr.constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True, want_details=True)
    bad = Xs.copy()
    bad[13, 2] = math.nan
    val, best, grad, ei, pof, _, _ = gpr.constrained_ei(fks[0], fks[1:], bad, fmin, limits, want_grad=True, want_details=True)
    keep = np.arange(40) != 13
    assert math.isnan(val[13]) and math.isnan(ei[13]) and math.isnan(pof[13]) and np.isnan(grad[13]).all()
    assert val[keep].tobytes() == clean[0][keep].tobytes() and grad[keep].tobytes() == clean[2][keep].tobytes()
    assert ei[keep].tobytes() == clean[3][keep].tobytes() and pof[keep].tobytes() == clean[4][keep].tobytes()
    assert best == R.argmax_last(np.where(keep, val, -1.0))
    # m = 0 is a no-op
    b = C.c_int(5)
    handles = (C.c_void_p * 2)(fks[1]._h, fks[2]._h)
    fn = getattr(_lib.load(), "hbegp_constrained_ei_" + ("f64" if dtype == np.float64 else "f32"))
    rc = fn(fks[0]._h, handles, 2, None, 0, fmin, _lib.dptr(limits), None, None, C.byref(b), None, None, None, None)
    assert rc == _lib.OK and b.value == -1
    val, best = gpr.constrained_ei(fks[0], fks[1:], np.zeros((0, D), dtype), fmin, limits)
    assert val.shape == (0,) and best == -1
    for fk in fks:
        fk.release()


def test_wrong_arguments_on_real_models():
    lib = _lib.load()
    fks = [_model(k, np.float64, n=60) for k in range(3)]
    f32 = _model(1, np.float32, n=60)
    d2 = _model(2, np.float64, d=2, n=60)
    limits, fmin = _limits(fks), _fmin(fks)
    Xs = _candidates(3, 1, np.float64)
    val, grad, ei, best = np.full(3, 7.0), np.full((3, D), 7.0), np.full(3, 7.0), C.c_int(5)

    def hs(*a):
        return (C.c_void_p * max(len(a), 1))(*[x._h if x is not None else None for x in a])

    def call(obj, cons, n_con=None, m=3, lim=limits, fm=fmin, fn=lib.hbegp_constrained_ei_f64, x=Xs, v=val):
        f32_call = x is not None and x.dtype == np.float32
        xp, gp = (_lib.fptr(x), None) if f32_call else (_lib.dptr(x), _lib.dptr(grad))
        return fn(obj._h if obj is not None else None, cons, len(cons) if n_con is None else n_con, xp, m, fm, _lib.dptr(lim), _lib.dptr(v),
                  gp, C.byref(best), _lib.dptr(ei), None, None, None)

    def einval(rc, what):
        assert rc == _lib.EINVAL and what in _lib.last_error() and _lib.last_error(), _lib.last_error()

    ok = hs(fks[1], fks[2])
    einval(call(None, ok), "NULL objective")
    einval(call(fks[0], ok, n_con=-1), "n_con must lie in [0, 8]")
    einval(call(fks[0], ok, n_con=9), "n_con must lie in [0, 8]")
    einval(call(fks[0], None, n_con=2), "constraints/limits is NULL")
    einval(call(fks[0], ok, lim=None), "constraints/limits is NULL")
    einval(call(fks[0], hs(fks[1], None)), "NULL model")
    einval(call(fks[0], hs(fks[1], fks[1])), "same model")
    einval(call(fks[0], hs(fks[1], fks[0])), "objective's model")
    einval(call(fks[0], hs(fks[1], d2)), "differ in d")
    einval(call(fks[0], hs(f32, fks[2])), "model 1 holds f32 data")
    einval(call(f32, ok), "model 0 holds f32 data")
    einval(call(fks[0], ok, fn=lib.hbegp_constrained_ei_f32, x=Xs.astype(np.float32)), "holds f64 data")
    for v in (math.nan, math.inf, -math.inf):
        lm = limits.copy()
        lm[1] = v
        einval(call(fks[0], ok, lim=lm), "non-finite limit")
    einval(call(fks[0], ok, fm=math.nan), "fmin_normalized")
    einval(call(fks[0], ok, fm=-math.inf), "fmin_normalized")
    einval(call(fks[0], ok, n_con=0, fm=math.inf), "nothing to compute")
    einval(call(fks[0], ok, m=-1), "m must be >= 0")
    einval(call(fks[0], ok, x=None), "Xs/cei is NULL")
    einval(call(fks[0], ok, v=None), "Xs/cei is NULL")
    # a refused call writes nothing
    assert (val == 7.0).all() and (grad == 7.0).all() and (ei == 7.0).all() and best.value == 5
    # a size that cannot fit is ENOMEM, counted before anything is taken (or read: Xs holds three rows)
    assert call(fks[0], ok, m=2 ** 31 - 1) == _lib.ENOMEM and "device memory" in _lib.last_error()
    assert (val == 7.0).all() and best.value == -1
    assert call(fks[0], ok) == _lib.OK and call(fks[0], ok, fm=math.inf) == _lib.OK and call(fks[0], ok, n_con=0) == _lib.OK
    # the maximiser: the same checks, then maximize_ei's own
    lo, hi = np.zeros(D), np.ones(D)
    st = np.full((2, D), 0.5)
    xo, vo = np.full((2, D), 7.0), np.full(2, 7.0)

    def mcall(obj, cons, n_con=None, S=2, starts=st, lo=lo, hi=hi, fm=fmin, lim=limits, maxeval=10):
        return lib.hbegp_maximize_constrained_ei_f64(obj._h if obj is not None else None, cons, len(cons) if n_con is None else n_con,
                                                     _lib.dptr(starts), S, _lib.dptr(lo), _lib.dptr(hi), fm, _lib.dptr(lim), maxeval,
                                                     _lib.dptr(xo), _lib.dptr(vo), None)

    einval(mcall(None, ok), "NULL objective")
    einval(mcall(fks[0], ok, n_con=9), "n_con must lie in [0, 8]")
    einval(mcall(fks[0], hs(fks[1], fks[1])), "same model")
    einval(mcall(fks[0], hs(fks[0], fks[2])), "objective's model")
    einval(mcall(fks[0], hs(fks[1], f32)), "holds f32 data")
    einval(mcall(fks[0], hs(fks[1], d2)), "differ in d")
    einval(mcall(fks[0], ok, lim=np.array([math.nan, 1.0])), "non-finite limit")
    einval(mcall(fks[0], ok, fm=math.nan), "fmin_normalized")
    einval(mcall(fks[0], ok, n_con=0, fm=math.inf), "nothing to compute")
    einval(mcall(fks[0], ok, S=0), "S must be >= 1")
    einval(mcall(fks[0], ok, maxeval=0), "maxeval must be >= 1")
    einval(mcall(fks[0], ok, starts=np.full((2, D), 1.5)), "outside the box")
    einval(mcall(fks[0], ok, lo=np.full(D, 2.0)), "lo[0] > hi[0]")
    assert (xo == 7.0).all() and (vo == 7.0).all()
    assert mcall(fks[0], ok) == _lib.OK
    for fk in fks + [f32, d2]:
        fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_maximiser(dtype):
    fks = _models(2, dtype)
    limits, fmin = _limits(fks), _fmin(fks)
    bounds = [(0.0, 1.0)] * D
    cand = np.random.default_rng(41).uniform(0, 1, (2000, D)).astype(dtype)
    for fm in (fmin, math.inf):
        cval, cbest = gpr.constrained_ei(fks[0], fks[1:], cand, fm, limits)
        order = np.argsort(cval, kind="stable")
        starts = np.vstack([cand[order[-3:]], cand[:3]])  # the three best of the random candidates and three arbitrary ones
        s_val, _ = gpr.constrained_ei(fks[0], fks[1:], starts, fm, limits)
        x, val, nevals = gpr.maximize_constrained_ei(fks[0], fks[1:], starts, bounds, fm, limits, maxeval=60)
        assert x.dtype == dtype and x.shape == (6, D) and (x >= 0).all() and (x <= 1).all()
        assert (val >= s_val).all(), (val, s_val)
        assert (nevals >= 1).all() and (nevals <= 60).all()
        again, _ = gpr.constrained_ei(fks[0], fks[1:], x, fm, limits)
        assert again.tobytes() == val.tobytes()
        # informational: no bar on it
        print(f"{np.dtype(dtype).name} fmin={fm:.3g}: starts {s_val}, maximised {val}, evaluations {nevals}, best run {val.max():.4e}, "
              f"best of 2000 random {cval[cbest]:.4e}")
    for fk in fks:
        fk.release()


def test_acquire_by_constrained_ei():
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 1, (120, 3))
    y = ((X - 0.3) ** 2).sum(axis=1) + 0.5 + 0.02 * rng.standard_normal(120) ** 2
    g1 = ((X - 0.7) ** 2).sum(axis=1) + 0.5 + 0.02 * rng.standard_normal(120) ** 2
    g2 = X.sum(axis=1) + 1.0 + 0.02 * rng.standard_normal(120) ** 2
    model, c1, c2 = (E.EstimatorGPR.new(3).estimate(X, t, None, E.RNG.new_with_seed(4 + i)) for i, t in enumerate((y, g1, g2)))
    limits = [float(np.median(g1)), float(np.quantile(g2, 0.7))]
    fmin = E.feasible_fmin(y, np.stack([g1, g2], axis=1), limits)
    assert math.isfinite(fmin)
    cand = np.random.default_rng(9).uniform(0, 1, (200, 3))
    val, best = E.constrained_ei_a(model, [c1, c2], cand, fmin, limits)
    assert best == R.argmax_last(val) and (val >= 0).all()
    idx, means, vals, fmins = E.acquire_by_constrained_ei(cand, model, [c1, c2], 3, limits, fmin=fmin)
    assert len(set(idx.tolist())) == 3 and idx[0] == best and vals[0] == val[best]
    assert means.shape == (3, 3) and np.isfinite(means).all()
    fn, _ = E._cei_normalized(model, [c1, c2], fmin, limits)
    print(f"picks {idx.tolist()}, cei {vals}, believed fmin {fn:.6f} -> {fmins}")
    assert fmins[0] <= fn and (np.diff(fmins) <= 0).all()  # the believed incumbent only falls
    # the default incumbent: feasible_fmin of the shared training rows (the targets projected back: fmin up to rounding)
    idx_d, _, vals_d, _ = E.acquire_by_constrained_ei(cand, model, [c1, c2], 2, limits)
    assert idx_d.tolist() == idx[:2].tolist() and np.allclose(vals_d, vals[:2], rtol=1e-6, atol=1e-12)
    # no feasible row: the search for feasibility, by the probability of feasibility
    tight = [float(g1.min()) - 1.0, float(g2.min()) - 1.0]
    assert E.feasible_fmin(y, np.stack([g1, g2], axis=1), tight) == math.inf
    pval, pbest = E.constrained_ei_a(model, [c1, c2], cand, math.inf, limits)
    idx_p, _, vals_p, fmins_p = E.acquire_by_constrained_ei(cand, model, [c1, c2], 2, limits, fmin=math.inf)
    assert idx_p[0] == pbest and vals_p[0] == pval[pbest] and ((pval >= 0) & (pval <= 1)).all() and len(set(idx_p.tolist())) == 2
    x, v, ne = E.maximize_constrained_ei(model, [c1, c2], cand[[best, 0]], [(0.0, 1.0)] * 3, fmin, limits, maxeval=30)
    assert v[0] >= val[best] and v[1] >= val[0] and (ne <= 30).all()
    other = E.EstimatorGPR.new(3).estimate(X[:100], g1[:100], None, E.RNG.new_with_seed(7))
    with pytest.raises(ValueError):
        E.acquire_by_constrained_ei(cand, model, [other, c2], 2, limits)
    idx_o, _, _, _ = E.acquire_by_constrained_ei(cand, model, [other, c2], 2, limits, fmin=fmin)  # with an incumbent it works
    assert len(set(idx_o.tolist())) == 2


def test_cpp_mirror_cei(tmp_path):
    exe = str(tmp_path / "test_cei")
    lib_dir = os.path.join(ROOT, "hbetune_rs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cei.cpp"),
                           "-L", lib_dir, "-lhbegp", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0 threw=1" in out.stdout


def test_debug_cei_phases():
    lib = _lib.load()
    fks = _models(2, np.float64)
    limits, fmin = _limits(fks), _fmin(fks)
    Xs = _candidates(300, 5, np.float64)
    ph = np.full(2, -1.0)
    assert lib.hbegp_debug_cei_phases(1, None) == _lib.OK
    timed = gpr.constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True)
    assert lib.hbegp_debug_cei_phases(0, _lib.dptr(ph)) == _lib.OK
    print(f"phases: the predicts {ph[0]:.3f} ms, the cEI kernel and the arg-max {ph[1]:.3f} ms")
    assert (ph > 0).all()
    untimed = gpr.constrained_ei(fks[0], fks[1:], Xs, fmin, limits, want_grad=True)
    assert _same(timed, untimed)  # timing changes no bit
    for fk in fks:
        fk.release()
