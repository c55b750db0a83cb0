"""GPU: the expected hypervolume improvement of two to four objectives (hbegp_ehvi_nd_* / hbegp_maximize_ehvi_nd_*).

The device's ehvi and grad replayed through the NumPy restatement (tests/ehvi_nd_ref.py) on the engine's own predict_grad outputs of
the n_obj models; best, mean and var against predict / predict_grad bit for bit; the fronts at either side of the kernel's regime
boundaries; n_obj = 2 against gpr.ehvi; bits across batch sizes, positions, gradient on / off, threads and the models' order;
clamped variances, NaN rows, m = 0, argument checks; the maximiser; the estimator's acquire_by_ehvi_nd; one pool-hygiene subject;
the phase record; the C++ mirror.

Bars: 1e-8 (f64) / 1e-4 (f32) times max(1, H), H = prod_k (r_k - min a_k + sqrt(c_k)); for the gradient times
max(1, max |dmean|, max |dvar| / (2 sigma)) as well.  Measured deviations: DESIGN section 28."""
import ctypes as C
import math
import os
import subprocess
import threading

import numpy as np
import pytest

import ehvi_nd_ref as R
import test_gpu_pool_hygiene as PH
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 4
# f32: a noise of the amplitude's size keeps cond(K) <= n + 1 (tests/test_gpu_kg.py)
F32_NOISE = 1.0
AMP = (1.3, 0.8, 1.0, 0.6)
NS = (100, 300, 60, 200)
NUS = (0.5, 1.5, 2.5, math.inf)
LDS4, LDS1 = 682, 6826  # EHVI_ND_LDS4_ENTRIES, EHVI_ND_LDS1_ENTRIES of csrc/engine.hpp


def _model(n, nu, dtype, obj, seed=1, d=D):
    """tests/test_gpu_ehvi.py::_model with one of four response functions."""
    rng = np.random.default_rng(seed + 100 * obj)
    X = rng.uniform(0, 1, (n, d))
    if obj == 0:
        y = np.sin(3 * X).sum(axis=1)
    elif obj == 1:
        y = ((X - 0.6) ** 2).sum(axis=1) * 3 - np.cos(4 * X[:, 0])
    elif obj == 2:
        y = np.cos(2.5 * X).sum(axis=1) + X[:, 1]
    else:
        y = np.abs(X - 0.4).sum(axis=1) - 0.5 * np.sin(5 * X[:, d - 1])
    y = y + 0.1 * rng.standard_normal(n)
    X, y = X.astype(dtype), y.astype(dtype)
    amp = AMP[obj]
    noise_over_amp = 1e-2 if dtype == np.float64 else F32_NOISE
    scales = np.linspace(0.3, 0.9, d) if obj % 2 == 0 else np.linspace(0.8, 0.4, d)
    theta = np.log(np.concatenate([[noise_over_amp * amp, amp], scales]))
    return gpr.FittedKernel.extend(X, y, theta, nu=nu)


def _models(dtype, M, ns=NS, nus=NUS, seed=1, d=D):
    return [_model(ns[k], nus[k], dtype, k, seed, d) for k in range(M)]


def _release(fks):
    for fk in fks:
        fk.release()


def _amps(fks):
    return [fk.amplitude for fk in fks]


def _candidates(m, seed, dtype, d=D):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (m, d)).astype(dtype)


def _box(fks):
    lo = np.array([float(fk.y_train.min()) for fk in fks])
    hi = np.array([float(fk.y_train.max()) for fk in fks])
    return lo, hi, hi + 0.1 * (hi - lo)


def _shell(P, fks, seed=0):
    """(front [P, M], ref): P mutually non-dominated points -- the positive part of a sphere shell -- scaled into the models' y ranges."""
    lo, hi, ref = _box(fks)
    M = len(fks)
    if P == 0:
        return np.zeros((0, M)), ref
    x = np.abs(np.random.default_rng(seed + 10 * P + M).standard_normal((P, M))) + 0.05
    return lo + (hi - lo) * x / np.linalg.norm(x, axis=1, keepdims=True), ref


def _tie(f, at):
    """Two neighbours along objective 0 share that coordinate."""
    order = np.argsort(f[:, 0])
    f[order[at], 0] = f[order[at - 1], 0]


def _front(P, fks, seed=0):
    """The shell with a tied coordinate, shuffled, with a few dominated points, a duplicate and a point outside the box added (the
    library reduces them away)."""
    f, ref = _shell(P, fks, seed)
    if P == 0:
        return f, ref
    lo, hi, _ = _box(fks)
    if P >= 2:
        _tie(f, P // 2)
    out = f[0].copy()
    out[0] = ref[0] + 1.0
    extra = np.vstack([f[: min(P, 3)] + 0.01 * (hi - lo), f[:1], out[None]])
    return np.vstack([f, extra])[np.random.default_rng(seed + P).permutation(P + len(extra))], ref


def _line_front(P, fks):
    """Two objectives: P mutually non-dominated points with distinct coordinates -- 2 P + 4 thresholds, P + 1 boxes."""
    lo, hi, ref = _box(fks)
    t = np.arange(P) / P
    return np.stack([lo[0] + (hi[0] - lo[0]) * t, lo[1] + (hi[1] - lo[1]) * (1 - np.sqrt(t)) ** 2], axis=1), ref


def _posterior(fks, Xs):
    pg = [fk.predict_with_gradient(Xs) for fk in fks]
    return pg, tuple(np.stack([p[i] for p in pg], axis=1).astype(np.float64) for i in range(4))


def _replay(fks, Xs, front, ref, dtype, dec=None):
    """Device ehvi / grad against the restatement on the engine's own predict_grad outputs; best, mean, var bit for bit.  Returns
    (worst deviation of ehvi / its bar, of grad / its bar)."""
    m, M = len(Xs), len(fks)
    val, best, grad, mean, var = gpr.ehvi_nd(fks, Xs, front, ref, want_grad=True, want_posterior=True)
    assert val.dtype == np.float64 and val.shape == (m,) and grad.dtype == dtype and grad.shape == (m, Xs.shape[1])
    assert mean.shape == (m, M) and var.shape == (m, M)
    pg, (mu, vr, dmu, dvr) = _posterior(fks, Xs)
    for k in range(M):
        assert mean[:, k].tobytes() == pg[k][0].tobytes() and var[:, k].tobytes() == pg[k][1].tobytes()
    rv, rg = R.ehvi_grad_x(mu, vr, dmu, dvr, front, ref, dec)
    bar = R.bars(dtype, _amps(fks), front, ref)
    sd = np.sqrt(vr)
    with np.errstate(all="ignore"):
        dsd = np.where(sd[:, :, None] > R.EPS, np.abs(dvr) / (2.0 * sd[:, :, None]), 0.0)
    gbar = bar * max(1.0, float(np.abs(dmu).max()), float(dsd.max()))
    dev = float(np.abs(val - rv).max())
    gdev = float(np.abs(grad.astype(np.float64) - rg).max())
    print(f"  n_obj={M} m={m} P={len(front)}: ehvi max {val.max():.3e} deviation {dev:.1e} (bar {bar:.1e}), grad deviation {gdev:.1e} "
          f"(bar {gbar:.1e})")
    assert dev <= bar, (M, m, len(front), dev, bar)
    assert gdev <= gbar, (M, m, len(front), gdev, gbar)
    assert (val >= 0.0).all()
    assert best == R.argmax_last(val)
    # without a gradient: the same bits, and the batched predict's posterior
    val2, best2, mean2, var2 = gpr.ehvi_nd(fks, Xs, front, ref, want_posterior=True)
    assert val2.tobytes() == val.tobytes() and best2 == best
    assert mean2.tobytes() == mean.tobytes() and var2.tobytes() == var.tobytes()
    if m > 16:  # predict's batched path: the same launches
        for k in range(M):
            pm, pv, _ = fks[k].predict(Xs)
            assert mean2[:, k].tobytes() == pm.tobytes() and var2[:, k].tobytes() == pv.tobytes()
    return dev / bar, gdev / gbar


@pytest.mark.parametrize("M", [2, 3, 4])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_ehvi_nd_replays_through_the_restatement(dtype, M):
    fks = _models(dtype, M)
    pool = _candidates(70, 11, dtype)
    worst = [0.0, 0.0]
    for P in (0, 1, 7, 40):
        front, ref = _front(P, fks)
        dec = R.boxes(front, ref)
        nb = len(dec[1])
        if M == 3 and P == 7:
            assert nb < 64
        if M == 3 and P == 40:
            assert nb > 128 and nb % 64 != 0
        print(f" n_obj={M} P={P}: {nb} boxes over {sum(len(t) for t in dec[0])} thresholds")
        for m in (1, 5, 70):
            r = _replay(fks, pool[:m], front, ref, dtype, dec)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"{np.dtype(dtype).name} n_obj={M}: worst deviation / bar: ehvi {worst[0]:.1e}, grad {worst[1]:.1e}")
    _release(fks)


def _entries(front, ref):
    return sum(len(t) for t in R.boxes(front, ref)[0])


@pytest.mark.parametrize("P,nt", [(339, LDS4), (340, LDS4 + 2), (3411, LDS1), (3412, LDS1 + 2)])
def test_replay_at_the_regime_boundaries_with_two_objectives(P, nt):
    """The table of a candidate holds 2 P + 4 entries with two objectives: 682 is the last size with four candidates per workgroup,
    684 the first with one; 6826 the last in the LDS, 6828 the first in global scratch."""
    fks = _models(np.float64, 2)
    front, ref = _line_front(P, fks)
    assert _entries(front, ref) == nt
    r = _replay(fks, _candidates(8, 6, np.float64), front, ref, np.float64)
    print(f"P={P} ({nt} entries) m=8: deviation / bar: ehvi {r[0]:.1e}, grad {r[1]:.1e}")
    _release(fks)


@pytest.mark.parametrize("ties,nt", [(2, LDS4), (1, LDS4 + 1)])
def test_replay_at_the_first_regime_boundary_with_three_objectives(ties, nt):
    """226 points give 3 x 226 + 6 = 684 entries; every tied coordinate takes one away: exactly 682 and 683."""
    fks = _models(np.float64, 3)
    front, ref = _shell(226, fks)
    for t in range(ties):
        _tie(front, 50 + 60 * t)
    assert len(R.reduce_front(front, ref)) == 226 and _entries(front, ref) == nt
    r = _replay(fks, _candidates(8, 6, np.float64), front, ref, np.float64)
    print(f"n_obj=3 P=226 ({nt} entries) m=8: deviation / bar: ehvi {r[0]:.1e}, grad {r[1]:.1e}")
    _release(fks)


def test_two_objectives_agree_with_the_strip_kernel():
    for dtype in (np.float64, np.float32):
        fks = _models(dtype, 2)
        Xs = _candidates(70, 13, dtype)
        for P in (0, 7, 40):
            front, ref = _front(P, fks)
            a = gpr.ehvi(fks, Xs, front, ref, want_grad=True, want_posterior=True)
            b = gpr.ehvi_nd(fks, Xs, front, ref, want_grad=True, want_posterior=True)
            bar = R.bars(dtype, _amps(fks), front, ref)
            _, (mu, vr, dmu, dvr) = _posterior(fks, Xs)
            with np.errstate(all="ignore"):
                dsd = np.where(vr[:, :, None] > 0, np.abs(dvr) / (2.0 * np.sqrt(vr)[:, :, None]), 0.0)
            gbar = bar * max(1.0, float(np.abs(dmu).max()), float(dsd.max()))
            dev, gdev = np.abs(a[0] - b[0]).max(), np.abs(a[2].astype(np.float64) - b[2].astype(np.float64)).max()
            print(f"{np.dtype(dtype).name} P={P}: boxes against strips: ehvi {dev:.1e} (bar {bar:.1e}), grad {gdev:.1e} (bar {gbar:.1e})")
            assert dev <= bar and gdev <= gbar
            assert a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes()
        _release(fks)


def _same(a, b):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b))


def test_bits_positions_gradient_threads_and_model_order():
    dtype = np.float64
    fks = _models(dtype, 3)
    front, ref = _front(7, fks)
    pool = _candidates(70, 21, dtype)
    full = gpr.ehvi_nd(fks, pool, front, ref, want_grad=True, want_posterior=True)
    again = gpr.ehvi_nd(fks, pool, front, ref, want_grad=True, want_posterior=True)
    assert _same(full, again)
    nograd = gpr.ehvi_nd(fks, pool, front, ref)
    assert nograd[0].tobytes() == full[0].tobytes() and nograd[1] == full[1]
    for j in (0, 17, 69):
        for want_grad in (False, True):
            alone = gpr.ehvi_nd(fks, pool[j:j + 1], front, ref, want_grad=want_grad)
            assert alone[0][0] == full[0][j] and alone[1] == 0
            if want_grad:
                assert alone[2].tobytes() == full[2][j].tobytes()
    moved = gpr.ehvi_nd(fks, np.vstack([pool[40:60], pool[17:18], pool[:5]]), front, ref, want_grad=True)
    assert moved[0][20] == full[0][17] and moved[2][20].tobytes() == full[2][17].tobytes()
    assert moved[0][:20].tobytes() == full[0][40:60].tobytes()
    # the objectives permuted together with the front's columns: the same quantity by another sweep
    perm = [2, 0, 1]
    pfks, pfront, pref = [fks[k] for k in perm], np.ascontiguousarray(front[:, perm]), ref[perm]
    swapped = gpr.ehvi_nd(pfks, pool, pfront, pref, want_grad=True)
    bar = R.bars(dtype, _amps(fks), front, ref)
    assert np.abs(swapped[0] - full[0]).max() <= bar
    # two threads on the same models at once, naming them in different orders: no deadlock, each the bits of its own solo run
    got = [None, None]

    def run(i):
        for _ in range(5):
            if i == 0:
                got[0] = gpr.ehvi_nd(fks, pool, front, ref, want_grad=True, want_posterior=True)
            else:
                got[1] = gpr.ehvi_nd(pfks, pool, pfront, pref, want_grad=True)

    ts = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "two concurrent calls on the same models did not return"
    assert _same(full, got[0]) and _same(swapped, got[1])
    _release(fks)


def test_clamped_variance_counts_as_sigma_zero():
    """The f32 amplitude-1e4 model of tests/test_gpu_predict_grad.py at its own training rows: variances that are rounding of size
    eps32 * c, about half of them clamped at 0."""
    g = np.stack(np.meshgrid(np.linspace(0, 1, 8), np.linspace(0, 1, 8)), axis=-1).reshape(-1, 2)
    dtype, scale, theta = np.float32, 100.0, np.log([1e-4, 1e4, 0.05, 0.05])
    X = g.astype(dtype)
    ys = [(np.sin(3 * g).sum(axis=1) * scale).astype(dtype), (np.cos(2 * g).sum(axis=1) * scale).astype(dtype),
          (np.sin(2 * g[:, 0] - g[:, 1]) * scale).astype(dtype)]
    fks = [gpr.FittedKernel.extend(X, y, theta, nu=2.5) for y in ys]
    front = np.array([[-0.5, 0.5, 0.2], [0.2, -0.3, 0.6], [1.0, -1.0, -0.5], [0.3, 0.3, -0.8]]) * scale
    ref = np.array([1.5, 1.5, 1.2]) * scale
    val, best, grad, mean, var = gpr.ehvi_nd(fks, X, front, ref, want_grad=True, want_posterior=True)
    n_clamped = int((var == 0).sum())
    assert np.isfinite(val).all() and np.isfinite(grad).all() and (val >= 0).all()
    _, (mu, vr, dmu, dvr) = _posterior(fks, X)
    rv, rg = R.ehvi_grad_x(mu, vr, dmu, dvr, front, ref)  # the restatement takes dsigma = 0 where sigma is 0
    bar = R.bars(dtype, _amps(fks), front, ref)
    with np.errstate(all="ignore"):
        dsd = np.where(vr[:, :, None] > 0, np.abs(dvr) / (2.0 * np.sqrt(vr)[:, :, None]), 0.0)
    gbar = bar * max(1.0, float(np.abs(dmu).max()), float(dsd.max()))
    print(f"clamped variances among 3 x 64 rows: {n_clamped}; deviation {np.abs(val - rv).max():.1e} (bar {bar:.1e}), "
          f"grad {np.abs(grad - rg).max():.1e} (bar {gbar:.1e})")
    assert np.abs(val - rv).max() <= bar
    assert np.abs(grad - rg).max() <= gbar
    assert n_clamped > 0
    _release(fks)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_row_and_no_rows(dtype):
    fks = _models(dtype, 3)
    front, ref = _front(7, fks)
    Xs = _candidates(40, 31, dtype)
    clean = gpr.ehvi_nd(fks, Xs, front, ref, want_grad=True)
    bad = Xs.copy()
    bad[13, 2] = math.nan
    val, best, grad = gpr.ehvi_nd(fks, bad, front, ref, want_grad=True)
    keep = np.arange(40) != 13
    assert math.isnan(val[13]) and np.isnan(grad[13]).all()
    assert val[keep].tobytes() == clean[0][keep].tobytes() and grad[keep].tobytes() == clean[2][keep].tobytes()
    assert best == R.argmax_last(np.where(keep, val, -1.0))
    # m = 0 is a no-op
    b = C.c_int(5)
    handles = (C.c_void_p * 3)(*[fk._h for fk in fks])
    fn = getattr(_lib.load(), "hbegp_ehvi_nd_" + ("f64" if dtype == np.float64 else "f32"))
    assert fn(handles, 3, None, 0, _lib.dptr(front), len(front), _lib.dptr(ref), None, None, C.byref(b), None, None) == _lib.OK
    assert b.value == -1
    val, best = gpr.ehvi_nd(fks, np.zeros((0, D), dtype), front, ref)
    assert val.shape == (0,) and best == -1
    _release(fks)


def test_wrong_arguments_on_real_models():
    lib = _lib.load()
    fks = _models(np.float64, 3, ns=(60, 80, 70))
    f32 = _model(60, 2.5, np.float32, 0)
    d2 = _model(60, 2.5, np.float64, 1, d=2)
    front, ref = _front(7, fks)
    Xs = _candidates(3, 1, np.float64)
    val = np.zeros(3)

    def hs(*ms):
        return (C.c_void_p * 4)(*[m._h if m is not None else None for m in ms])

    def call(h, n_obj=3, m=3, fr=front, P=None, rf=ref, fn=lib.hbegp_ehvi_nd_f64, x=Xs, v=val):
        xp = None if x is None else (_lib.fptr(x) if x.dtype == np.float32 else _lib.dptr(x))
        return fn(h, n_obj, xp, m, None if fr is None else _lib.dptr(fr), len(front) if P is None else P,
                  None if rf is None else _lib.dptr(rf), None if v is None else _lib.dptr(v), None, None, None, None)

    def einval(rc, what):
        assert rc == _lib.EINVAL and what in _lib.last_error() and _lib.last_error(), _lib.last_error()

    ok = hs(*fks)
    einval(call(ok, n_obj=1), "n_obj must be 2, 3 or 4")
    einval(call(ok, n_obj=5), "n_obj must be 2, 3 or 4")
    einval(call(hs(fks[0], None, fks[2])), "NULL model")
    einval(call(hs(fks[0], fks[1], None)), "NULL model")
    einval(call(None), "models is NULL")
    einval(call(hs(fks[0], fks[1], fks[0])), "same model")
    einval(call(hs(fks[0], fks[1], fks[1])), "same model")
    einval(call(hs(fks[0], fks[1], d2)), "differ in d")
    einval(call(hs(fks[0], fks[1], f32)), "model 2 holds f32 data")
    einval(call(hs(f32, fks[1], fks[2])), "model 0 holds f32 data")
    einval(call(ok, fn=lib.hbegp_ehvi_nd_f32, x=Xs.astype(np.float32)), "holds f64 data")
    einval(call(ok, m=-1), "m must be >= 0")
    einval(call(ok, P=-1), "P must be >= 0")
    einval(call(ok, rf=None), "ref is NULL")
    einval(call(ok, fr=None), "front is NULL")
    einval(call(ok, x=None), "Xs/ehvi is NULL")
    einval(call(ok, v=None), "Xs/ehvi is NULL")
    for v in (math.nan, math.inf, -math.inf):
        fr = front.copy()
        fr[2, 1] = v
        einval(call(ok, fr=fr), "non-finite front")
        rf = ref.copy()
        rf[0] = v
        einval(call(ok, rf=rf), "non-finite reference")
    assert call(ok) == _lib.OK
    # two of the three models are a valid call with two objectives (the front's rows then hold two values)
    assert call(ok, n_obj=2, P=5) == _lib.OK
    # a size that cannot fit is ENOMEM, counted before anything is taken (or read: Xs holds three rows)
    assert call(ok, m=2 ** 31 - 1) == _lib.ENOMEM and "device memory" in _lib.last_error()
    # the maximiser: the same checks, then maximize_ei's own
    lo, hi = np.zeros(D), np.ones(D)
    st = np.full((2, D), 0.5)
    xo, vo = np.zeros((2, D)), np.zeros(2)

    def mcall(h, n_obj=3, S=2, starts=st, lo=lo, hi=hi, rf=ref, maxeval=10):
        return lib.hbegp_maximize_ehvi_nd_f64(h, n_obj, _lib.dptr(starts), S, _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(front), len(front),
                                              _lib.dptr(rf), maxeval, _lib.dptr(xo), _lib.dptr(vo), None)

    einval(mcall(ok, n_obj=1), "n_obj must be 2, 3 or 4")
    einval(mcall(hs(fks[0], fks[1], fks[0])), "same model")
    einval(mcall(hs(fks[0], fks[1], f32)), "holds f32 data")
    einval(mcall(ok, rf=np.array([math.nan, 1.0, 1.0])), "non-finite reference")
    einval(mcall(ok, S=0), "S must be >= 1")
    einval(mcall(ok, maxeval=0), "maxeval must be >= 1")
    einval(mcall(ok, starts=np.full((2, D), 1.5)), "outside the box")
    einval(mcall(ok, lo=np.full(D, 2.0)), "lo[0] > hi[0]")
    assert mcall(ok) == _lib.OK
    _release(fks + [f32, d2])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_maximiser(dtype):
    fks = _models(dtype, 3)
    front, ref = _front(7, fks)
    bounds = [(0.0, 1.0)] * D
    cand = np.random.default_rng(41).uniform(0, 1, (2000, D)).astype(dtype)
    cval, cbest = gpr.ehvi_nd(fks, cand, front, ref)
    order = np.argsort(cval, kind="stable")
    starts = np.vstack([cand[order[-3:]], cand[:3]])  # the three best of the random candidates and three arbitrary ones
    s_val, _ = gpr.ehvi_nd(fks, starts, front, ref)
    x, val, nevals = gpr.maximize_ehvi_nd(fks, starts, bounds, front, ref, maxeval=30)
    assert x.dtype == dtype and x.shape == (6, D) and (x >= 0).all() and (x <= 1).all()
    assert (val >= s_val).all(), (val, s_val)
    assert (nevals >= 1).all() and (nevals <= 30).all()
    again, _ = gpr.ehvi_nd(fks, x, front, ref)
    assert again.tobytes() == val.tobytes()
    print(f"{np.dtype(dtype).name}: starts {s_val}, maximised {val}, evaluations {nevals}, best of 2000 random {cval[cbest]:.4e}")
    _release(fks)


def test_acquire_by_ehvi_nd():
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 1, (80, 3))
    ys = [((X - c) ** 2).sum(axis=1) + 0.5 + 0.02 * rng.standard_normal(80) ** 2 for c in (0.3, 0.7, np.array([0.2, 0.8, 0.5]))]
    models = [E.EstimatorGPR.new(3).estimate(X, y, None, E.RNG.new_with_seed(4 + i)) for i, y in enumerate(ys)]
    handles = [mo.fitted for mo in models]
    cand = np.random.default_rng(9).uniform(0, 1, (60, 3))
    front = E.pareto_front_nd(np.stack(ys, axis=1))
    ref = E.default_reference_point_nd(front)
    val, best = E.ehvi_nd_a(models, cand, front, ref)
    assert best == R.argmax_last(val) and (val >= 0).all()
    idx, means, vals, hvs = E.acquire_by_ehvi_nd(cand, models, 3, front=front, ref=ref)
    assert len(set(idx.tolist())) == 3 and idx[0] == best and vals[0] == val[best]
    assert means.shape == (3, 3) and np.isfinite(means).all()
    fn, rn = E._ehvi_nd_normalized(models, front, ref)
    hv0 = E.hypervolume_nd(fn, rn)
    print(f"picks {idx.tolist()}, ehvi {vals}, believed hypervolume {hv0:.6f} -> {hvs}")
    assert hvs[0] >= hv0 and (np.diff(hvs) >= 0).all()
    # the models' own handles survive the call
    assert all(mo.fitted is h for mo, h in zip(models, handles))
    val2, best2 = E.ehvi_nd_a(models, cand, front, ref)
    assert val2.tobytes() == val.tobytes() and best2 == best
    # default front and reference point: the models share their training rows
    idx_d, _, vals_d, _ = E.acquire_by_ehvi_nd(cand, models, 2)
    assert len(set(idx_d.tolist())) == 2 and (vals_d >= 0).all()
    x, v, ne = E.maximize_ehvi_nd(models, cand[[best, 0]], [(0.0, 1.0)] * 3, front, ref, maxeval=20)
    assert v[0] >= val[best] and v[1] >= val[0] and (ne <= 20).all()


def _q_ehvi_nd(fk, case, m, dtype):
    others = [PH._model(case, dtype, k=1), PH._model(case, dtype, k=2)]
    fks = [fk] + others
    front, ref = _shell(6, fks)
    out = list(gpr.ehvi_nd(fks, PH._candidates(m, fk.d, 27 + m, dtype), front, ref, want_grad=True, want_posterior=True))
    _release(others)
    return out


@pytest.mark.parametrize("dtype", PH.DTYPES, ids=PH._id)
def test_ehvi_nd_ignores_what_its_blocks_held(dtype):
    case = PH.CASES[1]
    PH._check(lambda: PH._on_model(_q_ehvi_nd, case, 70, dtype), 15, 6 * PH._mat_bytes(case[0], dtype))


def test_phase_record():
    lib = _lib.load()
    ph = np.full(5, -1.0)
    for M in (4, 2, 3):  # fewer objectives after more: nothing of the earlier record stays
        fks = _models(np.float64, M)
        front, ref = _front(7, fks)
        Xs = _candidates(70, 5, np.float64)
        assert lib.hbegp_debug_ehvi_nd_phases(1, None) == _lib.OK
        gpr.ehvi_nd(fks, Xs, front, ref, want_grad=True)
        assert lib.hbegp_debug_ehvi_nd_phases(0, _lib.dptr(ph)) == _lib.OK
        print(f"n_obj={M}: phases (ms) {ph}")
        assert (ph[: M + 1] > 0).all() and (ph[M + 1:] == 0).all()
        before = ph.copy()
        gpr.ehvi_nd(fks, Xs, front, ref)  # untimed: the record stays as it was
        assert lib.hbegp_debug_ehvi_nd_phases(0, _lib.dptr(ph)) == _lib.OK
        assert ph.tobytes() == before.tobytes()
        _release(fks)


def test_cpp_mirror_ehvi_nd(tmp_path):
    exe = str(tmp_path / "test_ehvi_nd")
    lib_dir = os.path.join(ROOT, "hbetune_rs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_ehvi_nd.cpp"),
                           "-L", lib_dir, "-lhbegp", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0 threw=1" in out.stdout
