"""GPU: the two-objective expected hypervolume improvement (hbegp_ehvi_* / hbegp_maximize_ehvi_*).

The device's ehvi and grad replayed through the NumPy restatement (tests/ehvi_ref.py) on the engine's own predict_grad outputs of
the two models; best, mean and var against predict / predict_grad bit for bit; a front past the kernel's LDS capacity; bits across
batch sizes, positions, gradient on / off, threads and the models' order; clamped variances, NaN rows, m = 0, argument checks; the
maximiser; the estimator's acquire_by_ehvi; the C++ mirror.  (Models on different devices are refused too; one device cannot show it.)

Bars: 1e-8 (f64) / 1e-4 (f32) times max(1, H), H = (r1 - min a + sqrt(c1)) (r2 - min b + sqrt(c2)); for the gradient times
max(1, max |dmean|, max |dvar| / (2 sigma)) as well.  Measured deviations: DESIGN section 20."""
import ctypes as C
import math
import os
import subprocess
import threading

import numpy as np
import pytest

import ehvi_ref as R
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 4
# f32: a noise of the amplitude's size keeps cond(K) <= n + 1 (tests/test_gpu_kg.py)
F32_NOISE = 1.0
AMP = (1.3, 0.8)


def _model(n, nu, dtype, obj, seed=1, d=D):
    """tests/test_gpu_kg.py::_model with one of two response functions."""
    rng = np.random.default_rng(seed + 100 * obj)
    X = rng.uniform(0, 1, (n, d))
    if obj == 0:
        y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    else:
        y = ((X - 0.6) ** 2).sum(axis=1) * 3 - np.cos(4 * X[:, 0]) + 0.1 * rng.standard_normal(n)
    X, y = X.astype(dtype), y.astype(dtype)
    amp = AMP[obj]
    noise_over_amp = 1e-2 if dtype == np.float64 else F32_NOISE
    theta = np.log(np.concatenate([[noise_over_amp * amp, amp], np.linspace(0.3, 0.9, d) if obj == 0 else np.linspace(0.8, 0.4, d)]))
    return gpr.FittedKernel.extend(X, y, theta, nu=nu)


def _pair(dtype, nus=(1.5, 2.5), ns=(100, 300), seed=1, d=D):
    return [_model(ns[0], nus[0], dtype, 0, seed, d), _model(ns[1], nus[1], dtype, 1, seed, d)]


def _candidates(m, seed, dtype, d=D):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (m, d)).astype(dtype)


def _front(P, fks, seed=0):
    """(front [P + extras, 2], ref): a convex front a_i = i / P, b_i = (1 - sqrt(i / P))^2 scaled into the models' y ranges, shuffled,
    with a few dominated points, a duplicate and a point outside the box added (the library reduces them away)."""
    lo = np.array([float(fk.y_train.min()) for fk in fks])
    hi = np.array([float(fk.y_train.max()) for fk in fks])
    ref = hi + 0.1 * (hi - lo)
    if P == 0:
        return np.zeros((0, 2)), ref
    t = np.arange(P) / P
    f = np.stack([lo[0] + (hi[0] - lo[0]) * t, lo[1] + (hi[1] - lo[1]) * (1 - np.sqrt(t)) ** 2], axis=1)
    rng = np.random.default_rng(seed + P)
    extra = np.vstack([f[: min(P, 3)] + 0.01 * (hi - lo), f[:1], [[ref[0] + 1.0, lo[1]]]])
    f = np.vstack([f, extra])[rng.permutation(P + len(extra))]
    return f, ref


def _replay(fks, Xs, front, ref, dtype):
    """Device ehvi / grad against the restatement on the engine's own predict_grad outputs; best, mean, var bit for bit.  Returns
    (worst deviation of ehvi / its bar, of grad / its bar)."""
    m = len(Xs)
    val, best, grad, mean, var = gpr.ehvi(fks, Xs, front, ref, want_grad=True, want_posterior=True)
    assert val.dtype == np.float64 and val.shape == (m,) and grad.dtype == dtype and grad.shape == (m, D)
    pg = [fk.predict_with_gradient(Xs) for fk in fks]
    for k in range(2):
        assert mean[:, k].tobytes() == pg[k][0].tobytes() and var[:, k].tobytes() == pg[k][1].tobytes()
    mu = np.stack([pg[0][0], pg[1][0]], axis=1).astype(np.float64)
    vr = np.stack([pg[0][1], pg[1][1]], axis=1).astype(np.float64)
    dmu = np.stack([pg[0][2], pg[1][2]], axis=1).astype(np.float64)
    dvr = np.stack([pg[0][3], pg[1][3]], axis=1).astype(np.float64)
    rv, rg = R.ehvi_grad_x(mu, vr, dmu, dvr, front, ref)
    bar = R.bars(dtype, fks[0].amplitude, fks[1].amplitude, front, ref)
    sd = np.sqrt(vr)
    with np.errstate(all="ignore"):
        dsd = np.where(sd[:, :, None] > R.EPS, np.abs(dvr) / (2.0 * sd[:, :, None]), 0.0)
    gbar = bar * max(1.0, float(np.abs(dmu).max()), float(dsd.max()))
    dev = float(np.abs(val - rv).max())
    gdev = float(np.abs(grad.astype(np.float64) - rg).max())
    print(f"  m={m} P={len(front)}: ehvi max {val.max():.3e} deviation {dev:.1e} (bar {bar:.1e}), grad deviation {gdev:.1e} (bar {gbar:.1e})")
    assert dev <= bar, (m, len(front), dev, bar)
    assert gdev <= gbar, (m, len(front), gdev, gbar)
    assert (val >= 0.0).all()
    assert best == R.argmax_last(val)
    # without a gradient: the same bits, and the batched predict's posterior
    val2, best2, mean2, var2 = gpr.ehvi(fks, Xs, front, ref, want_posterior=True)
    assert val2.tobytes() == val.tobytes() and best2 == best
    assert mean2.tobytes() == mean.tobytes() and var2.tobytes() == var.tobytes()
    if m > 16:  # predict's batched path: the same launches
        for k in range(2):
            pm, pv, _ = fks[k].predict(Xs)
            assert mean2[:, k].tobytes() == pm.tobytes() and var2[:, k].tobytes() == pv.tobytes()
    return dev / bar, gdev / gbar


@pytest.mark.parametrize("nus", [(0.5, math.inf), (1.5, 2.5)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_ehvi_replays_through_the_restatement(dtype, nus):
    fks = _pair(dtype, nus)
    pool = _candidates(300, 11, dtype)
    worst = [0.0, 0.0]
    for P in (0, 1, 7, 200):
        front, ref = _front(P, fks)
        for m in (1, 40, 300):
            r = _replay(fks, pool[:m], front, ref, dtype)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"{np.dtype(dtype).name} nu={nus}: worst deviation / bar: ehvi {worst[0]:.1e}, grad {worst[1]:.1e}")
    for fk in fks:
        fk.release()


def test_replay_past_the_lds_capacity():
    fks = _pair(np.float64)
    front, ref = _front(5000, fks)  # 5001 strips: beyond the 4096 the kernel stages in the LDS
    assert len(R.reduce_front(front, ref)[0]) == 5000
    r = _replay(fks, _candidates(8, 6, np.float64), front, ref, np.float64)
    print(f"P=5000 m=8: deviation / bar: ehvi {r[0]:.1e}, grad {r[1]:.1e}")
    front, ref = _front(4095, fks)  # 4096 strips: the last size that is staged
    _replay(fks, _candidates(8, 6, np.float64), front, ref, np.float64)
    for fk in fks:
        fk.release()


def test_replay_at_n_1000_m_2000():
    fks = _pair(np.float64, ns=(1000, 1000), seed=3)
    front, ref = _front(64, fks)
    r = _replay(fks, _candidates(2000, 5, np.float64), front, ref, np.float64)
    print(f"n=1000/1000 m=2000 P=64: deviation / bar: ehvi {r[0]:.1e}, grad {r[1]:.1e}")
    for fk in fks:
        fk.release()


def test_bits_positions_gradient_threads_and_model_order():
    dtype = np.float64
    fks = _pair(dtype)
    front, ref = _front(7, fks)
    pool = _candidates(300, 21, dtype)
    full = gpr.ehvi(fks, pool, front, ref, want_grad=True, want_posterior=True)
    again = gpr.ehvi(fks, pool, front, ref, want_grad=True, want_posterior=True)

    def same(a, b):
        return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b))

    assert same(full, again)
    nograd = gpr.ehvi(fks, pool, front, ref)
    assert nograd[0].tobytes() == full[0].tobytes() and nograd[1] == full[1]
    for j in (0, 17, 299):
        for want_grad in (False, True):
            alone = gpr.ehvi(fks, pool[j:j + 1], front, ref, want_grad=want_grad)
            assert alone[0][0] == full[0][j] and alone[1] == 0
            if want_grad:
                assert alone[2].tobytes() == full[2][j].tobytes()
    moved = gpr.ehvi(fks, np.vstack([pool[40:60], pool[17:18], pool[:5]]), front, ref, want_grad=True)
    assert moved[0][20] == full[0][17] and moved[2][20].tobytes() == full[2][17].tobytes()
    assert moved[0][:20].tobytes() == full[0][40:60].tobytes()
    # the objectives exchanged through the transposed front: the same quantity by another sum (strips along the other objective)
    swapped = gpr.ehvi(fks[::-1], pool, front[:, ::-1], ref[::-1], want_grad=True)
    bar = R.bars(dtype, fks[0].amplitude, fks[1].amplitude, front, ref)
    assert np.abs(swapped[0] - full[0]).max() <= bar
    # two threads on the same pair at once, one of them naming the models in the other order: no deadlock, the same bits
    got = [None, None]

    def run(i):
        for _ in range(5):
            if i == 0:
                got[0] = gpr.ehvi(fks, pool, front, ref, want_grad=True, want_posterior=True)
            else:
                got[1] = gpr.ehvi(fks[::-1], pool, front[:, ::-1], ref[::-1], want_grad=True)

    ts = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "two concurrent EHVI calls on the same pair of models did not return"
    assert same(full, got[0]) and same(swapped, got[1])
    for fk in fks:
        fk.release()


def test_clamped_variance_counts_as_sigma_zero():
    g = np.stack(np.meshgrid(np.linspace(0, 1, 8), np.linspace(0, 1, 8)), axis=-1).reshape(-1, 2)
    n_clamped = {}
    # a low-noise f64 model at its own training rows, and the f32 model of tests/test_gpu_predict_grad.py whose variances there are
    # rounding of size eps32 * c, far beyond 1e-5: about half of them come out negative and are clamped
    for dtype, scale, theta in ((np.float64, 1.0, np.log([1e-9, 1.0, 0.05, 0.05])), (np.float32, 100.0, np.log([1e-4, 1e4, 0.05, 0.05]))):
        X = g.astype(dtype)
        ys = [(np.sin(3 * g).sum(axis=1) * scale).astype(dtype), (np.cos(2 * g).sum(axis=1) * scale).astype(dtype)]
        fks = [gpr.FittedKernel.extend(X, y, theta, nu=2.5) for y in ys]
        front = np.array([[-0.5, 0.5], [0.2, -0.3], [1.0, -1.0]]) * scale
        ref = np.array([1.5, 1.5]) * scale
        val, best, grad, mean, var = gpr.ehvi(fks, X, front, ref, want_grad=True, want_posterior=True)
        n_clamped[np.dtype(dtype).name] = int((var == 0).sum())
        assert np.isfinite(val).all() and np.isfinite(grad).all() and (val >= 0).all()
        pg = [fk.predict_with_gradient(X) for fk in fks]
        mu, vr, dmu, dvr = (np.stack([pg[0][i], pg[1][i]], axis=1).astype(np.float64) for i in range(4))
        rv, rg = R.ehvi_grad_x(mu, vr, dmu, dvr, front, ref)  # the restatement takes dsigma = 0 where sigma is 0
        bar = R.bars(dtype, fks[0].amplitude, fks[1].amplitude, front, ref)
        with np.errstate(all="ignore"):
            dsd = np.where(vr[:, :, None] > 0, np.abs(dvr) / (2.0 * np.sqrt(vr)[:, :, None]), 0.0)
        assert np.abs(val - rv).max() <= bar
        assert np.abs(grad - rg).max() <= bar * max(1.0, float(np.abs(dmu).max()), float(dsd.max()))
        for fk in fks:
            fk.release()
    print(f"clamped variances among 2 x 64 rows: {n_clamped}")
    assert n_clamped["float32"] > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_row_and_no_rows(dtype):
    fks = _pair(dtype)
    front, ref = _front(7, fks)
    Xs = _candidates(40, 31, dtype)
    clean = gpr.ehvi(fks, Xs, front, ref, want_grad=True)
    bad = Xs.copy()
    bad[13, 2] = math.nan
    val, best, grad = gpr.ehvi(fks, bad, front, ref, want_grad=True)
    keep = np.arange(40) != 13
    assert math.isnan(val[13]) and np.isnan(grad[13]).all()
    assert val[keep].tobytes() == clean[0][keep].tobytes() and grad[keep].tobytes() == clean[2][keep].tobytes()
    assert best == R.argmax_last(np.where(keep, val, -1.0))
    # m = 0 is a no-op
    b = C.c_int(5)
    handles = (C.c_void_p * 2)(fks[0]._h, fks[1]._h)
    fn = getattr(_lib.load(), "hbegp_ehvi_" + ("f64" if dtype == np.float64 else "f32"))
    assert fn(handles, 2, None, 0, _lib.dptr(front), len(front), _lib.dptr(ref), None, None, C.byref(b), None, None) == _lib.OK
    assert b.value == -1
    val, best = gpr.ehvi(fks, np.zeros((0, D), dtype), front, ref)
    assert val.shape == (0,) and best == -1
    for fk in fks:
        fk.release()


def test_wrong_arguments_on_real_models():
    lib = _lib.load()
    fks = _pair(np.float64, ns=(60, 80))
    f32 = _model(60, 2.5, np.float32, 0)
    d2 = _model(60, 2.5, np.float64, 1, d=2)
    front, ref = _front(7, fks)
    Xs = _candidates(3, 1, np.float64)
    val = np.zeros(3)

    def hs(a, b):
        return (C.c_void_p * 2)(a._h if a is not None else None, b._h if b is not None else None)

    def call(h, n_obj=2, m=3, fr=front, P=None, rf=ref, fn=lib.hbegp_ehvi_f64, x=Xs):
        xp = _lib.fptr(x) if x.dtype == np.float32 else _lib.dptr(x)
        return fn(h, n_obj, xp, m, _lib.dptr(fr), len(fr) if P is None else P, _lib.dptr(rf), _lib.dptr(val), None, None, None, None)

    def einval(rc, what):
        assert rc == _lib.EINVAL and what in _lib.last_error() and _lib.last_error(), _lib.last_error()

    ok = hs(fks[0], fks[1])
    einval(call(ok, n_obj=1), "n_obj must be 2")
    einval(call(ok, n_obj=3), "n_obj must be 2")
    einval(call(hs(fks[0], None)), "NULL model")
    einval(call(hs(None, fks[1])), "NULL model")
    einval(call(hs(fks[0], fks[0])), "same model")
    einval(call(hs(fks[0], d2)), "differ in d")
    einval(call(hs(fks[0], f32)), "model 1 holds f32 data")
    einval(call(hs(f32, fks[1])), "model 0 holds f32 data")
    einval(call(ok, fn=lib.hbegp_ehvi_f32, x=Xs.astype(np.float32)), "holds f64 data")
    einval(call(ok, m=-1), "m must be >= 0")
    einval(call(ok, P=-1), "P must be >= 0")
    for v in (math.nan, math.inf, -math.inf):
        fr = front.copy()
        fr[2, 1] = v
        einval(call(ok, fr=fr), "non-finite front")
        rf = ref.copy()
        rf[0] = v
        einval(call(ok, rf=rf), "non-finite reference")
    assert call(ok) == _lib.OK
    # a size that cannot fit is ENOMEM, counted before anything is taken (or read: Xs holds three rows)
    assert call(ok, m=2 ** 31 - 1) == _lib.ENOMEM and "device memory" in _lib.last_error()
    # the maximiser: the same checks, then maximize_ei's own
    lo, hi = np.zeros(D), np.ones(D)
    st = np.full((2, D), 0.5)
    xo, vo = np.zeros((2, D)), np.zeros(2)

    def mcall(h, n_obj=2, S=2, starts=st, lo=lo, hi=hi, rf=ref, maxeval=10):
        return lib.hbegp_maximize_ehvi_f64(h, n_obj, _lib.dptr(starts), S, _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(front), len(front),
                                           _lib.dptr(rf), maxeval, _lib.dptr(xo), _lib.dptr(vo), None)

    einval(mcall(ok, n_obj=1), "n_obj must be 2")
    einval(mcall(hs(fks[0], fks[0])), "same model")
    einval(mcall(hs(fks[0], f32)), "holds f32 data")
    einval(mcall(ok, rf=np.array([math.nan, 1.0])), "non-finite reference")
    einval(mcall(ok, S=0), "S must be >= 1")
    einval(mcall(ok, maxeval=0), "maxeval must be >= 1")
    einval(mcall(ok, starts=np.full((2, D), 1.5)), "outside the box")
    einval(mcall(ok, lo=np.full(D, 2.0)), "lo[0] > hi[0]")
    assert mcall(ok) == _lib.OK
    for fk in fks + [f32, d2]:
        fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_maximiser(dtype):
    fks = _pair(dtype)
    front, ref = _front(7, fks)
    bounds = [(0.0, 1.0)] * D
    cand = np.random.default_rng(41).uniform(0, 1, (2000, D)).astype(dtype)
    cval, cbest = gpr.ehvi(fks, cand, front, ref)
    order = np.argsort(cval, kind="stable")
    starts = np.vstack([cand[order[-3:]], cand[:3]])  # the three best of the random candidates and three arbitrary ones
    s_val, _ = gpr.ehvi(fks, starts, front, ref)
    x, val, nevals = gpr.maximize_ehvi(fks, starts, bounds, front, ref, maxeval=60)
    assert x.dtype == dtype and x.shape == (6, D) and (x >= 0).all() and (x <= 1).all()
    assert (val >= s_val).all(), (val, s_val)
    assert (nevals >= 1).all() and (nevals <= 60).all()
    again, _ = gpr.ehvi(fks, x, front, ref)
    assert again.tobytes() == val.tobytes()
    bar = R.bars(dtype, fks[0].amplitude, fks[1].amplitude, front, ref)
    print(f"{np.dtype(dtype).name}: starts {s_val}, maximised {val}, evaluations {nevals}, best of 2000 random {cval[cbest]:.4e}")
    assert val.max() >= cval[cbest] - bar
    for fk in fks:
        fk.release()


def test_acquire_by_ehvi():
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 1, (120, 3))
    y0 = ((X - 0.3) ** 2).sum(axis=1) + 0.5 + 0.02 * rng.standard_normal(120) ** 2
    y1 = ((X - 0.7) ** 2).sum(axis=1) + 0.5 + 0.02 * rng.standard_normal(120) ** 2
    models = [E.EstimatorGPR.new(3).estimate(X, y, None, E.RNG.new_with_seed(4 + i)) for i, y in enumerate((y0, y1))]
    cand = np.random.default_rng(9).uniform(0, 1, (200, 3))
    front = E.pareto_front(np.stack([y0, y1], axis=1))
    ref = E.default_reference_point(front)
    val, best = E.ehvi_a(models, cand, front, ref)
    assert best == R.argmax_last(val) and (val >= 0).all()
    idx, means, vals, hvs = E.acquire_by_ehvi(cand, models, 3, front=front, ref=ref)
    assert len(set(idx.tolist())) == 3 and idx[0] == best and vals[0] == val[best]
    assert means.shape == (3, 2) and np.isfinite(means).all()
    fn, rn = E._ehvi_normalized(models, front, ref)
    hv0 = E.hypervolume_2d(fn, rn)
    print(f"picks {idx.tolist()}, ehvi {vals}, believed hypervolume {hv0:.6f} -> {hvs}")
    assert hvs[0] >= hv0 and (np.diff(hvs) >= 0).all()
    # default front and reference point: the models share their training rows
    idx_d, _, vals_d, _ = E.acquire_by_ehvi(cand, models, 2)
    assert len(set(idx_d.tolist())) == 2 and (vals_d >= 0).all()
    x, v, ne = E.maximize_ehvi(models, cand[[best, 0]], [(0.0, 1.0)] * 3, front, ref, maxeval=30)
    assert v[0] >= val[best] and v[1] >= val[0] and (ne <= 30).all()
    other = E.EstimatorGPR.new(3).estimate(X[:100], y1[:100], None, E.RNG.new_with_seed(7))
    with pytest.raises(ValueError):
        E.acquire_by_ehvi(cand, [models[0], other], 2)
    idx_o, _, _, _ = E.acquire_by_ehvi(cand, [models[0], other], 2, front=front, ref=ref)  # with a front it works
    assert len(set(idx_o.tolist())) == 2


def test_cpp_mirror_ehvi(tmp_path):
    exe = str(tmp_path / "test_ehvi")
    lib_dir = os.path.join(ROOT, "hbetune_rs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_ehvi.cpp"),
                           "-L", lib_dir, "-lhbegp", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0 threw=1" in out.stdout
