"""GPU: greedy batch selection by expected improvement with fantasised observations (hbegp_select_batch_*).

The device's picks replayed through the NumPy restatement (tests/batch_select_ref.py) on the engine's own Sigma and mean; the
meaning of the state after t picks, checked against predict on the model extended with the fantasies; k = 1 against the host
argmax of EI; bits, prefixes and threads; edge cases and argument checks; the estimator's select_batch_a."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import batch_select_ref as BS
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

NUS = [0.5, 1.5, 2.5, math.inf]
D = 4
# f32: a noise of the amplitude's size keeps cond(K) <= n + 1 (tests/test_gpu_posterior_cov.py)
F32_NOISE = 1.0


def _model(n, nu, dtype, seed=1, d=D):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    X, y = X.astype(dtype), y.astype(dtype)
    amp = 1.3
    noise_over_amp = 1e-2 if dtype == np.float64 else F32_NOISE
    theta = np.log(np.concatenate([[noise_over_amp * amp, amp], np.linspace(0.3, 0.9, d)]))
    fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    cond_bound = (n * fk.amplitude + fk.noise) / fk.noise
    return fk, X, y, cond_bound


def _candidates(m, seed, dtype, d=D):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (m, d)).astype(dtype)


def _fmin_lie(y, lie):
    fmin = float(np.min(y))
    return fmin, (None if not lie else float(np.median(y)))


_bars = BS.bars
_replay = BS.replay


@pytest.mark.parametrize("lie", [False, True])
@pytest.mark.parametrize("n", [100, 300, 1000])
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_picks_replay_through_the_restatement(dtype, nu, n, lie):
    fk, X, y, cond_bound = _model(n, nu, dtype, seed=n)
    assert cond_bound <= (5e5 if dtype == np.float64 else 4.2e3)
    fmin, L = _fmin_lie(y, lie)
    pool = _candidates(300, 11 + n, dtype)
    worst = np.zeros(4)
    for m in (1, 40, 300):
        for k in sorted({1, 5, min(32, m)}):
            if k > m:
                continue
            *_, devs = _replay(fk, pool[:m], k, fmin, L, dtype)
            worst = np.maximum(worst, devs)
    print(f"{np.dtype(dtype).name} nu={nu} n={n} lie={lie}: pick gap {worst[0]:.1e} ei {worst[1]:.1e} mean {worst[2]:.1e} "
          f"var {worst[3]:.1e} (cond(K) <= {cond_bound:.1e})")
    fk.release()


@pytest.mark.parametrize("lie", [False, True])
def test_replay_at_n_4096_m_2000_k_64(lie):
    fk, X, y, _ = _model(4096, 2.5, np.float64, seed=3)
    fmin, L = _fmin_lie(y, lie)
    *_, devs = _replay(fk, _candidates(2000, 5, np.float64), 64, fmin, L, np.float64)
    print(f"n=4096 m=2000 k=64 lie={lie}: pick gap {devs[0]:.1e} ei {devs[1]:.1e} mean {devs[2]:.1e} var {devs[3]:.1e}")
    fk.release()


@pytest.mark.parametrize("lie", [False, True])
@pytest.mark.parametrize("nu", [0.5, 2.5])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_state_after_t_picks_is_predict_of_the_extended_model(dtype, nu, lie):
    fk, X, y, _ = _model(300, nu, dtype, seed=21)
    fmin, L = _fmin_lie(y, lie)
    Xs = _candidates(40, 22, dtype)
    _, bar = _bars(dtype)
    c = fk.amplitude
    mean0, _, _ = fk.predict(Xs, want_variance=False)
    for t in (1, 3, 8):
        idx, _, mean, var = fk.select_batch(Xs, t, fmin, lie=L)
        fant = mean0[idx] if L is None else np.full(t, L)
        ext = fk.extend_with(np.vstack([X, Xs[idx]]), np.concatenate([y, fant]).astype(dtype))
        em, ev, _ = ext.predict(Xs)
        dm = float(np.abs(mean.astype(np.float64) - em).max()) / max(1.0, float(np.abs(em).max()))
        dv = float(np.abs(var.astype(np.float64) - ev).max()) / c
        print(f"{np.dtype(dtype).name} nu={nu} lie={lie} t={t}: mean {dm:.1e} var {dv:.1e} vs the extended model")
        assert dm <= bar and dv <= bar, (t, dm, dv)
        ext.release()
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_k1_is_the_host_argmax_of_ei(dtype):
    checked = 0
    for seed in range(6):
        fk, X, y, _ = _model(300, NUS[seed % 4], dtype, seed=40 + seed)
        Xs = _candidates(200, 50 + seed, dtype)
        fmin = float(np.min(y))
        mean, var, _ = fk.predict(Xs)
        e = np.array([E.expected_improvement(float(a), math.sqrt(float(b)), fmin) for a, b in zip(mean, var)])
        top = np.sort(e)[-2:]
        idx, ei, _, _ = fk.select_batch(Xs, 1, fmin)
        if top[1] - top[0] > 1e-9 * max(1.0, top[1]):
            assert idx[0] == len(e) - 1 - int(np.argmax(e[::-1])), (seed, idx, top)
            checked += 1
        fk.release()
    assert checked >= 4


def test_bits_prefixes_and_threads():
    fk, X, y, _ = _model(700, 2.5, np.float64, seed=8)
    fmin = float(np.min(y))
    Xs = [_candidates(50 + 100 * i, 60 + i, np.float64) for i in range(4)]
    lies = [None, float(np.median(y)), None, fmin - 0.2]
    solo = [fk.select_batch(x, 32, fmin, lie=L) for x, L in zip(Xs, lies)]
    again = [fk.select_batch(x, 32, fmin, lie=L) for x, L in zip(Xs, lies)]
    for a, b in zip(solo, again):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    for t in (1, 7, 20):
        idx, ei, _, _ = fk.select_batch(Xs[1], t, fmin, lie=lies[1])
        assert idx.tobytes() == solo[1][0][:t].tobytes() and ei.tobytes() == solo[1][1][:t].tobytes(), t
    # 4 threads on one model, then 4 threads on 4 models
    got = [None] * 4

    def run(i, model):
        for _ in range(3):
            got[i] = model.select_batch(Xs[i], 32, fmin, lie=lies[i])

    ts = [threading.Thread(target=run, args=(i, fk)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i in range(4):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(solo[i], got[i])), i
    models = [gpr.FittedKernel.extend(X, y, fk.theta, nu=2.5) for _ in range(4)]
    ref = [mdl.select_batch(Xs[i], 32, fmin, lie=lies[i]) for i, mdl in enumerate(models)]
    got = [None] * 4
    ts = [threading.Thread(target=run, args=(i, models[i])) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i in range(4):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(ref[i], got[i])), i
        models[i].release()
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_edges(dtype):
    fk, X, y, _ = _model(300, 1.5, dtype, seed=9)
    fmin = float(np.min(y))
    Xs = _candidates(60, 10, dtype)
    idx, ei, mean, var = fk.select_batch(Xs, 60, fmin)  # k = m
    assert sorted(idx.tolist()) == list(range(60))
    assert np.isfinite(ei).all() and np.isfinite(mean).all() and np.isfinite(var).all() and (var >= 0).all()
    # duplicate candidate rows and candidates on training points
    q = _candidates(20, 11, dtype)
    dup = np.vstack([X[:10], q, q[:7], X[:3]])
    for L in (None, float(np.median(y))):
        idx, ei, mean, var = fk.select_batch(dup, 30, fmin, lie=L)
        assert len(set(idx.tolist())) == 30
        assert np.isfinite(ei).all() and np.isfinite(mean).all() and np.isfinite(var).all()
    # k = 0 writes nothing
    lib = _lib.load()
    sfx = "f64" if dtype == np.float64 else "f32"
    idx0 = np.full(2, -7, np.int32)
    ei0 = np.full(2, 42.0)
    out = np.full(60, 42.0, dtype)
    rc = getattr(lib, f"hbegp_select_batch_{sfx}")(fk._h, _lib.aptr(Xs), 60, 0, fmin, None, idx0.ctypes.data_as(C.POINTER(C.c_int)),
                                                   _lib.dptr(ei0), _lib.aptr(out), _lib.aptr(out))
    assert rc == _lib.OK and (idx0 == -7).all() and (ei0 == 42.0).all() and (out == 42.0).all()
    fk.release()


def test_wrong_arguments_on_a_real_model():
    lib = _lib.load()
    fk, X, y, _ = _model(100, 2.5, np.float64, seed=12, d=2)
    Xs = _candidates(3, 1, np.float64, d=2)
    idx = np.zeros(3, np.int32)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int))

    def einval(rc, what):
        assert rc == _lib.EINVAL and what in _lib.last_error(), _lib.last_error()

    Xf = Xs.astype(np.float32)
    einval(lib.hbegp_select_batch_f32(fk._h, _lib.fptr(Xf), 3, 1, 0.0, None, ip, None, None, None), "f64 data")
    bad = Xs.copy()
    bad[1, 1] = math.nan
    einval(lib.hbegp_select_batch_f64(fk._h, _lib.dptr(bad), 3, 1, 0.0, None, ip, None, None, None), "non-finite coordinate")
    bad[1, 1] = -math.inf
    einval(lib.hbegp_select_batch_f64(fk._h, _lib.dptr(bad), 3, 2, 0.0, None, ip, None, None, None), "non-finite coordinate")
    einval(lib.hbegp_select_batch_f64(fk._h, _lib.dptr(Xs), 3, 4, 0.0, None, ip, None, None, None), "k must be <= m")
    einval(lib.hbegp_select_batch_f64(fk._h, _lib.dptr(Xs), 3, 1, math.nan, None, ip, None, None, None), "fmin must be finite")
    fk.release()


def _estimator_model(projection, d=3, n=120, seed=4):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = ((X - 0.37) ** 2).sum(axis=1) + 0.5
    est = E.EstimatorGPR.new(d).y_projection(projection)
    return est.estimate(X, y, None, E.RNG.new_with_seed(seed)), y


@pytest.mark.parametrize("projection", ["logarithmic", "linear"])
def test_select_batch_a_is_the_direct_call_with_projected_fmin_and_lie(projection):
    model, y = _estimator_model(projection)
    cand = np.random.default_rng(9).uniform(0, 1, (200, 3))
    fmin, lie = float(y.min()), float(np.median(y))
    for L in (None, lie):
        idx, means, ei = E.acquire_by_batch_ei(cand, model, 8, fmin, lie=L)
        fn = model._fmin_normalized(fmin)
        ln = None if L is None else model._fmin_normalized(L)
        didx, dei, _, _ = model.fitted.select_batch(cand, 8, fn, lie=ln)
        assert np.array_equal(idx, didx) and ei.tobytes() == dei.tobytes()
        pm = model.predict_mean_a(cand[idx])
        assert means.tobytes() == pm.tobytes()
        # k = 1 is find_best_candidate_by_ei's pick
        i1, _, _ = E.find_best_candidate_by_ei(cand, model, fmin)
        assert idx[0] == i1 or abs(ei[0] - model.predict_mean_ei_a(cand[[i1]], fmin)[1][0]) <= 1e-9 * max(1.0, ei[0])
