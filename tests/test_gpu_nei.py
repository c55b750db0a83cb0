"""GPU: noisy expected improvement over a candidate set (hbegp_noisy_ei_*).

The device's nei, fmin_draws and rho replayed through the NumPy restatement (tests/nei_ref.py) on the engine's own predict_cov
mean and Sigma of the union, over the shapes where the block logic can go wrong; the meaning of nei_j end to end through
sample_posterior on [baseline; x_j]; zero draws; candidates that repeat (they never enter a factorisation); the PD contract of
the baseline block; bits, threads and a clean pool; argument checks on a real model; the estimator's acquire_by_noisy_ei.

Bars: the project's plain 1e-8 (f64) / 1e-4 (f32) times max(1, sqrt(c)) on nei and fmin_draws, times c on rho.  Measured
deviations from the restatement: see DESIGN section 18."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import nei_ref as NEI
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

NUS = [0.5, 1.5, 2.5, math.inf]
D = 4
# f32: a noise of the amplitude's size keeps cond(K) <= n + 1 (tests/test_gpu_batch_select.py)
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
    return fk, X, y


def _candidates(m, seed, dtype, d=D):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (m, d)).astype(dtype)


def _normals(S, mb, seed, dtype):
    return np.random.default_rng(seed).standard_normal((S, mb)).astype(dtype)


def _rel(dtype):
    return 1e-8 if dtype == np.float64 else 1e-4


def _replay(fk, base, cand, z, dtype, mean0=None, cov0=None, jitter=0.0):
    """The device's outputs against the restatement on the engine's own mean and Sigma of [base; cand] (mean0 / cov0 when the
    caller already holds them).  Returns the deviations (nei, fmin_draws, rho / c)."""
    mb, mc = len(base), len(cand)
    nei, best, fmin_draws, rho = fk.noisy_ei(base, cand, z, jitter=jitter, want_details=True)
    assert nei.dtype == np.float64 and nei.shape == (mc,) and rho.shape == (mc,) and fmin_draws.shape == (len(z),)
    if mean0 is None:
        mean0, cov0 = fk.predict_cov(np.vstack([base, cand]), jitter=jitter)
    ref, rho_ref, fmin_ref = NEI.nei(mean0, cov0, mb, z)
    bar = NEI.bars(dtype, fk.amplitude)
    d_nei = float(np.abs(nei - ref).max()) if mc else 0.0
    d_rho = float(np.abs(rho - rho_ref).max()) / fk.amplitude if mc else 0.0
    d_fmin = float(np.abs(fmin_draws - fmin_ref).max())
    assert d_nei <= bar and d_fmin <= bar and d_rho <= _rel(dtype), (mb, mc, len(z), d_nei, d_fmin, d_rho)
    assert (nei >= 0.0).all() and (rho >= 0.0).all()
    assert best == (NEI.argmax_last(nei) if mc else -1)
    return d_nei, d_fmin, d_rho


@pytest.mark.parametrize("n", [100, 300, 1000])
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_nei_replays_through_the_restatement(dtype, nu, n):
    """Worst deviations measured on an MI355X over all 24 cases (the table per case: DESIGN section 18):
    f64: nei 2.6e-15, fmin_draws 5.6e-16, rho / c 1.7e-16 (bars 1.1e-8, 1.1e-8, 1e-8);
    f32: nei 7.2e-5, fmin_draws 4.6e-5, rho / c 1.1e-6 (bars 1.1e-4, 1.1e-4, 1e-4) -- both at nu = inf, n = 300, where
    cond(Sigma_bb) = 1.3e5 (n = 1000: 5.9e-5); every f32 case with a finite nu stays below 1e-6."""
    fk, X, y = _model(n, nu, dtype, seed=n)
    pool = _candidates(130, 11 + n, dtype)
    mbs = sorted({min(mb, n) for mb in (1, 127, 128, 129, 300)})
    top = mbs[-1]
    mean_u, cov_u = fk.predict_cov(np.vstack([X[:top], pool]))  # once per model: every shape's Sigma is a sub-matrix
    worst = np.zeros(3)
    for mb in mbs:
        for mc in (0, 1, 130):
            rows = np.concatenate([np.arange(mb), top + np.arange(mc)])
            mean0, cov0 = mean_u[rows], cov_u[np.ix_(rows, rows)]
            for S in (1, 64, 129):
                z = _normals(S, mb, 1000 * mb + S, dtype)
                worst = np.maximum(worst, _replay(fk, X[:mb], pool[:mc], z, dtype, mean0, cov0))
    print(f"{np.dtype(dtype).name} nu={nu} n={n}: deviation nei {worst[0]:.1e} fmin {worst[1]:.1e} (bar "
          f"{NEI.bars(dtype, fk.amplitude):.1e}) rho/c {worst[2]:.1e} (bar {_rel(dtype):.0e})")
    fk.release()


def test_replay_with_a_baseline_of_eight_blocks():
    fk, X, y = _model(1024, 2.5, np.float64, seed=3)
    dev = _replay(fk, X, _candidates(600, 5, np.float64), _normals(256, 1024, 6, np.float64), np.float64)
    print(f"n=1024 mb=1024 mc=600 S=256: deviation nei {dev[0]:.1e} fmin {dev[1]:.1e} rho/c {dev[2]:.1e}")
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nei_is_the_average_ei_of_posterior_draws_on_the_baseline_and_one_candidate(dtype):
    """An independent device path: sample_posterior factors [baseline; x_j] as one matrix, so with the normals [z_s, 0] and
    [z_s, 1] its last column is mu_js and mu_js + sqrt(rho_j), its first mb columns give fmin_s."""
    fk, X, y = _model(300, 2.5, dtype, seed=21)
    mb, S = 150, 96
    base, cand = X[:mb], _candidates(20, 22, dtype)
    z = _normals(S, mb, 23, dtype)
    nei, best, fmin_draws, rho = fk.noisy_ei(base, cand, z, want_details=True)
    bar = NEI.bars(dtype, fk.amplitude)
    zmax = float(np.abs(z).max())
    for j in sorted({best, 0, 17}):
        pts = np.vstack([base, cand[j:j + 1]])
        s0, _ = fk.sample_posterior(pts, np.hstack([z, np.zeros((S, 1), dtype)]))
        s1, _ = fk.sample_posterior(pts, np.hstack([z, np.ones((S, 1), dtype)]))
        s0, s1 = s0.astype(np.float64), s1.astype(np.float64)
        mu_js, sd = s0[:, mb], float(np.mean(s1[:, mb] - s0[:, mb]))
        fmin_s = s0[:, :mb].min(axis=1)
        host = float(np.mean(NEI.ei(mu_js, sd, fmin_s)))
        # mu_js against the restatement on predict_cov's Sigma of the same mb + 1 rows
        mean0, cov0 = fk.predict_cov(pts)
        _, A, _ = NEI.parts(cov0, mb)
        d_mu = float(np.abs(mu_js - (float(mean0[mb]) + z.astype(np.float64) @ A[0])).max())
        print(f"{np.dtype(dtype).name} j={j}: nei {nei[j]:.6e} draws {host:.6e} (bar {bar:.1e}); mu_js deviation {d_mu:.1e}; "
              f"fmin deviation {np.abs(fmin_s - fmin_draws).max():.1e}")
        assert d_mu <= _rel(dtype) * math.sqrt(fk.amplitude) * max(1.0, zmax), (j, d_mu)
        assert np.abs(fmin_s - fmin_draws).max() <= bar, j
        assert abs(sd - math.sqrt(rho[j])) <= bar, (j, sd, rho[j])
        assert abs(host - nei[j]) <= bar, (j, host, nei[j])
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_draws_give_plain_ei_at_the_lowest_baseline_mean(dtype):
    fk, X, y = _model(300, 1.5, dtype, seed=9)
    base, cand = X[:200], _candidates(50, 31, dtype)
    nei, best, fmin_draws, rho = fk.noisy_ei(base, cand, np.zeros((5, 200), dtype), want_details=True)
    mean_b, _, _ = fk.predict(base, want_variance=False)
    mean_c, _, _ = fk.predict(cand, want_variance=False)
    lo = float(mean_b.astype(np.float64).min())
    assert np.abs(fmin_draws - lo).max() <= 1e-12 * max(1.0, abs(lo))
    ref = NEI.ei(mean_c.astype(np.float64), np.sqrt(rho), lo)
    assert np.abs(nei - ref).max() <= NEI.bars(dtype, fk.amplitude)
    assert best == NEI.argmax_last(nei)
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_candidates_never_enter_a_factorisation(dtype):
    fk, X, y = _model(300, 2.5, dtype, seed=12)
    q = _candidates(8, 13, dtype)
    cand = np.vstack([np.repeat(q[:1], 200, axis=0), X[:10], q[1:], q[1:]])  # 200 copies of one point, training rows, repeats
    z = _normals(64, 140, 14, dtype)
    lib = _lib.load()
    x = np.ascontiguousarray(np.vstack([X[:140], cand]))
    nei = np.zeros(len(cand))
    rc = getattr(lib, "hbegp_noisy_ei_" + ("f64" if dtype == np.float64 else "f32"))(
        fk._h, _lib.aptr(x), len(x), 140, _lib.aptr(z), 64, 0.0, _lib.dptr(nei), None, None, None, None)
    assert rc == _lib.OK and np.isfinite(nei).all()
    bar = NEI.bars(dtype, fk.amplitude)
    assert np.abs(nei[:200] - nei[0]).max() <= bar
    assert np.abs(nei[210:217] - nei[217:224]).max() <= bar
    dev = _replay(fk, X[:140], cand, z, dtype)
    print(f"{np.dtype(dtype).name} 200 copies / training rows / repeats: deviation nei {dev[0]:.1e} fmin {dev[1]:.1e} rho/c {dev[2]:.1e}")
    fk.release()


def test_the_baseline_block_alone_decides_not_positive_definite():
    # a baseline of many copies of two points in f32: Sigma_bb's smallest eigenvalue (1e-5) is below what f32 resolves beside c,
    # so its factor may fail.  Either the call succeeds, or it reports HBEGP_NOT_PD with the failing panel and leaves every other
    # output alone; a jitter of the amplitude's size always factors.
    rng = np.random.default_rng(2)
    X = rng.uniform(0, 1, (300, D)).astype(np.float32)
    y = (np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(300)).astype(np.float32)
    theta = np.log(np.concatenate([[1e-3 * 1.3, 1.3], np.linspace(0.3, 0.9, D)]))
    fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
    lib = _lib.load()
    mb, mc, S = 256, 5, 3
    base = np.repeat(_candidates(2, 6, np.float32), mb // 2, axis=0)
    cand = _candidates(mc, 7, np.float32)
    x = np.ascontiguousarray(np.vstack([base, cand]))
    z = np.ones((S, mb), np.float32)
    nei, fm, rho = np.full(mc, 42.0), np.full(S, 42.0), np.full(mc, 42.0)
    best, info = C.c_int(-7), C.c_int(-1)
    rc = lib.hbegp_noisy_ei_f32(fk._h, _lib.fptr(x), mb + mc, mb, _lib.fptr(z), S, 0.0, _lib.dptr(nei), C.byref(best), _lib.dptr(fm),
                                _lib.dptr(rho), C.byref(info))
    print(f"f32, a baseline of {mb} rows of 2 points, jitter 0: rc {rc}, info {info.value}")
    if rc == _lib.NOT_PD:
        assert 1 <= info.value <= mb and (nei == 42.0).all() and (fm == 42.0).all() and (rho == 42.0).all() and best.value == -7
        with pytest.raises(_lib.HbegpError) as e:
            fk.noisy_ei(base, cand, z)
        assert e.value.code == _lib.NOT_PD
    else:
        assert rc == _lib.OK and info.value == 0 and np.isfinite(nei).all()
    n2, b2, f2, r2 = fk.noisy_ei(base, cand, z, jitter=1.0, want_details=True)
    assert np.isfinite(n2).all() and np.isfinite(f2).all() and np.isfinite(r2).all() and b2 == NEI.argmax_last(n2)
    fk.release()


def test_bits_threads_and_a_clean_pool():
    fk, X, y = _model(700, 2.5, np.float64, seed=8)
    shapes = [(100, 50, 16), (128, 200, 64), (300, 1, 33), (700, 130, 8)]
    args = [(X[:mb], _candidates(mc, 60 + i, np.float64), _normals(S, mb, 80 + i, np.float64)) for i, (mb, mc, S) in enumerate(shapes)]
    probe = _candidates(200, 70, np.float64)
    p0, c0 = fk.predict(probe), fk.predict_cov(probe)
    solo = [fk.noisy_ei(*a, want_details=True) for a in args]
    again = [fk.noisy_ei(*a, want_details=True) for a in args]

    def same(a, b):
        return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b))

    for a, b in zip(solo, again):
        assert same(a, b)
    p1, c1 = fk.predict(probe), fk.predict_cov(probe)  # the pool went back clean
    assert p0[0].tobytes() == p1[0].tobytes() and p0[1].tobytes() == p1[1].tobytes()
    assert c0[0].tobytes() == c1[0].tobytes() and c0[1].tobytes() == c1[1].tobytes()
    got = [None] * 4

    def run(i):
        for _ in range(3):
            got[i] = fk.noisy_ei(*args[i], want_details=True)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i in range(4):
        assert same(solo[i], got[i]), i
    fk.release()


def test_wrong_arguments_on_a_real_model():
    lib = _lib.load()
    fk, X, y = _model(100, 2.5, np.float64, seed=12, d=2)
    Xs = _candidates(5, 1, np.float64, d=2)
    z = np.zeros((2, 3))
    nei = np.full(2, 7.0)

    def einval(rc, what):
        assert rc == _lib.EINVAL and what in _lib.last_error(), _lib.last_error()

    def f64(x, m, mb, nei_p):
        return lib.hbegp_noisy_ei_f64(fk._h, _lib.dptr(x), m, mb, _lib.dptr(z), 2, 0.0, nei_p, None, None, None, None)

    Xf, zf = Xs.astype(np.float32), z.astype(np.float32)
    einval(lib.hbegp_noisy_ei_f32(fk._h, _lib.fptr(Xf), 5, 3, _lib.fptr(zf), 2, 0.0, _lib.dptr(nei), None, None, None, None), "f64 data")
    bad = Xs.copy()
    bad[1, 1] = math.nan  # a baseline row
    einval(f64(bad, 5, 3, _lib.dptr(nei)), "non-finite coordinate")
    bad = Xs.copy()
    bad[4, 0] = -math.inf  # a candidate row
    einval(f64(bad, 5, 3, _lib.dptr(nei)), "non-finite coordinate")
    einval(f64(Xs, 3, 4, _lib.dptr(nei)), "mb must be <= m")
    einval(f64(Xs, 5, 3, None), "nei is NULL")
    assert (nei == 7.0).all()  # a refused call writes nothing
    assert f64(Xs, 5, 3, _lib.dptr(nei)) == _lib.OK and np.isfinite(nei).all() and (nei >= 0).all()
    assert f64(Xs, 3, 3, None) == _lib.OK  # mc = 0 needs no nei
    fk.release()


@pytest.mark.parametrize("projection", ["logarithmic", "linear"])
def test_acquire_by_noisy_ei(projection):
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 1, (120, 3))
    y = ((X - 0.37) ** 2).sum(axis=1) + 0.5 + 0.05 * rng.standard_normal(120) ** 2
    model = E.EstimatorGPR.new(3).y_projection(projection).estimate(X, y, None, E.RNG.new_with_seed(4))
    cand = np.random.default_rng(9).uniform(0, 1, (150, 3))
    nei, best = model.noisy_ei_a(cand, 64, np.random.default_rng(5))
    z = np.random.default_rng(5).standard_normal((64, 120)).astype(model.dtype)
    dnei, dbest = model.fitted.noisy_ei(model.fitted.x_train, cand.astype(model.dtype), z)
    assert nei.tobytes() == dnei.tobytes() and best == dbest == NEI.argmax_last(nei) and nei[best] > 0
    nei30, best30 = model.noisy_ei_a(cand, 64, np.random.default_rng(5), max_baseline=30)
    assert nei30.shape == (150,) and best30 == NEI.argmax_last(nei30)
    pm = model.predict_mean_a(cand)
    idx, means, neis = E.acquire_by_noisy_ei(cand, model, 1, np.random.default_rng(5), n_samples=64)
    assert idx.tolist() == [best] and neis[0] == nei[best] and means[0] == pm[best]
    idx, means, neis = E.acquire_by_noisy_ei(cand, model, 4, np.random.default_rng(5), n_samples=64)
    assert len(set(idx.tolist())) == 4 and idx[0] == best and neis[0] == nei[best] and (neis >= 0).all() and np.isfinite(means).all()
