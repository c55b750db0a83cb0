"""GPU: the knowledge gradient over a candidate set (hbegp_knowledge_gradient_*).

The device's kg replayed through the NumPy restatement (tests/kg_ref.py) on the engine's own Sigma and mean; best / imin / the
posterior outputs against predict_cov bit for bit; the meaning of kg_j end to end, against predict on the model extended with
one noisy sample over a grid of z; bits, prefixes, threads and a clean pool; edge cases and argument checks; the estimator's
acquire_by_knowledge_gradient.

Measured deviations from the restatement, in y units (bars: 1e-8 / 1e-4 times max(1, sqrt(c))): see DESIGN section 16."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import kg_ref as KG
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


def _replay(fk, Xs, mc, dtype):
    """The device's kg[mc] against the restatement on the engine's own mean and Sigma; best, imin and the posterior outputs
    against predict_cov.  Returns the worst deviation of kg in y units."""
    m = len(Xs)
    kg, best, imin, mean, var = fk.knowledge_gradient(Xs, n_candidates=mc, want_posterior=True)
    assert kg.dtype == np.float64 and kg.shape == (mc,) and mean.dtype == dtype and var.dtype == dtype
    mean0, cov = fk.predict_cov(Xs)
    ref = KG.kg(mean0, np.asarray(cov, np.float64), fk.device_params()[0], mc=mc)  # (one conversion, not one per candidate)
    dev = float(np.abs(kg - ref).max()) if mc else 0.0
    assert dev <= KG.bars(dtype, fk.amplitude), (m, mc, dev)
    assert (kg >= 0.0).all()
    assert best == (KG.argmax_last(kg) if mc else -1)
    assert imin == int(np.argmin(mean0))
    assert mean.tobytes() == mean0.tobytes()
    assert var.tobytes() == np.maximum(np.diag(cov), 0).astype(dtype).tobytes()
    if m > 16:  # predict's batched path: the same launches
        pm, _, _ = fk.predict(Xs, want_variance=False)
        assert mean.tobytes() == pm.tobytes()
    return dev


@pytest.mark.parametrize("n", [100, 300, 1000])
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_kg_replays_through_the_restatement(dtype, nu, n):
    fk, X, y = _model(n, nu, dtype, seed=n)
    pool = _candidates(300, 11 + n, dtype)
    worst = 0.0
    for m in (1, 40, 300):
        for mc in sorted({1, m}):
            worst = max(worst, _replay(fk, pool[:m], mc, dtype))
    print(f"{np.dtype(dtype).name} nu={nu} n={n}: kg deviation {worst:.1e} (bar {KG.bars(dtype, fk.amplitude):.1e})")
    fk.release()


def test_replay_at_n_4096_m_2000():
    fk, X, y = _model(4096, 2.5, np.float64, seed=3)
    dev = _replay(fk, _candidates(2000, 5, np.float64), 2000, np.float64)
    print(f"n=4096 m=2000 mc=2000: kg deviation {dev:.1e}")
    fk.release()


def test_replay_past_the_lds_limit():
    fk, X, y = _model(300, 2.5, np.float64, seed=4)
    dev = _replay(fk, _candidates(10000, 6, np.float64), 8, np.float64)  # 16384 padded lines: the global workspace
    print(f"n=300 m=10000 mc=8: kg deviation {dev:.1e}")
    fk.release()


@pytest.mark.parametrize("m", [4096, 4097, 8192, 8193])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_replay_around_the_line_storage_limits(dtype, m):
    """The lines of a candidate live in dynamic LDS up to P = 8192 padded rows, above that in a pool block: m = 4096 is the first
    launch above the 64 KiB a kernel gets by default (P = 4096: 67,600 B), 4097 and 8192 the largest (P = 8192: 133,136 B), 8193
    the first with the global workspace (P = 16384)."""
    fk, X, y = _model(300, 2.5, dtype, seed=4)
    dev = _replay(fk, _candidates(m, 6, dtype), 8, dtype)
    print(f"{np.dtype(dtype).name} n=300 m={m} mc=8: kg deviation {dev:.1e} (bar {KG.bars(dtype, fk.amplitude):.1e})")
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_workgroups_second_candidate_in_the_global_workspace(dtype):
    """mc = 520 > KG_GLOBAL_WGS = 512 at m = 8193: workgroups 0 .. 7 run candidates 512 .. 519 in the lines their first candidate
    left behind."""
    fk, X, y = _model(300, 2.5, dtype, seed=4)
    Xs = _candidates(8193, 6, dtype)
    kg8, _, _ = fk.knowledge_gradient(Xs, n_candidates=8)
    kg, best, imin = fk.knowledge_gradient(Xs, n_candidates=520)
    assert kg[:8].tobytes() == kg8.tobytes()
    mean, cov = fk.predict_cov(Xs)
    s2 = fk.device_params()[0]
    cov64, mean64 = np.asarray(cov, np.float64), np.asarray(mean, np.float64)
    for j in (0, 511, 512, 513, 519):
        ref = KG.h(-mean64, -KG.sigma_tilde(cov64, j, s2)[0])
        assert abs(kg[j] - ref) <= KG.bars(dtype, fk.amplitude), (j, kg[j], ref)
    assert best == KG.argmax_last(kg) and imin == int(np.argmin(mean))
    fk.release()


def test_kg_is_the_expected_drop_of_the_minimum_of_the_extended_models_mean():
    dtype = np.float64
    fk, X, y = _model(300, 2.5, dtype, seed=21)
    Xs = _candidates(40, 22, dtype)
    kg, best, _, mean, var = fk.knowledge_gradient(Xs, want_posterior=True)
    s2 = fk.device_params()[0]
    _, cov = fk.predict_cov(Xs)
    # a dense trapezoid over z in [-8, 8] (beyond: phi(8) (|mu| + 8 |st|) < 1e-13), the coarser grids nested in the finest
    zmax, step = 8.0, 1.0 / 16
    z = np.linspace(-zmax, zmax, int(round(2 * zmax / step)) + 1)
    w = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    for j in sorted({best, 0, 17}):
        sd = math.sqrt(max(float(cov[j, j]) - KG.MIN_NOISE, 0.0) + s2)
        drop = np.zeros(len(z))
        for t, zt in enumerate(z):
            ext = fk.extend_with(np.vstack([X, Xs[j:j + 1]]), np.concatenate([y, [mean[j] + sd * zt]]))
            em, _, _ = ext.predict(Xs, want_variance=False)
            drop[t] = float(mean.min()) - float(em.min())
            ext.release()
        q = []
        for stride in (4, 2, 1):
            g = (drop * w)[::stride]
            q.append(float(step * stride * (g.sum() - 0.5 * (g[0] + g[-1]))))
        # the trapezoid's error at the kinks of min_i(.) falls by 4 per halving: four times the larger of the last two changes
        # (tests/test_kg_cpu.py), plus the extended model's own distance from the conditioning formula, the project's plain bar on
        # a mean, on both minima
        tol = 4.0 * max(abs(q[0] - q[1]), abs(q[1] - q[2])) + 2.0 * KG.bars(dtype, fk.amplitude)
        print(f"j={j}: kg {kg[j]:.6e} quadrature of the extended models {q[2]:.6e} (steps: {q[0]:.6e} {q[1]:.6e}) tol {tol:.1e}")
        assert abs(kg[j] - q[2]) <= tol, (j, kg[j], q, tol)
    fk.release()


def test_bits_prefixes_threads_and_a_clean_pool():
    fk, X, y = _model(700, 2.5, np.float64, seed=8)
    Xs = [_candidates(50 + 100 * i, 60 + i, np.float64) for i in range(4)]
    probe = _candidates(200, 70, np.float64)
    p0, c0 = fk.predict(probe), fk.predict_cov(probe)
    solo = [fk.knowledge_gradient(x, want_posterior=True) for x in Xs]
    again = [fk.knowledge_gradient(x, want_posterior=True) for x in Xs]

    def same(a, b):
        return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b))

    for a, b in zip(solo, again):
        assert same(a, b)
    for mc in (0, 1, 7, 100):
        kg, best, imin = fk.knowledge_gradient(Xs[1], n_candidates=mc)
        assert kg.tobytes() == solo[1][0][:mc].tobytes() and imin == solo[1][2], mc
        assert best == (KG.argmax_last(kg) if mc else -1)
    p1, c1 = fk.predict(probe), fk.predict_cov(probe)  # the pool went back clean
    assert p0[0].tobytes() == p1[0].tobytes() and p0[1].tobytes() == p1[1].tobytes()
    assert c0[0].tobytes() == c1[0].tobytes() and c0[1].tobytes() == c1[1].tobytes()
    got = [None] * 4

    def run(i):
        for _ in range(3):
            got[i] = fk.knowledge_gradient(Xs[i], want_posterior=True)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i in range(4):
        assert same(solo[i], got[i]), i
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_edges(dtype):
    fk, X, y = _model(300, 1.5, dtype, seed=9)
    q = _candidates(20, 11, dtype)
    dup = np.vstack([X[:10], q, q[:7], X[:3]])  # duplicate rows and rows on training points
    dev = _replay(fk, dup, len(dup), dtype)
    kg, best, imin = fk.knowledge_gradient(dup)
    assert np.isfinite(kg).all()
    assert kg[10:17].tobytes() == kg[30:37].tobytes() or np.abs(kg[10:17] - kg[30:37]).max() <= KG.bars(dtype, fk.amplitude)
    print(f"{np.dtype(dtype).name} duplicates / training rows: kg deviation {dev:.1e}")
    kg, best, imin = fk.knowledge_gradient(q[:1])  # m = 1: one line
    assert kg[0] == 0.0 and best == 0 and imin == 0
    kg, best, imin, mean, var = fk.knowledge_gradient(q, n_candidates=0, want_posterior=True)  # mc = 0
    mean0, cov = fk.predict_cov(q)
    assert kg.shape == (0,) and best == -1 and imin == int(np.argmin(mean0))
    assert mean.tobytes() == mean0.tobytes() and var.tobytes() == np.maximum(np.diag(cov), 0).astype(dtype).tobytes()
    # m = 0 is a no-op
    lib = _lib.load()
    b, i = C.c_int(5), C.c_int(5)
    fn = getattr(lib, "hbegp_knowledge_gradient_" + ("f64" if dtype == np.float64 else "f32"))
    assert fn(fk._h, None, 0, 0, None, C.byref(b), C.byref(i), None, None) == _lib.OK and b.value == -1 and i.value == -1
    fk.release()


def test_wrong_arguments_on_a_real_model():
    lib = _lib.load()
    fk, X, y = _model(100, 2.5, np.float64, seed=12, d=2)
    Xs = _candidates(3, 1, np.float64, d=2)
    kg = np.zeros(3)

    def einval(rc, what):
        assert rc == _lib.EINVAL and what in _lib.last_error(), _lib.last_error()

    Xf = Xs.astype(np.float32)
    einval(lib.hbegp_knowledge_gradient_f32(fk._h, _lib.fptr(Xf), 3, 1, _lib.dptr(kg), None, None, None, None), "f64 data")
    bad = Xs.copy()
    bad[1, 1] = math.nan
    einval(lib.hbegp_knowledge_gradient_f64(fk._h, _lib.dptr(bad), 3, 1, _lib.dptr(kg), None, None, None, None), "non-finite coordinate")
    bad[1, 1] = -math.inf
    einval(lib.hbegp_knowledge_gradient_f64(fk._h, _lib.dptr(bad), 3, 0, None, None, None, None, None), "non-finite coordinate")
    einval(lib.hbegp_knowledge_gradient_f64(fk._h, _lib.dptr(Xs), 3, 4, _lib.dptr(kg), None, None, None, None), "mc must be <= m")
    einval(lib.hbegp_knowledge_gradient_f64(fk._h, _lib.dptr(Xs), 3, 2, None, None, None, None, None), "kg is NULL")
    assert lib.hbegp_knowledge_gradient_f64(fk._h, _lib.dptr(Xs), 3, 3, _lib.dptr(kg), None, None, None, None) == _lib.OK
    fk.release()


@pytest.mark.parametrize("projection", ["logarithmic", "linear"])
def test_acquire_by_knowledge_gradient(projection):
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 1, (120, 3))
    y = ((X - 0.37) ** 2).sum(axis=1) + 0.5 + 0.05 * rng.standard_normal(120) ** 2
    model = E.EstimatorGPR.new(3).y_projection(projection).estimate(X, y, None, E.RNG.new_with_seed(4))
    cand = np.random.default_rng(9).uniform(0, 1, (200, 3))
    kg, best = model.knowledge_gradient_a(cand, n_candidates=150)
    dkg, dbest, dimin = model.fitted.knowledge_gradient(cand, n_candidates=150)
    assert kg.tobytes() == dkg.tobytes() and best == dbest == KG.argmax_last(kg)
    imin, m_imin = model.best_by_mean_a(cand)
    pm = model.predict_mean_a(cand)
    assert imin == dimin == int(np.argmin(pm)) and m_imin == pm[imin]
    idx, means, kgs = E.acquire_by_knowledge_gradient(cand, model, 1, n_candidates=150)
    assert idx.tolist() == [best] and kgs[0] == kg[best] and means[0] == pm[best]
    idx, means, kgs = E.acquire_by_knowledge_gradient(cand, model, 6, n_candidates=150)
    assert len(set(idx.tolist())) == 6 and idx[0] == best and idx.max() < 150 and (kgs >= 0).all()
    # conditioning on the first fantasy lowers what a second sample there is worth
    assert np.isfinite(means).all() and kgs[0] == kg[best]
