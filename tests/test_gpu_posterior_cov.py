"""GPU: the joint posterior at the query points (hbegp_predict_cov_*) and joint draws from it (hbegp_sample_posterior_*).

Sigma against the NumPy restatement (tests/posterior_cov_ref.py) and, on the fitted config-M model, against an extended-precision
truth from the referee; its diagonal against hbegp_predict's variance; the jitter; the draws against mean + cholesky(Sigma) z
on the engine's own Sigma; argmin and its ties; Monte-Carlo moments; edge cases, argument checks, bits and threads; the
estimator's sample_a / acquire_by_thompson."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import posterior_cov_ref as PC
from hbetune_rs_amd import _lib, gpr, synth
from hbetune_rs_amd import estimator as E
from oracle import gpr_oracle as O
from oracle import referee as R

pytestmark = pytest.mark.gpu

NUS = [0.5, 1.5, 2.5, math.inf]
D = 4


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


def _ref(fk, X, Xs, jitter=0.0):
    return PC.sigma_ref(Xs, X, fk.amplitude, fk.length_scale, fk.nu, fk.noise, jitter=jitter)


# f32: a noise of the amplitude's size keeps cond(K) <= n + 1 (4.1e3 at n = 4096), the range in which the f32 L^-1 of the model
# carries the 1e-4 bar (the same range as the f32 variance gradient, tests/test_gpu_predict_grad.py)
F32_NOISE = 1.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [200, 4096])
@pytest.mark.parametrize("nu", NUS)
def test_sigma_parity_with_the_restatement(nu, n, dtype):
    fk, X, cond_bound = _model(n, D, nu, dtype, noise_over_amp=1e-2 if dtype == np.float64 else F32_NOISE)
    assert cond_bound <= (5e5 if dtype == np.float64 else 4.2e3)
    pool = _candidates(2000, D, 7 + n).astype(dtype)
    ref = _ref(fk, X, pool)
    bar = 1e-8 if dtype == np.float64 else 1e-4
    c = fk.amplitude
    for m in (1, 5, 40, 300, 2000):
        Xs = pool[:m]
        mean, cov = fk.predict_cov(Xs)
        assert cov.dtype == dtype and cov.shape == (m, m) and mean.shape == (m,)
        assert np.array_equal(cov, cov.T)  # mirrored, bit for bit
        dev = float(np.abs(cov.astype(np.float64) - ref[:m, :m]).max()) / c
        pm, pv, _ = fk.predict(Xs)
        if m > 8:
            assert mean.tobytes() == pm.tobytes()  # the batched predict's own mean (predict takes another path for m <= 8)
        else:
            assert np.abs(mean.astype(np.float64) - pm).max() <= (1e-12 if dtype == np.float64 else 1e-5) * max(1.0, np.abs(pm).max())
        keep = pv > 0  # rows the variance clamp did not touch
        ddev = float(np.abs(np.diag(cov).astype(np.float64)[keep] - pv.astype(np.float64)[keep]).max(initial=0.0)) / c
        print(f"nu={nu} n={n} {np.dtype(dtype).name} m={m}: Sigma {dev:.2e} diag vs predict {ddev:.2e} (cond(K) <= {cond_bound:.1e})")
        assert dev <= bar, (m, dev)
        assert ddev <= (1e-12 if dtype == np.float64 else 1e-5), (m, ddev)
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_jitter_moves_the_diagonal_only(dtype):
    fk, X, _ = _model(300, D, 2.5, dtype, noise_over_amp=1e-2 if dtype == np.float64 else F32_NOISE)
    Xs = _candidates(150, D, 3).astype(dtype)
    _, c0 = fk.predict_cov(Xs)
    _, c1 = fk.predict_cov(Xs, jitter=0.125)
    off = ~np.eye(150, dtype=bool)
    assert c0[off].tobytes() == c1[off].tobytes()
    shift = np.diag(c1).astype(np.float64) - np.diag(c0).astype(np.float64)
    assert np.abs(shift - 0.125).max() <= (1e-12 if dtype == np.float64 else 1e-6), np.abs(shift - 0.125).max()
    fk.release()


def _truth_sigma(fk, X, y, Xs):
    """K** + 1e-5 I - K*^T K^-1 K* with the cross term in double-double (referee: iterative refinement in extended precision)."""
    rf = R.Referee(X, y, fk.noise, fk.amplitude, fk.length_scale, fk.nu)
    truth = rf.sigma(Xs)
    rf.close()
    return truth


def test_fitted_m_size_model():
    w = synth.make_workload("M")
    X, y = w["X"], w["y"]
    starts = synth.restart_points("M", w["lo"], w["hi"], 2)
    fk = gpr.FittedKernel.new(X, y, w["theta0"], w["lo"], w["hi"], starts)
    Xs = synth.candidates("M", 300, w["d"])
    _, cov = fk.predict_cov(Xs)
    truth = _truth_sigma(fk, X, y, Xs)
    # the reference's own form: K* K^-1 K*^T with an explicit potri inverse
    K = PC.kernel_matrix(X, fk.amplitude, fk.length_scale, fk.nu, fk.noise)
    chol, info = O._potrf(K)
    assert info == 0
    lapack = PC.sigma_ref_kinv(Xs, X, O._potri(chol), fk.amplitude, fk.length_scale, fk.nu)
    dg, dl = np.abs(cov - truth), np.abs(lapack - truth)
    print(f"M: |gpu - truth| max {dg.max():.2e}, |lapack - truth| max {dl.max():.2e}, amplitude {fk.amplitude:.3g}")
    assert (dg <= np.maximum(1e-8, 2 * dl)).all(), float((dg - np.maximum(1e-8, 2 * dl)).max())
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_draws_are_mean_plus_cholesky_of_the_engines_sigma(dtype):
    fk, X, _ = _model(500, D, 1.5, dtype, noise_over_amp=1e-2 if dtype == np.float64 else F32_NOISE)
    m, S = 300, 64
    Xs = _candidates(m, D, 5).astype(dtype)
    mean, cov = fk.predict_cov(Xs)
    z = E.RNG(9).standard_normal((S, m)).astype(dtype)
    samples, argmin = fk.sample_posterior(Xs, z)
    assert samples.dtype == dtype and samples.shape == (S, m) and argmin.shape == (S,)
    want = PC.draws_ref(mean, cov, z)
    dev = float(np.abs(samples.astype(np.float64) - want).max()) / (math.sqrt(fk.amplitude) * float(np.abs(z).max()))
    print(f"{np.dtype(dtype).name}: draws vs mean + chol(Sigma) z: {dev:.2e}")
    # measured: 3.6e-16 (f64) and 2.5e-7 (f32, Sigma factored in f32 with fp64 diagonal blocks); the f32 bar leaves 40x room
    assert dev <= (1e-10 if dtype == np.float64 else 1e-5), dev
    assert np.array_equal(argmin, np.argmin(samples, axis=1))
    _, argmin2 = fk.sample_posterior(Xs, z, want_samples=False)
    assert np.array_equal(argmin2, argmin)
    fk.release()


def test_argmin_ties_go_to_the_lower_index():
    fk, X, _ = _model(300, D, 2.5, np.float64)
    pool = _candidates(10, D, 8)
    pm, _, _ = fk.predict(pool)
    best = pool[int(np.argmin(pm))]
    others = pool[np.arange(10) != int(np.argmin(pm))]
    Xs = np.vstack([others[:2], best, others[2:5], best, others[5:]])  # the smallest mean at rows 2 and 6
    z = np.zeros((3, len(Xs)))
    samples, argmin = fk.sample_posterior(Xs, z)  # duplicate rows: Sigma is singular but for the 1e-5 floor
    assert samples[0, 2] == samples[0, 6]
    assert (argmin == 2).all(), argmin
    _, argmin2 = fk.sample_posterior(Xs, z, want_samples=False)
    assert (argmin2 == 2).all()
    fk.release()


def test_monte_carlo_moments():
    fk, X, _ = _model(400, D, 2.5, np.float64)
    m, N = 16, 20000
    Xs = _candidates(m, D, 12)
    mean, cov = fk.predict_cov(Xs)
    z = E.RNG(2024).standard_normal((N, m))
    samples, _ = fk.sample_posterior(Xs, z)
    emp_mean = samples.mean(axis=0)
    emp_cov = np.cov(samples.T)
    se_mean = np.sqrt(np.diag(cov) / N)
    se_cov = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov * cov) / N)
    assert (np.abs(emp_mean - mean) <= 5 * se_mean).all()
    assert (np.abs(emp_cov - cov) <= 5 * se_cov).all()
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_small_m_and_m_zero(dtype):
    fk, X, _ = _model(300, D, 0.5, dtype, noise_over_amp=1e-2 if dtype == np.float64 else F32_NOISE)
    lib = _lib.load()
    sfx = "f64" if dtype == np.float64 else "f32"
    empty = np.zeros(4, dtype=dtype)
    amin = np.full(2, -7, np.int32)
    info = C.c_int(-1)
    ip = amin.ctypes.data_as(C.POINTER(C.c_int))
    assert getattr(lib, f"hbegp_predict_cov_{sfx}")(fk._h, _lib.aptr(empty), 0, 0.0, None, None) == _lib.OK
    assert getattr(lib, f"hbegp_sample_posterior_{sfx}")(fk._h, None, 0, None, 2, 0.0, None, ip, C.byref(info)) == _lib.OK
    assert (amin == -7).all() and info.value == 0
    bar = 1e-8 if dtype == np.float64 else 1e-4
    for m in (1, 2, 7, 8):
        Xs = _candidates(m, D, 30 + m).astype(dtype)
        mean, cov = fk.predict_cov(Xs)
        assert float(np.abs(cov.astype(np.float64) - _ref(fk, X, Xs)).max()) / fk.amplitude <= bar
        z = E.RNG(m).standard_normal((5, m)).astype(dtype)
        samples, argmin = fk.sample_posterior(Xs, z)
        assert np.isfinite(samples).all() and np.array_equal(argmin, np.argmin(samples, axis=1))
    fk.release()


def test_training_rows_and_duplicates_factor_in_f64():
    fk, X, _ = _model(500, D, 2.5, np.float64)
    q = _candidates(20, D, 4)
    Xs = np.vstack([X[:10], q, q[:7], X[:3]])  # query rows on training points, and rows repeated
    mean, cov = fk.predict_cov(Xs)
    assert float(np.abs(cov - _ref(fk, X, Xs)).max()) / fk.amplitude <= 1e-8
    z = E.RNG(17).standard_normal((32, len(Xs)))
    samples, argmin = fk.sample_posterior(Xs, z)
    assert np.isfinite(samples).all()
    assert np.array_equal(argmin, np.argmin(samples, axis=1))
    # rows that are the same point get the same draw up to the 1e-5 floor's share
    assert np.abs(samples[:, 10:17] - samples[:, 30:37]).max() <= 10 * math.sqrt(1e-5) * np.abs(z).max()
    fk.release()


def test_not_positive_definite_in_f32_is_reported_and_writes_nothing():
    # many copies of one point in f32: Sigma's smallest eigenvalue (1e-5) is below what f32 resolves beside c, so the factor
    # may fail.  Either it succeeds, or it reports HBEGP_NOT_PD with the failing pivot and leaves the outputs alone; a jitter
    # of the amplitude's size always factors.
    fk, X, _ = _model(300, D, 2.5, np.float32, noise_over_amp=1e-3)
    lib = _lib.load()
    m, S = 256, 3
    Xs = np.repeat(_candidates(2, D, 6), m // 2, axis=0).astype(np.float32)
    z = np.ones((S, m), np.float32)
    samples = np.full((S, m), 42.0, np.float32)
    amin = np.full(S, -7, np.int32)
    info = C.c_int(-1)
    rc = lib.hbegp_sample_posterior_f32(fk._h, _lib.fptr(Xs), m, _lib.fptr(z), S, 0.0, _lib.fptr(samples),
                                        amin.ctypes.data_as(C.POINTER(C.c_int)), C.byref(info))
    print(f"f32, {m} rows of 2 points, jitter 0: rc {rc}, info {info.value}")
    if rc == _lib.NOT_PD:
        assert 1 <= info.value <= m and (samples == 42.0).all() and (amin == -7).all()
        with pytest.raises(_lib.HbegpError) as e:
            fk.sample_posterior(Xs, z)
        assert e.value.code == _lib.NOT_PD
    else:
        assert rc == _lib.OK and info.value == 0
    s2, a2 = fk.sample_posterior(Xs, z, jitter=1.0)
    assert np.isfinite(s2).all() and np.array_equal(a2, np.argmin(s2, axis=1))
    fk.release()


def test_wrong_arguments_on_a_real_model():
    lib = _lib.load()
    fk, X, _ = _model(100, 2, 2.5, np.float64)
    Xs = _candidates(3, 2, 1)
    z, out, cov = np.zeros((2, 3)), np.zeros(6), np.zeros(9)
    amin = np.zeros(2, np.int32)
    ip = amin.ctypes.data_as(C.POINTER(C.c_int))
    d, f = _lib.dptr, _lib.fptr

    def einval(rc, what):
        assert rc == _lib.EINVAL and what in _lib.last_error(), _lib.last_error()

    Xf, zf = Xs.astype(np.float32), z.astype(np.float32)
    einval(lib.hbegp_predict_cov_f32(fk._h, f(Xf), 3, 0.0, None, f(Xf)), "f64 data")
    einval(lib.hbegp_sample_posterior_f32(fk._h, f(Xf), 3, f(zf), 2, 0.0, None, ip, None), "f64 data")
    bad = Xs.copy()
    bad[1, 1] = math.nan
    einval(lib.hbegp_predict_cov_f64(fk._h, d(bad), 3, 0.0, None, d(cov)), "non-finite coordinate")
    bad[1, 1] = math.inf
    einval(lib.hbegp_sample_posterior_f64(fk._h, d(bad), 3, d(z), 2, 0.0, d(out), ip, None), "non-finite coordinate")
    einval(lib.hbegp_sample_posterior_f64(fk._h, d(Xs), 3, d(z), 0, 0.0, d(out), ip, None), "S must be")
    einval(lib.hbegp_sample_posterior_f64(fk._h, d(Xs), -1, d(z), 2, 0.0, d(out), ip, None), "m must be")
    einval(lib.hbegp_sample_posterior_f64(fk._h, d(Xs), 3, None, 2, 0.0, d(out), ip, None), "z is NULL")
    einval(lib.hbegp_sample_posterior_f64(fk._h, d(Xs), 3, d(z), 2, -1.0, d(out), ip, None), "jitter")
    einval(lib.hbegp_sample_posterior_f64(fk._h, d(Xs), 3, d(z), 2, math.nan, d(out), ip, None), "jitter")
    einval(lib.hbegp_sample_posterior_f64(fk._h, d(Xs), 3, d(z), 2, 0.0, None, None, None), "both NULL")
    einval(lib.hbegp_predict_cov_f64(fk._h, d(Xs), 3, 0.0, None, None), "cov is NULL")
    fk.release()


def test_repeated_calls_and_threads_give_the_same_bits():
    fk, X, _ = _model(700, D, 2.5, np.float64)
    Xs = [_candidates(50 + 100 * i, D, 40 + i) for i in range(4)]
    zs = [E.RNG(i).standard_normal((16, len(x))) for i, x in enumerate(Xs)]
    ref = [(fk.predict_cov(x), fk.sample_posterior(x, z)) for x, z in zip(Xs, zs)]
    again = [(fk.predict_cov(x), fk.sample_posterior(x, z)) for x, z in zip(Xs, zs)]
    got = [None] * 4

    def run(i):
        for _ in range(3):
            got[i] = (fk.predict_cov(Xs[i]), fk.sample_posterior(Xs[i], zs[i]))

    ts = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i in range(4):
        for other in (again[i], got[i]):
            (m0, c0), (s0, a0) = ref[i]
            (m1, c1), (s1, a1) = other
            assert m0.tobytes() == m1.tobytes() and c0.tobytes() == c1.tobytes(), i
            assert s0.tobytes() == s1.tobytes() and a0.tobytes() == a1.tobytes(), i
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_m_8192_leaves_predict_unchanged(dtype):
    fk, X, _ = _model(1024, D, 2.5, dtype, noise_over_amp=1e-2 if dtype == np.float64 else F32_NOISE)
    probe = _candidates(500, D, 50).astype(dtype)
    before = fk.predict(probe)
    m = 8192
    Xs = _candidates(m, D, 51).astype(dtype)
    z = E.RNG(8192).standard_normal((4, m)).astype(dtype)
    _, argmin = fk.sample_posterior(Xs, z, want_samples=False)
    samples, argmin2 = fk.sample_posterior(Xs, z)
    assert np.isfinite(samples).all() and np.array_equal(argmin, argmin2)
    assert np.array_equal(argmin, np.argmin(samples, axis=1))
    after = fk.predict(probe)
    for u, v in zip(before[:2], after[:2]):
        assert u.tobytes() == v.tobytes()
    fk.release()


def _estimator_model(projection, d=3, n=120, seed=4):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = ((X - 0.37) ** 2).sum(axis=1) + 0.5
    est = E.EstimatorGPR.new(d).y_projection(projection)
    return est.estimate(X, y, None, E.RNG.new_with_seed(seed))


@pytest.mark.parametrize("projection", ["logarithmic", "linear"])
def test_thompson_indices_are_those_of_the_normalised_draws(projection):
    model = _estimator_model(projection)
    cand = np.random.default_rng(9).uniform(0, 1, (200, 3))
    k = 12
    idx = E.acquire_by_thompson(cand, model, k, E.RNG(77))
    proj = model.sample_a(cand, k, E.RNG(77))  # same normals: same draws, projected
    assert proj.shape == (k, 200) and np.isfinite(proj).all()
    assert np.array_equal(idx, np.argmin(proj, axis=1))
    z = E.RNG(77).standard_normal((k, 200))
    norm, amin = model.fitted.sample_posterior(cand, z)
    assert np.array_equal(idx, amin) and np.array_equal(idx, np.argmin(norm, axis=1))
    assert np.allclose(proj, model.y_norm.project_location_from_normalized(norm), rtol=0, atol=0)
