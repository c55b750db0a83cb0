"""GPU: the factor of Sigma inside hbegp_sample_posterior_* at every depth of the recursion, and batch selection past the LDS
staging of its conditioning vectors.

The draws are mean + L z with L the device's lower Cholesky factor of Sigma (include/hbegp.h).  On a model whose training
targets are all zero the mean is exactly 0, and with z = I_m draw s is column s of the device's L, bit for bit (every product
is by 0 or 1): its structure, its backward error against the engine's Sigma and its forward error against an fp64 Cholesky, at
m from one to 33 blocks of 128.  Then random draws against mean + cholesky(Sigma) z at many row tiles of z and at m = 8192;
argmin ties spread over the epilogue's threads; and hbegp_select_batch_* at k = 4100, beyond the first BSEL_CJ = 4096 steps
whose conditioning entries the kernel stages in the LDS."""
import math
import time

import numpy as np
import pytest

import batch_select_ref as BS
import posterior_cov_ref as PC
from hbetune_rs_amd import gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

D = 4
# f32: a noise of the amplitude's size keeps cond(K) <= n + 1 (tests/test_gpu_posterior_cov.py)
F32_NOISE = 1.0


def _data(n, d, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    return X.astype(dtype), y.astype(dtype)


def _model(n, nu, dtype, seed=1, zero_y=False, noise_over_amp=None):
    """The set-up of tests/test_gpu_posterior_cov.py: d = 4, amplitude 1.3, noise 1e-2 c (f64) or F32_NOISE c (f32)."""
    X, y = _data(n, D, seed, dtype)
    if zero_y:
        y = np.zeros_like(y)  # alpha = K^-1 0 = 0: the posterior mean is exactly 0
    if noise_over_amp is None:
        noise_over_amp = 1e-2 if dtype == np.float64 else F32_NOISE
    amp = 1.3
    theta = np.log(np.concatenate([[noise_over_amp * amp, amp], np.linspace(0.3, 0.9, D)]))
    return gpr.FittedKernel.extend(X, y, theta, nu=nu), X, y


def _candidates(m, seed, dtype=np.float64):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (m, D)).astype(dtype)


def _device_factor(fk, Xs, jitter):
    """The device's L in fp64: with mean 0 and z = I_m, draw s is column s of L."""
    m = len(Xs)
    samples, argmin = fk.sample_posterior(Xs, np.eye(m, dtype=fk.dtype), jitter=jitter)
    assert np.array_equal(argmin, np.argmin(samples, axis=1))
    return samples.T.astype(np.float64)


# m -> nbm = ceil(m / 128): 1, 2, 2, 3, 5, 8, 9, 12, 17, 33 blocks; ragged and exact tile edges, odd splits, and up to six
# levels of the recursion, where the left half has more than one block (the need_x branch, L21 read from its own buffer)
F64_M = [128, 129, 255, 257, 513, 900, 1100, 1409, 2049, 4097]
F32_M = [129, 257, 513, 1100, 2049]
CASES = [(np.float64, m) for m in F64_M] + [(np.float32, m) for m in F32_M]


@pytest.mark.parametrize("nu", [0.5, 2.5])
@pytest.mark.parametrize("dtype,m", CASES, ids=[f"{np.dtype(t).name}-m{m}" for t, m in CASES])
def test_device_factor_is_the_cholesky_factor_of_sigma(dtype, m, nu):
    fk, X, _ = _model(500, nu, dtype, zero_y=True)
    c = fk.amplitude
    Xs = _candidates(m, 100 + m, dtype)
    f64 = dtype == np.float64
    # (jitter, forward error checked).  The eigenvalues of Sigma lie between 1e-5 + jitter and about m c + jitter: at
    # jitter 1e-2 c, cond(Sigma) <= about 100 m (f64); at jitter c, about m + 1 (f32).  At jitter 0 (f64) cond(Sigma) is
    # unbounded, so there only the structure and the backward error, which hold at any cond, are checked.  f32 at jitter 0 may
    # legitimately be HBEGP_NOT_PD (test_not_positive_definite_in_f32_is_reported_and_writes_nothing).
    runs = [(0.0, False), (1e-2 * c, True)] if f64 else [(c, True)]
    sig_bar = 1e-8 if f64 else 1e-4  # the bars of test_sigma_parity_with_the_restatement
    # measured over both orders and every m: backward <= 4.1e-15 (f64, m = 4097) and 1.6e-7 (f32); forward <= 1.0e-14 (f64,
    # m = 4097) and 1.2e-7 (f32).  The bars leave 25x (f64 backward), 100x (f64 forward) and 60x (f32) room
    back_bar = 1e-13 if f64 else 1e-5
    fwd_bar = 1e-12 if f64 else 1e-5
    for jitter, forward in runs:
        mean, sig = fk.predict_cov(Xs, jitter=jitter)
        assert (mean == 0).all()
        S = sig.astype(np.float64)
        dsig = float(np.abs(S - PC.sigma_ref(Xs, X, c, fk.length_scale, fk.nu, fk.noise, jitter=jitter)).max()) / c
        L = _device_factor(fk, Xs, jitter)
        # exact structure: zeros above the diagonal (the diagonal blocks' mask, no stale numbers in the factor's buffers)
        assert not np.triu(L, 1).any(), np.argwhere(np.triu(L, 1) != 0)[:5]
        dg = np.diag(L)
        assert np.isfinite(L).all() and (dg > 0).all()
        back = float(np.abs(L @ L.T - S).max()) / float(np.diag(S).max())
        msg = f"{np.dtype(dtype).name} nu={nu} m={m} jitter={jitter / c:g}c: Sigma {dsig:.2e} backward {back:.2e}"
        if forward:
            fwd = float(np.abs(L - np.linalg.cholesky(S)).max()) / math.sqrt(c)
            msg += f" forward {fwd:.2e}"
        print(msg)
        assert dsig <= sig_bar, dsig
        assert back <= back_bar, back
        if forward:
            assert fwd <= fwd_bar, fwd
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", [900, 2049])
def test_draws_with_many_row_tiles_of_z(m, dtype):
    fk, X, _ = _model(500, 1.5, dtype)
    c = fk.amplitude
    f64 = dtype == np.float64
    Xs = _candidates(m, 200 + m, dtype)
    for jitter in ((0.0, 1e-2 * c) if f64 else (c,)):
        mean, cov = fk.predict_cov(Xs, jitter=jitter)
        assert np.abs(mean).max() > 0
        for S in (129, 300):
            z = E.RNG(S * 7 + m).standard_normal((S, m)).astype(dtype)
            samples, argmin = fk.sample_posterior(Xs, z, jitter=jitter)
            want = PC.draws_ref(mean, cov, z)
            dev = float(np.abs(samples.astype(np.float64) - want).max()) / (math.sqrt(c) * float(np.abs(z).max()))
            print(f"{np.dtype(dtype).name} m={m} S={S} jitter={jitter / c:g}c: draws vs mean + chol(Sigma) z: {dev:.2e}")
            # the bars of test_draws_are_mean_plus_cholesky_of_the_engines_sigma; measured <= 1.1e-14 (f64) and 1.9e-7 (f32)
            assert dev <= (1e-10 if f64 else 1e-5), dev
            assert np.array_equal(argmin, np.argmin(samples, axis=1))
    fk.release()


def test_m_8192_draws_match_the_reference():
    fk, X, _ = _model(1024, 2.5, np.float64)
    m = 8192
    Xs = _candidates(m, 51)
    z = E.RNG(8192).standard_normal((6, m))
    mean, cov = fk.predict_cov(Xs)
    samples, argmin = fk.sample_posterior(Xs, z)
    want = PC.draws_ref(mean, cov, z)
    dev = float(np.abs(samples - want).max()) / (math.sqrt(fk.amplitude) * float(np.abs(z).max()))
    print(f"f64 m=8192 S=6: draws vs mean + chol(Sigma) z: {dev:.2e}")  # measured 1.5e-13
    assert dev <= 1e-10, dev
    assert np.array_equal(argmin, np.argmin(samples, axis=1))
    fk.release()


def test_argmin_ties_across_the_epilogues_threads():
    # sample_epilogue_kernel: thread t scans rows t, t + 256, ...; then a fixed tree over the 256 threads.  The best point at
    # rows 200, 260 and 700 sits on threads 200, 4 and 188: the lowest index is on the highest thread
    fk, X, _ = _model(300, 2.5, np.float64)
    m, rows = 800, [200, 260, 700]
    pool = _candidates(m - 2, 9)
    pm, _, _ = fk.predict(pool)
    b = int(np.argmin(pm))
    rest = np.ones(m, bool)
    rest[rows] = False
    Xs = np.empty((m, D))
    Xs[rows] = pool[b]
    Xs[rest] = np.delete(pool, b, axis=0)
    z = np.zeros((4, m))
    samples, argmin = fk.sample_posterior(Xs, z)
    assert (samples[:, 200] == samples[:, 260]).all() and (samples[:, 200] == samples[:, 700]).all()
    assert (samples[:, 200] < samples[:, rest].min(axis=1)).all()
    assert (argmin == 200).all(), argmin
    _, argmin2 = fk.sample_posterior(Xs, z, want_samples=False)
    assert (argmin2 == 200).all(), argmin2
    fk.release()


# batch_select_kernel stages C[s][j] of the first BSEL_CJ = 4096 earlier picks in the LDS and reads the rest from global memory:
# k = 4100 runs four steps through that second loop.  m = 4224 is 33 tiles of 128.  A noise of the amplitude's size keeps the
# 4100 rank-one updates well conditioned (every update divides by sqrt(r_j + s2) >= sqrt(c)).
@pytest.mark.parametrize("dtype,lie", [(np.float64, False), (np.float32, True)], ids=["f64-believer", "f32-lie"])
def test_batch_select_past_the_lds_staging(dtype, lie):
    m, k = 4224, 4100
    fk, X, y = _model(500, 2.5, dtype, seed=3, noise_over_amp=F32_NOISE)
    fmin = float(np.min(y))
    L = float(np.median(y)) if lie else None
    Xs = _candidates(m, 5, dtype)
    t0 = time.perf_counter()
    pidx, pei, _, _ = fk.select_batch(Xs, 4096, fmin, lie=L)
    t1 = time.perf_counter()
    idx, ei, _, _, devs = BS.replay(fk, Xs, k, fmin, L, dtype)
    t2 = time.perf_counter()
    print(f"{np.dtype(dtype).name} m={m} k={k} lie={lie}: pick gap {devs[0]:.1e} ei {devs[1]:.1e} mean {devs[2]:.1e} "
          f"var {devs[3]:.1e}; device k=4096 {t1 - t0:.1f} s, replay of k={k} (device + restatement) {t2 - t1:.1f} s")
    # the first t picks do not depend on k (include/hbegp.h), across the staging boundary too
    assert pidx.tobytes() == idx[:4096].tobytes() and pei.tobytes() == ei[:4096].tobytes()
    fk.release()
