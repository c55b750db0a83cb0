"""GPU: Monte Carlo batch expected improvement and its batch maximiser (hbegp_qei_* / hbegp_maximize_qei_*).

The device against the NumPy restatement (tests/qei_ref.py) over the Matern orders, sizes, batch shapes, draw counts and jitters; q = 1
against hbegp_predict_grad through the closed form; Sigma against hbegp_predict_cov; the device's gradient against central differences
of its own qEI; bits (repeat, batch alone vs within 200, threads); the argument checks that need a model; the maximiser's contract and
its advantage over the greedy kriging-believer batch; the estimator's opt-in acquire_by_qei."""
import math
import threading

import numpy as np
import pytest

import qei_ref as QR
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

NUS = [0.5, 1.5, 2.5, math.inf]
D = 4
# f32: a noise of the amplitude's size keeps cond(K) <= n + 1 (tests/test_gpu_posterior_cov.py)
F32_NOISE = 1.0
AMP = 1.3


def _data(n, dtype, seed=1, d=D):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    X, y = X.astype(dtype), y.astype(dtype)
    noise_over_amp = 1e-2 if dtype == np.float64 else F32_NOISE
    theta = np.log(np.concatenate([[noise_over_amp * AMP, AMP], np.linspace(0.3, 0.9, d)]))
    return X, y, theta


def _model(n, nu, dtype, seed=1, d=D):
    X, y, theta = _data(n, dtype, seed, d)
    fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    noise, amp, ell = fk.device_params()
    post = QR.Posterior(X, y, amp, ell, nu, noise)
    return fk, X, y, post


def _batches(B, q, seed, dtype, d=D):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (B, q, d)).astype(dtype)


def _normals(S, q, seed, dtype):
    return np.random.default_rng(seed).standard_normal((S, q)).astype(dtype)


def _fmin(y):
    return float(np.min(y)) + 0.2  # a little above the best observation: most batches improve on some draws


def _check(fk, post, Xb, z, fmin, jitter, tol):
    qei, grad, info = fk.qei(Xb, z, fmin, jitter=jitter)
    assert (info == 0).all(), info
    rq, rg = QR.qei_many(post, Xb.astype(np.float64), z.astype(np.float64), fmin, jitter)
    c = post.amp
    dq = np.abs(qei - rq).max()
    assert dq <= tol * max(1.0, math.sqrt(c)), (dq, qei, rq)
    worst = 0.0
    for b in range(len(Xb)):
        scale = max(1.0, float(np.abs(rg[b]).max()))
        dev = float(np.abs(grad[b].astype(np.float64) - rg[b]).max()) / scale
        worst = max(worst, dev)
        assert dev <= tol, (b, dev)
    return dq, worst


# (q, B, S) shapes of the f64 comparison; q = 64 and B = 200 keep the restatement's time in bounds
SHAPES64 = [(1, 7, 2048), (2, 200, 128), (10, 7, 2048), (10, 1, 1), (64, 1, 128), (64, 7, 2048)]


@pytest.mark.parametrize("n", [100, 300, 1000])
@pytest.mark.parametrize("nu", NUS)
def test_device_matches_restatement_f64(nu, n):
    fk, X, y, post = _model(n, nu, np.float64, seed=n)
    fmin = _fmin(y)
    worst = np.zeros(2)
    for i, (q, B, S) in enumerate(SHAPES64):
        for jitter in (0.0, 1e-6):
            Xb = _batches(B, q, 100 * n + i, np.float64)
            z = _normals(S, q, 7 + i, np.float64)
            worst = np.maximum(worst, _check(fk, post, Xb, z, fmin, jitter, 1e-8))
    print(f"f64 nu={nu} n={n}: qei {worst[0]:.1e} grad {worst[1]:.1e}")
    fk.release()


# f32: seeds whose restated draws stay > 1e-3 sqrt(c) away from every kink (top-two gap, fmin - f_min); asserted below
SHAPES32 = [(1, 7, 128), (2, 7, 128), (10, 1, 64), (4, 7, 16)]


@pytest.mark.parametrize("n", [100, 300, 1000])
@pytest.mark.parametrize("nu", NUS)
def test_device_matches_restatement_f32(nu, n):
    fk, X, y, post = _model(n, nu, np.float32, seed=n)
    assert (n * post.amp + post.noise) / post.noise <= 4.1e3
    fmin = _fmin(y)
    worst = np.zeros(2)
    checked = 0
    for i, (q, B, S) in enumerate(SHAPES32):
        for jitter in (0.0, 1e-6):
            for seed in range(40):
                Xb = _batches(B, q, 1000 * n + 10 * i + seed, np.float32)
                z = _normals(S, q, 7 + i, np.float32)
                gaps = [QR.top_two_gap(post, xb.astype(np.float64), z.astype(np.float64), fmin, jitter) for xb in Xb]
                if min(min(g) for g in gaps) > 1e-3 * math.sqrt(post.amp):
                    break
            else:
                raise AssertionError(f"no seed keeps q={q} B={B} S={S} away from the kinks")
            worst = np.maximum(worst, _check(fk, post, Xb, z, fmin, jitter, 1e-4))
            checked += 1
    assert checked == 2 * len(SHAPES32)
    print(f"f32 nu={nu} n={n}: qei {worst[0]:.1e} grad {worst[1]:.1e}")
    fk.release()


# f32 at the largest shapes: q = 64, S = 2048 and B = 200.  fmin lies midway between the 8th and 9th smallest restated draw
# minimum over the whole call, so that eight draws improve and every draw keeps away from the fmin kink; the batch seed is searched
# until the top-two gaps of the improving draws clear the same bar as above (asserted)
SHAPES32_LARGE = [(64, 1, 2048), (64, 7, 256), (10, 200, 128)]


def test_device_matches_restatement_f32_large_shapes():
    fk, X, y, post = _model(300, 2.5, np.float32, seed=301)
    worst = np.zeros(2)
    for q, B, S in SHAPES32_LARGE:
        z = _normals(S, q, 60 + q + B, np.float32)
        z64 = z.astype(np.float64)
        for seed in range(40):
            Xb = _batches(B, q, 7000 + 100 * q + B + seed, np.float32)
            mins = np.sort(np.concatenate([QR.draw_values(post, xb.astype(np.float64), z64).min(axis=1) for xb in Xb]))
            fmin = float(0.5 * (mins[7] + mins[8]))
            gaps = [QR.top_two_gap(post, xb.astype(np.float64), z64, fmin) for xb in Xb]
            if min(min(g) for g in gaps) > 1e-3 * math.sqrt(post.amp):
                break
        else:
            raise AssertionError(f"no seed keeps q={q} B={B} S={S} away from the kinks")
        worst = np.maximum(worst, _check(fk, post, Xb, z, fmin, 0.0, 1e-4))
    print(f"f32 large shapes: qei {worst[0]:.1e} grad {worst[1]:.1e}")
    fk.release()


# A coordinate that is finite but overflows when divided by a length scale (1e308 in f64, 3e38 in f32) makes the point's Kstar
# row NaN (inf * exp(-inf) in the Matern 5/2 map), so its Q row and its column of Sigma are NaN and the batch's factor fails
# deterministically at that point's column.  The rows of the other batches are computed from their own points only.
def _huge(dtype):
    return 1e308 if dtype == np.float64 else 3e38


@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_failed_batches_report_and_leave_the_others_alone(dtype, want_grad):
    fk, X, y, post = _model(300, 2.5, dtype, seed=14)
    fmin = _fmin(y)
    Xb = _batches(6, 5, 41, dtype)
    Xb[1, 2, 1] = _huge(dtype)
    Xb[4, 0, 3] = _huge(dtype)
    z = _normals(256, 5, 42, dtype)
    qei, grad, info = fk.qei(Xb, z, fmin, want_grad=want_grad)
    assert info.tolist() == [0, 3, 0, 0, 1, 0], info
    assert math.isnan(qei[1]) and math.isnan(qei[4])
    good = [0, 2, 3, 5]
    assert np.isfinite(qei[good]).all()
    if want_grad:
        assert (grad[1] == 0).all() and (grad[4] == 0).all()
        assert np.isfinite(grad[good]).all()
    else:
        assert grad is None
    solo_q, solo_g, solo_i = fk.qei(Xb[good], z, fmin, want_grad=want_grad)
    assert (solo_i == 0).all() and solo_q.tobytes() == qei[good].tobytes()
    if want_grad:
        assert solo_g.tobytes() == grad[good].tobytes()
    with pytest.raises(_lib.HbegpError) as e:
        fk.qei(Xb, z, fmin, want_grad=want_grad, raise_not_pd=True)
    assert e.value.code == _lib.NOT_PD and "batch 1" in str(e.value)
    # the same through the C ABI with info = NULL: NOT_PD, every output written
    lib = _lib.load()
    sfx = "f64" if dtype == np.float64 else "f32"
    q2 = np.full(6, -7.0)
    rc = getattr(lib, f"hbegp_qei_{sfx}")(fk._h, _lib.aptr(_lib.as_c(Xb, dtype)), 6, 5, _lib.aptr(z), 256, float(fmin), 0.0,
                                         _lib.dptr(q2), None, None)
    assert rc == _lib.NOT_PD and q2[good].tobytes() == qei[good].tobytes() and np.isnan(q2[[1, 4]]).all()
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_maximiser_treats_a_failed_batch_as_a_failed_evaluation(dtype):
    fk, X, y, post = _model(300, 2.5, dtype, seed=15)
    fmin = _fmin(y)
    lo, hi = np.full(D, -0.1), np.full(D, 1.1)
    starts = np.random.default_rng(3).uniform(0, 1, (4, 3, D)).astype(dtype)
    starts[2, 1, 2] = _huge(dtype)
    hi[2] = float(starts[2, 1, 2])  # room for a start that fails (the element type's own value)
    z = _normals(256, 3, 43, dtype)
    q0, _, i0 = fk.qei(starts, z, fmin, want_grad=False)
    assert i0.tolist() == [0, 0, 2, 0]
    x, qv, ne = fk.maximize_qei(starts, lo, hi, z, fmin, maxeval=30)
    assert _lib.last_error() == ""  # the failed rounds left no error behind a call that succeeded
    assert qv[2] == -np.inf and ne[2] == 1 and x[2].tobytes() == starts[2].tobytes()
    for r in (0, 1, 3):
        assert np.isfinite(qv[r]) and qv[r] >= q0[r] and 1 <= ne[r] <= 30
        assert (x[r] >= lo).all() and (x[r] <= hi).all()
    fk.release()


@pytest.mark.parametrize("nu", NUS)
def test_q1_is_the_closed_form_of_predict_grad(nu):
    fk, X, y, post = _model(300, nu, np.float64, seed=5)
    fmin = _fmin(y)
    x = _batches(20, 1, 9, np.float64)
    z = _normals(512, 1, 3, np.float64)
    qei, grad, info = fk.qei(x, z, fmin)
    mean, var, dmean, dvar, _ = fk.predict_with_gradient(x[:, 0, :])
    for b in range(20):
        sd = math.sqrt(var[b])
        f = mean[b] + sd * z[:, 0]
        act = f < fmin
        ref = np.maximum(fmin - f, 0.0).sum() / len(z)
        rg = (-dmean[b][None, :] - z[act, 0][:, None] * dvar[b][None, :] / (2 * sd)).sum(axis=0) / len(z)
        assert abs(qei[b] - ref) <= 1e-12 * max(1.0, abs(ref)), (b, qei[b], ref)
        assert np.abs(grad[b, 0] - rg).max() <= 1e-12 * max(1.0, np.abs(rg).max()), (b, grad[b, 0], rg)
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sigma_is_predict_cov(dtype):
    fk, X, y, post = _model(300, 2.5, dtype, seed=6)
    fmin = _fmin(y)
    Xb = _batches(5, 10, 12, dtype)
    z = _normals(1024, 10, 13, dtype)
    qei, _, _ = fk.qei(Xb, z, fmin, jitter=1e-6, want_grad=False)
    for b in range(5):
        mean, cov = fk.predict_cov(Xb[b], jitter=1e-6)
        ref = QR.qei_from(mean.astype(np.float64), cov.astype(np.float64), z.astype(np.float64), fmin)
        tol = 1e-10 if dtype == np.float64 else 1e-4
        assert abs(qei[b] - ref) <= tol * max(1.0, abs(ref)), (b, qei[b], ref)
    fk.release()


@pytest.mark.parametrize("nu", [1.5, 2.5, math.inf])
def test_gradient_is_the_derivative_of_the_device_qei(nu):
    fk, X, y, post = _model(300, nu, np.float64, seed=8)
    fmin = _fmin(y)
    xb = _batches(1, 6, 21, np.float64)
    z = _normals(256, 6, 22, np.float64)
    qei, grad, _ = fk.qei(xb, z, fmin)
    h = 1e-6
    plus, minus = [], []
    for a in range(6):
        for k in range(D):
            xp, xm = xb.copy(), xb.copy()
            xp[0, a, k] += h
            xm[0, a, k] -= h
            plus.append(xp[0])
            minus.append(xm[0])
    qp, _, _ = fk.qei(np.stack(plus), z, fmin, want_grad=False)
    qm, _, _ = fk.qei(np.stack(minus), z, fmin, want_grad=False)
    fd = ((qp - qm) / (2 * h)).reshape(6, D)
    rel = np.abs(fd - grad[0]).max() / np.abs(grad[0]).max()
    print(f"nu={nu}: finite differences vs gradient {rel:.1e}")
    assert rel <= 1e-5, rel
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bits_repeat_batch_alone_and_threads(dtype):
    fk, X, y, post = _model(1000, 2.5, dtype, seed=4)
    fmin = _fmin(y)
    Xb = _batches(200, 10, 31, dtype)
    z = _normals(256, 10, 32, dtype)
    q1, g1, _ = fk.qei(Xb, z, fmin)
    q2, g2, _ = fk.qei(Xb, z, fmin)
    assert q1.tobytes() == q2.tobytes() and g1.tobytes() == g2.tobytes()
    for b in (0, 77, 199):
        qa, ga, _ = fk.qei(Xb[b], z, fmin)
        assert qa.tobytes() == q1[b:b + 1].tobytes() and ga[0].tobytes() == g1[b].tobytes(), b
    out = [None] * 4

    def run(t):
        out[t] = [fk.qei(Xb[t * 50:(t + 1) * 50], z, fmin)[:2] for _ in range(3)]

    ths = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    for t in range(4):
        for qv, gv in out[t]:
            assert qv.tobytes() == q1[t * 50:(t + 1) * 50].tobytes() and gv.tobytes() == g1[t * 50:(t + 1) * 50].tobytes(), t
    fk.release()


def test_checks_that_need_a_model():
    fk, X, y, post = _model(100, 2.5, np.float64, seed=2)
    lib = _lib.load()
    Xb = _batches(2, 3, 1, np.float64)
    z = _normals(8, 3, 2, np.float64)
    out, grad = np.zeros(2), np.zeros((2, 3, D))
    f32 = Xb.astype(np.float32)
    rc = lib.hbegp_qei_f32(fk._h, _lib.fptr(f32), 2, 3, _lib.fptr(z.astype(np.float32)), 8, 0.0, 0.0, _lib.dptr(out), None, None)
    assert rc == _lib.EINVAL and "f64" in _lib.last_error()
    bad = Xb.copy()
    bad[1, 2, 3] = math.nan
    rc = lib.hbegp_qei_f64(fk._h, _lib.dptr(bad), 2, 3, _lib.dptr(z), 8, 0.0, 0.0, _lib.dptr(out), _lib.dptr(grad), None)
    assert rc == _lib.EINVAL and "non-finite" in _lib.last_error()
    rc = lib.hbegp_qei_f64(fk._h, _lib.dptr(Xb), 0, 3, _lib.dptr(z), 8, 0.0, 0.0, None, None, None)
    assert rc == _lib.OK  # B = 0: a no-op
    lo, hi = np.zeros(D), np.ones(D)
    starts = np.full((1, 3, D), 0.5)
    starts[0, 1, 2] = 1.5
    x, qv, ne = np.zeros_like(starts), np.zeros(1), np.zeros(1, np.int32)
    rc = lib.hbegp_maximize_qei_f64(fk._h, _lib.dptr(starts), 1, 3, _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(z), 8, 0.0, 0.0, 10,
                                    _lib.dptr(x), _lib.dptr(qv), None)
    assert rc == _lib.EINVAL and "outside the box" in _lib.last_error()
    fk.release()


@pytest.mark.parametrize("d", [2, 8])
@pytest.mark.parametrize("q", [3, 10])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_maximiser_contract(dtype, q, d):
    fk, X, y, post = _model(300, 2.5, dtype, seed=10 + d, d=d)
    fmin = _fmin(y)
    lo, hi = np.zeros(d), np.ones(d)
    starts = np.random.default_rng(q + d).uniform(0, 1, (8, q, d)).astype(dtype)
    z = _normals(256, q, 40 + q, dtype)
    q0, _, _ = fk.qei(starts, z, fmin, want_grad=False)
    x, qv, ne = fk.maximize_qei(starts, lo, hi, z, fmin, maxeval=60)
    assert x.dtype == dtype and x.shape == starts.shape
    assert (x >= lo).all() and (x <= hi).all()
    assert (ne >= 1).all() and (ne <= 60).all()
    assert (qv >= q0).all(), (qv, q0)
    qa, _, _ = fk.qei(x, z, fmin)
    assert qa.tobytes() == qv.tobytes()
    print(f"{np.dtype(dtype).name} q={q} d={d}: qEI {q0.max():.4g} -> {qv.max():.4g}, evaluations {ne.min()}..{ne.max()}")
    fk.release()


def test_maximised_batch_beats_the_greedy_batch():
    fk, X, y, post = _model(60, 2.5, np.float64, seed=3, d=2)
    fmin = _fmin(y)
    cand = np.random.default_rng(5).uniform(0, 1, (4096, 2))
    idx, _, _, _ = fk.select_batch(cand, 4, fmin)
    greedy = cand[idx][None]
    z = _normals(1024, 4, 6, np.float64)
    qg, _, _ = fk.qei(greedy, z, fmin, want_grad=False)
    starts = np.concatenate([greedy, np.random.default_rng(7).uniform(0, 1, (7, 4, 2))])
    x, qv, _ = fk.maximize_qei(starts, np.zeros(2), np.ones(2), z, fmin)
    best, _, _ = fk.qei(x[np.argmax(qv)], z, fmin, want_grad=False)
    print(f"greedy kriging believer {qg[0]:.6g}, maximised {best[0]:.6g}")
    assert best[0] >= qg[0]
    fk.release()


def test_estimator_acquire_by_qei():
    rng = np.random.default_rng(0)
    X = rng.uniform(-2, 2, (80, 2))
    y = (X ** 2).sum(axis=1) + 0.05 * rng.standard_normal(80)
    est = E.EstimatorGPR.new(2)
    model = est.estimate(X, y, None, E.RNG(1))
    cand = rng.uniform(-2, 2, (500, 2))
    x, v = E.acquire_by_qei(cand, model, 5, float(y.min()), E.RNG(3), n_samples=256, n_restarts=4, maxeval=40)
    assert x.shape == (5, 2) and math.isfinite(v) and v >= 0
    assert (x >= cand.min(axis=0)).all() and (x <= cand.max(axis=0)).all()
