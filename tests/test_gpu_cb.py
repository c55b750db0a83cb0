"""GPU: the confidence bound (hbegp_confidence_bound_* / hbegp_minimize_confidence_bound_*).

The device's cb and grad replayed through the NumPy restatement (tests/cb_ref.py) on the engine's own posteriors
(predict_with_gradient); best, mean and var bit for bit; kappa = 0; clamped variances; NaN rows; the arg-min around BSEL_THREADS =
1024; bits across batch sizes, positions, gradient on / off, repeats and threads; the refusals that need a model; the minimiser;
the estimator's suggest_optimum; the pool's poisons; the phase clock; the C++ mirror.  The models are
tests/feature_count_cases.py's recipe through FittedKernel.extend at a fixed theta.

Bars (tests/cb_ref.py): 1e-8 (f64) / 1e-4 (f32) times max(1, |reference value|) for cb; for the gradient times
max(1, |dmean| + |kappa| |dvar| / (2 sigma)) as well, row by row.  Measured deviations: DESIGN section 30."""
import ctypes as C
import math
import os
import subprocess
import threading

import numpy as np
import pytest

import cb_ref as R
import feature_count_cases as FC
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(n=40, d=2, nu=2.5, m=5, kappa=1.0)  # the base case every axis is varied against
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=lambda t: np.dtype(t).name)


def _model(n, d, nu, dtype):
    X, y, theta = FC.inputs(d, n, dtype)
    return gpr.FittedKernel.extend(X, y, theta, nu=nu)


def _candidates(m, d, seed, dtype):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (m, d)).astype(dtype)


def _compare(dtype, val, grad, mean, var, dmean, dvar, kappa):
    """The device's (cb, grad) against the restatement's on the same posteriors: deviation / bar of both.  Asserts both."""
    rv, rg, scale = R.cb_grad(mean, var, dmean, dvar, kappa)
    assert np.isfinite(rv).all() and np.isfinite(val).all()
    dev = float((np.abs(val - rv) / R.value_bar(dtype, rv)).max())
    gdev = float((np.abs(grad.astype(np.float64) - rg).max(axis=1) / R.grad_bar(dtype, rv, scale)).max())
    assert dev <= 1.0 and gdev <= 1.0, (dev, gdev)
    return dev, gdev


def _replay(fk, Xs, kappa):
    dtype, m, d = fk.dtype, len(Xs), fk.d
    val, best, grad, mean, var = fk.confidence_bound(Xs, kappa, want_grad=True, want_posterior=True)
    assert val.dtype == np.float64 and val.shape == (m,) and grad.dtype == dtype and grad.shape == (m, d)
    pmean, pvar, dmean, dvar, _ = fk.predict_with_gradient(Xs)
    assert mean.tobytes() == pmean.tobytes() and var.tobytes() == pvar.tobytes()  # hbegp_predict_grad_*'s bits
    r = _compare(dtype, val, grad, mean, var, dmean, dvar, kappa)
    assert best == R.argmin_first(val)
    # without a gradient: the same cb bits, and the batched predict's posterior
    val2, best2, mean2, var2 = fk.confidence_bound(Xs, kappa, want_posterior=True)
    assert val2.tobytes() == val.tobytes() and best2 == best
    if m > 16:
        bmean, bvar, _ = fk.predict(Xs)
        assert mean2.tobytes() == bmean.tobytes() and var2.tobytes() == bvar.tobytes()
    return r


def _axis_cases():
    """Every value of each axis against BASE.  d = 9 takes 16 lanes per row of which 7 idle, d = 64 a whole wave per row; m = 70 is
    the batched predict past m = 16, ragged over the gradient kernel's four rows; n = 130 lies beyond the 128-row regime."""
    cases = []
    for key, values in (("n", (40, 130)), ("d", (1, 2, 8, 9, 64)), ("nu", (0.5, 1.5, 2.5, math.inf)), ("m", (1, 3, 4, 5, 9, 70)),
                        ("kappa", (-2.0, 0.0, 1.0, 3.0))):
        for v in values:
            c = dict(BASE, **{key: v})
            if c not in cases:
                cases.append(c)
    return cases


@DTYPES
@pytest.mark.parametrize("case", _axis_cases(), ids=lambda c: "n%d-d%d-nu%s-m%d-k%g" % (c["n"], c["d"], c["nu"], c["m"], c["kappa"]))
def test_device_cb_replays_through_the_restatement(case, dtype):
    fk = _model(case["n"], case["d"], case["nu"], dtype)
    Xs = _candidates(case["m"], case["d"], 11, dtype)
    r = _replay(fk, Xs, case["kappa"])
    print(f"{np.dtype(dtype).name} {case}: deviation / bar: values {r[0]:.1e}, grad {r[1]:.1e}")
    fk.release()


@DTYPES
def test_kappa_zero_is_the_mean_and_its_gradient(dtype):
    fk = _model(40, 3, 2.5, dtype)
    Xs = _candidates(9, 3, 13, dtype)
    val, best, grad, mean, var = fk.confidence_bound(Xs, 0.0, want_grad=True, want_posterior=True)
    _, _, dmean, _, _ = fk.predict_with_gradient(Xs)
    assert val.tobytes() == mean.astype(np.float64).tobytes()  # mean widened to double
    assert grad.tobytes() == dmean.tobytes() and best == R.argmin_first(mean)
    fk.release()


def _clamped_model():
    """The f32 amplitude-1e4 model of tests/test_gpu_lcei.py at its own training rows: about half of the variances clamp to 0."""
    g = np.stack(np.meshgrid(np.linspace(0, 1, 8), np.linspace(0, 1, 8)), axis=-1).reshape(-1, 2)
    dtype, theta = np.float32, np.log([1e-4, 1e4, 0.05, 0.05])
    X, y = g.astype(dtype), (np.sin(3 * g).sum(axis=1) * 100.0).astype(dtype)
    return gpr.FittedKernel.extend(X, y, theta, nu=2.5), X


@pytest.mark.parametrize("kappa", [-2.0, 1.0])
def test_clamped_variance_gives_the_mean_and_its_gradient(kappa):
    fk, X = _clamped_model()
    val, best, grad, mean, var = fk.confidence_bound(X, kappa, want_grad=True, want_posterior=True)
    zero = var == 0
    assert 0 < zero.sum() < len(X)
    assert np.isfinite(val).all() and np.isfinite(grad).all()
    _, _, dmean, dvar, _ = fk.predict_with_gradient(X)
    assert val[zero].tobytes() == mean[zero].astype(np.float64).tobytes() and grad[zero].tobytes() == dmean[zero].tobytes()
    assert (val[~zero] != mean[~zero]).any() and best == R.argmin_first(val)
    _compare(np.float32, val, grad, mean, var, dmean, dvar, kappa)
    print(f"{int(zero.sum())} clamped variances among 64")
    fk.release()


@DTYPES
def test_nan_rows_and_no_rows(dtype):
    fk = _model(40, 3, 2.5, dtype)
    Xs = _candidates(9, 3, 31, dtype)
    clean = fk.confidence_bound(Xs, 1.0, want_grad=True)
    bad = Xs.copy()
    bad[clean[1], 1] = math.nan  # the row that won
    val, best, grad = fk.confidence_bound(bad, 1.0, want_grad=True)
    keep = np.arange(9) != clean[1]
    assert math.isnan(val[clean[1]]) and np.isnan(grad[clean[1]]).all()
    assert val[keep].tobytes() == clean[0][keep].tobytes() and grad[keep].tobytes() == clean[2][keep].tobytes()
    assert best == R.argmin_first(val) and best != clean[1] and best >= 0
    bad[:, 0] = math.nan
    val, best, grad = fk.confidence_bound(bad, 1.0, want_grad=True)
    assert np.isnan(val).all() and np.isnan(grad).all() and best == -1
    assert fk.confidence_bound(bad, 1.0)[1] == -1 and fk.confidence_bound(bad[:1], -2.0)[1] == -1
    val0, best0 = fk.confidence_bound(np.zeros((0, 3), dtype), 1.0)
    assert val0.shape == (0,) and best0 == -1
    fk.release()


@pytest.mark.parametrize("m", [1023, 1024, 1025, 2049])
def test_argmin_returns_the_first_of_two_equal_rows(m):
    """The lowest-bound row placed twice: bit-equal bounds, the early index has to come back.  (5, m - 3): far apart, in
    different threads' strides; (1023, 1024): the last thread's first entry against thread 0's second, which meet in the tree's
    last round; (0, 1024): both in thread 0's own scan."""
    dtype = np.float64
    fk = _model(40, 2, 2.5, dtype)
    pool = _candidates(m, 2, 41, dtype)
    val, best = fk.confidence_bound(pool, 1.0)
    assert best == R.argmin_first(val)
    lowest, other = pool[best].copy(), pool[(best + 1) % m].copy()
    pairs = [(5, m - 3)] if m > 8 else []
    if m > 1024:
        pairs += [(1023, 1024), (0, 1024)]
    for a, b in pairs:
        Xs = pool.copy()
        Xs[best] = other  # the pair holds the only copies of the minimum
        Xs[a] = Xs[b] = lowest
        val, got = fk.confidence_bound(Xs, 1.0)
        rest = np.ones(m, dtype=bool)
        rest[[a, b]] = False
        assert val[a] == val[b] and (val[rest] > val[a]).all()
        assert got == a == R.argmin_first(val), (a, b, got)
    single = fk.confidence_bound(pool[:1], 1.0)
    assert single[1] == 0
    fk.release()


def _same(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def test_bits_batch_position_gradient_repeat_and_threads():
    dtype = np.float64
    fk, fk2 = _model(130, 3, 2.5, dtype), _model(40, 3, 1.5, dtype)
    pool = _candidates(70, 3, 21, dtype)
    full = fk.confidence_bound(pool, 1.0, want_grad=True, want_posterior=True)
    full2 = fk2.confidence_bound(pool, -2.0, want_grad=True, want_posterior=True)
    assert _same(full, fk.confidence_bound(pool, 1.0, want_grad=True, want_posterior=True))  # the same call twice
    nograd = fk.confidence_bound(pool, 1.0)
    assert nograd[0].tobytes() == full[0].tobytes() and nograd[1] == full[1]
    for j in (0, 4, 69):  # a row alone, with and without a gradient
        for want_grad in (False, True):
            alone = fk.confidence_bound(pool[j:j + 1], 1.0, want_grad=want_grad)
            assert alone[0][0] == full[0][j] and alone[1] == 0
            if want_grad:
                assert alone[2].tobytes() == full[2][j].tobytes()
    moved = fk.confidence_bound(np.vstack([pool[5:9], pool[2:3], pool[:2]]), 1.0, want_grad=True)  # row 2 at position 4, m = 7
    assert moved[0][4] == full[0][2] and moved[2][4].tobytes() == full[2][2].tobytes()
    assert moved[0][:4].tobytes() == full[0][5:9].tobytes() and moved[2][:4].tobytes() == full[2][5:9].tobytes()
    rolled = fk.confidence_bound(np.roll(pool, 33, axis=0), 1.0, want_grad=True)  # another lane group, another workgroup
    assert np.roll(rolled[0], -33).tobytes() == full[0].tobytes() and np.roll(rolled[2], -33, axis=0).tobytes() == full[2].tobytes()
    got = [None, None]

    def run(i, model, kappa):
        for _ in range(5):
            got[i] = model.confidence_bound(pool, kappa, want_grad=True, want_posterior=True)

    ts = [threading.Thread(target=run, args=a, daemon=True) for a in ((0, fk, 1.0), (1, fk2, -2.0))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "two concurrent calls on two models did not return"
    assert _same(full, got[0]) and _same(full2, got[1])
    fk.release()
    fk2.release()


def test_wrong_arguments_on_a_real_model():
    lib = _lib.load()
    fk, fk32 = _model(40, 2, 2.5, np.float64), _model(40, 2, 2.5, np.float32)
    x, val, best = np.full((2, 2), 0.5), np.full(2, 7.0), C.c_int(5)

    def call(h=None, fn=lib.hbegp_confidence_bound_f64, xs=x, m=2, kappa=1.0, out=val):
        return fn(h or fk._h, _lib.aptr(xs), m, kappa, _lib.dptr(out), None, C.byref(best), None, None)

    for kw, what in ((dict(h=fk32._h), "model holds f32 data"),
                     (dict(fn=lib.hbegp_confidence_bound_f32, xs=x.astype(np.float32)), "model holds f64 data"),
                     (dict(m=-1), "m must be >= 0"), (dict(xs=None), "Xs/cb is NULL"), (dict(out=None), "Xs/cb is NULL"),
                     (dict(kappa=math.nan), "kappa is not finite"), (dict(kappa=-math.inf), "kappa is not finite")):
        assert call(**kw) == _lib.EINVAL and what in _lib.last_error(), (kw, _lib.last_error())
    assert val.tolist() == [7.0, 7.0] and best.value == 5  # a refused call writes nothing
    # a size that cannot fit is ENOMEM, counted before anything is taken (or read: Xs holds two rows)
    assert call(m=2 ** 31 - 1) == _lib.ENOMEM and "device memory" in _lib.last_error() and val.tolist() == [7.0, 7.0]
    assert call() == _lib.OK and best.value == 0 and val[0] == val[1] != 7.0  # two equal rows: the first
    lo, hi = np.zeros(2), np.ones(2)
    for kw, what in ((dict(kappa=math.inf), "kappa is not finite"), (dict(maxeval=0), "maxeval"),
                     (dict(starts=np.full((1, 2), 1.5)), "outside the box"), (dict(hi=-hi), "lo[0] > hi[0]")):
        args = dict(starts=x, lo=lo, hi=hi, kappa=1.0, maxeval=5)
        args.update(kw)
        with pytest.raises(_lib.HbegpError, match=what.replace("[", r"\[").replace("]", r"\]")):
            fk.minimize_confidence_bound(**args)
    xf, xo = x.astype(np.float32), np.full((2, 2), 7.0, np.float32)
    rc = lib.hbegp_minimize_confidence_bound_f32(fk._h, _lib.aptr(xf), 2, _lib.dptr(lo), _lib.dptr(hi), 1.0, 5, _lib.aptr(xo), _lib.dptr(val), None)
    assert rc == _lib.EINVAL and "model holds f64 data" in _lib.last_error() and (xo == 7).all()
    fk.release()
    fk32.release()


def _projected_gradient(x, g, lo, hi):
    pg = g.astype(np.float64).copy()
    pg[(x <= lo) & (g > 0)] = 0.0
    pg[(x >= hi) & (g < 0)] = 0.0
    return pg


@DTYPES
@pytest.mark.parametrize("kappa", [-2.0, 1.0])
@pytest.mark.parametrize("d", [1, 2, 8])
def test_minimiser(d, kappa, dtype):
    """S = 10 runs, the first three of them again as S = 3, and three of them alone (S = 1): a run's bits do not depend on the runs
    it shares its rounds with."""
    fk = _model(60, d, 2.5, dtype)
    lo, hi = np.zeros(d), np.ones(d)
    starts = np.random.default_rng(17 + d).uniform(0, 1, (10, d)).astype(dtype)
    s_val, _, s_grad = fk.confidence_bound(starts, kappa, want_grad=True)
    x, val, nevals = fk.minimize_confidence_bound(starts, lo, hi, kappa, maxeval=40)
    assert x.dtype == dtype and x.shape == (10, d) and (x >= 0).all() and (x <= 1).all()  # f32 results lie in the box too
    assert (val <= s_val).all(), (val, s_val)  # never worse than its start
    assert (nevals >= 1).all() and (nevals <= 40).all()
    again, _ = fk.confidence_bound(x, kappa)
    assert again.tobytes() == val.tobytes()
    x3, v3, n3 = fk.minimize_confidence_bound(starts[:3], lo, hi, kappa, maxeval=40)
    assert x3.tobytes() == x[:3].tobytes() and v3.tobytes() == val[:3].tobytes() and n3.tolist() == nevals[:3].tolist()
    for r in (0, 4, 9):  # a run alone
        x1, v1, n1 = fk.minimize_confidence_bound(starts[r:r + 1], lo, hi, kappa, maxeval=40)
        assert x1.tobytes() == x[r].tobytes() and v1[0] == val[r] and n1[0] == nevals[r]
    sloped = np.abs(_projected_gradient(starts.astype(np.float64), s_grad, lo, hi)).max(axis=1) > 1e-3
    assert sloped.any() and (val[sloped] < s_val[sloped]).any()
    x2, v2, n2 = fk.minimize_confidence_bound(starts, lo, hi, kappa, maxeval=2)  # a budget that binds
    assert (n2 <= 2).all() and (v2 <= s_val).all() and (x2 >= 0).all() and (x2 <= 1).all()
    print(f"{np.dtype(dtype).name} d={d} kappa={kappa}: starts {s_val}, minimised {val}, evaluations {nevals}")
    fk.release()


@DTYPES
def test_a_nan_start_fails_only_its_own_run(dtype):
    fk = _model(60, 2, 2.5, dtype)
    lo, hi = np.zeros(2), np.ones(2)
    starts = np.random.default_rng(19).uniform(0, 1, (3, 2)).astype(dtype)
    x, val, nevals = fk.minimize_confidence_bound(starts, lo, hi, 1.0, maxeval=30)
    bad = starts.copy()
    bad[1, 0] = math.nan
    xb, vb, nb = fk.minimize_confidence_bound(bad, lo, hi, 1.0, maxeval=30)
    assert xb[1].tobytes() == bad[1].tobytes() and vb[1] == math.inf and nb[1] == 1
    for r in (0, 2):
        assert xb[r].tobytes() == x[r].tobytes() and vb[r] == val[r] and nb[r] == nevals[r]
    fk.release()


@pytest.mark.parametrize("projection", ["linear", "logarithmic"])
def test_suggest_optimum_on_a_fitted_sphere(projection):
    g = np.linspace(0.0, 1.0, 7)
    X = np.array([[a, b] for a in g for b in g])
    nat = X * 4.0 - 2.0 + np.array([0.3, -0.45])  # the minimum lies between the grid's points
    y = (nat ** 2).sum(axis=1) + 0.5 + 0.05 * np.random.default_rng(5).standard_normal(len(X))
    model = E.EstimatorGPR.new(2).y_projection(projection).estimate(X, y, None, E.RNG.new_with_seed(77))
    kappa = 1.0
    start, suggestion_y = E.find_best_individual_by_confidence_bound(X, model, kappa)
    # the start individual's bound from the call the minimiser descends, projected as the suggestion's is
    start_cb, _ = model.fitted.confidence_bound(X[start:start + 1].astype(model.dtype), kappa)
    start_bound = model.y_norm.project_location_from_normalized(start_cb)[0]
    x, bound, mean, ei, idx = E.suggest_optimum(X, model, confidence_bound=kappa)
    assert idx == start and x.shape == (2,) and (x >= 0).all() and (x <= 1).all()
    assert bound <= start_bound, (bound, start_bound)
    # and against the batched predict's bound of the same individual, whose mean and variance may differ in the last bits
    batched = float(model.predict_confidence_bound_a(X, kappa)[start])
    assert bound <= batched + FC.tol_of(model.dtype) * max(1.0, abs(batched))
    m2, e2 = model.predict_mean_ei(x, suggestion_y)
    assert mean == m2 and ei == e2
    x3, bound3, _, _, idx3 = E.suggest_optimum(X, model, confidence_bound=kappa, n_starts=3)
    assert idx3 == start and bound3 <= bound
    print(f"{projection}: individual {start} bound {start_bound:.6g} -> {bound:.6g} at {x} (three starts: {bound3:.6g} at {x3}), "
          f"mean {mean:.6g}, EI {ei:.3g}")
    model.fitted.release()


@DTYPES
def test_pool_hygiene_of_the_two_new_calls(dtype):
    """tests/test_gpu_pool_hygiene.py's method: the bytes of a run on fresh blocks against runs under
    HBEGP_POOL_POISON = 1 and 2, the switch set in-process around the model's creation and the calls."""
    import test_gpu_pool_hygiene as H

    def evaluate(fk, case, m, dt):
        Xs = H._candidates(m, fk.d, 27 + m, dt)
        out = list(fk.confidence_bound(Xs, 1.0, want_grad=True, want_posterior=True)) + list(fk.confidence_bound(Xs[:9], -2.0, want_posterior=True))
        return out + list(fk.minimize_confidence_bound(Xs[:4], np.full(fk.d, -0.5), np.full(fk.d, 1.5), 1.0, maxeval=8))

    H._check(lambda: H._on_model(evaluate, (100, 4, 2.5), 70, dtype), 5, 1)  # at least cb, best and grad, then cb and best


def test_debug_cb_phases():
    lib = _lib.load()
    fk = _model(130, 2, 2.5, np.float64)
    Xs = _candidates(70, 2, 5, np.float64)
    ph, ph2 = np.full(4, -1.0), np.full(4, -2.0)
    assert lib.hbegp_debug_cb_phases(1, None) == _lib.OK
    timed = fk.confidence_bound(Xs, 1.0, want_grad=True)
    assert lib.hbegp_debug_cb_phases(0, _lib.dptr(ph)) == _lib.OK  # reading switches timing off
    print(f"phases: the predict {ph[0]:.3f} ms, the confidence-bound kernel and the arg-min {ph[1]:.3f} ms")
    assert np.isfinite(ph[:2]).all() and (ph[:2] > 0).all() and ph[2:].tolist() == [-1.0, -1.0]  # two phases, nothing past them
    untimed = fk.confidence_bound(Xs, 1.0, want_grad=True)
    assert lib.hbegp_debug_cb_phases(0, _lib.dptr(ph2)) == _lib.OK
    assert ph2[:2].tobytes() == ph[:2].tobytes() and ph2[2:].tolist() == [-2.0, -2.0]  # an untimed call stores nothing
    assert _same(timed, untimed)  # timing changes no bit
    fk.release()


def test_cpp_mirror_cb(tmp_path):
    exe = str(tmp_path / "test_cb")
    lib_dir = os.path.join(ROOT, "hbetune_rs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cb.cpp"),
                           "-L", lib_dir, "-lhbegp", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0 threw=1" in out.stdout
