"""GPU: max-value entropy search (hbegp_mes_* / hbegp_maximize_mes_*).

The device's mes and grad replayed through the NumPy / scipy restatement (tests/mes_ref.py) on the engine's own posteriors
(mean and var as the call returns them, dmean and dvar from predict_with_gradient); best, mean and var bit for bit; every branch
of the scalar function through y* placed at chosen gamma; clamped variances; NaN rows; bits across batch sizes, positions,
gradient on / off, repeats and threads; the refusals that need a model; the pool's poisons; the maximiser, with a start where
every gamma lies below -38; the phase clock; the estimator's layer through real sample paths; the C++ mirror.  The models are
tests/feature_count_cases.py's recipe through FittedKernel.extend at a fixed theta.

Bars (tests/mes_ref.py): 1e-8 (f64) / 1e-4 (f32) times max(1, |reference value|) for mes; for the gradient times
max(1, |d mes / d mu| |dmean| + |d mes / d sigma| |dsigma|) as well, row by row.  Measured deviations: DESIGN section 26."""
import ctypes as C
import math
import os
import subprocess
import threading

import numpy as np
import pytest

import feature_count_cases as FC
import mes_ref as R
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(n=40, d=2, nu=2.5, m=5, S=5)  # the base case every axis is varied against


def _model(n, d, nu, dtype):
    X, y, theta = FC.inputs(d, n, dtype)
    return gpr.FittedKernel.extend(X, y, theta, nu=nu)


def _candidates(m, d, seed, dtype):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (m, d)).astype(dtype)


def _ystar(fk, S, seed):
    """S plausible minimum values: around and below the lowest training target, a few above it (negative gamma)."""
    y = np.asarray(fk.y_train, dtype=np.float64)
    return y.min() + y.std() * np.random.default_rng(seed).uniform(-1.0, 0.5, S)


def _compare(dtype, val, grad, mean, var, dmean, dvar, ystar):
    """The device's (mes, grad) against the restatement's on the same posteriors: deviation / bar of both.  Asserts both."""
    rv, rg, scale = R.mes_grad_x(mean, var, dmean, dvar, ystar)
    assert np.isfinite(rv).all() and np.isfinite(val).all()
    dev = float((np.abs(val - rv) / R.value_bar(dtype, rv)).max())
    gdev = float((np.abs(grad.astype(np.float64) - rg).max(axis=1) / R.grad_bar(dtype, rv, scale)).max())
    assert dev <= 1.0 and gdev <= 1.0, (dev, gdev)
    return dev, gdev


def _replay(fk, Xs, ystar):
    dtype, m, d = fk.dtype, len(Xs), fk.d
    val, best, grad, mean, var = fk.mes(Xs, ystar, want_grad=True, want_posterior=True)
    assert val.dtype == np.float64 and val.shape == (m,) and grad.dtype == dtype and grad.shape == (m, d)
    pmean, pvar, dmean, dvar, _ = fk.predict_with_gradient(Xs)
    assert mean.tobytes() == pmean.tobytes() and var.tobytes() == pvar.tobytes()  # hbegp_predict_grad_*'s bits
    r = _compare(dtype, val, grad, mean, var, dmean, dvar, ystar)
    assert (val >= 0).all() and best == R.argmax_last(val)
    # without a gradient: the same mes bits, and the batched predict's posterior
    val2, best2, mean2, var2 = fk.mes(Xs, ystar, want_posterior=True)
    assert val2.tobytes() == val.tobytes() and best2 == best
    if m > 16:
        bmean, bvar, _ = fk.predict(Xs)
        assert mean2.tobytes() == bmean.tobytes() and var2.tobytes() == bvar.tobytes()
    return r


def _axis_cases():
    """Every value of each axis against BASE.  d = 64 is the most the library admits (engine.hpp: MAXD): a second trip of the
    kernel's feature stride, which would take d = 65, cannot be reached through the ABI."""
    cases = []
    for key, values in (("n", (40, 130)), ("d", (1, 2, 8, 64)), ("nu", (0.5, 1.5, 2.5, math.inf)), ("m", (1, 3, 4, 5, 9)),
                        ("S", (1, 63, 64, 65, 130, 1024))):
        for v in values:
            c = dict(BASE, **{key: v})
            if c not in cases:
                cases.append(c)
    return cases


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("case", _axis_cases(), ids=lambda c: "n%d-d%d-nu%s-m%d-S%d" % (c["n"], c["d"], c["nu"], c["m"], c["S"]))
def test_device_mes_replays_through_the_restatement(case, dtype):
    fk = _model(case["n"], case["d"], case["nu"], dtype)
    Xs = _candidates(case["m"], case["d"], 11, dtype)
    r = _replay(fk, Xs, _ystar(fk, case["S"], 3))
    print(f"{np.dtype(dtype).name} {case}: deviation / bar: values {r[0]:.1e}, grad {r[1]:.1e}")
    fk.release()


def test_a_larger_batch_returns_the_batched_predicts_posterior():
    fk = _model(130, 2, 2.5, np.float64)
    r = _replay(fk, _candidates(70, 2, 12, np.float64), _ystar(fk, 65, 4))  # m > 16: hbegp_predict_*'s batched path, 18 workgroups
    print(f"m = 70: deviation / bar: values {r[0]:.1e}, grad {r[1]:.1e}")
    fk.release()


GAMMAS = (-1e6, -30.0, -25.0, -24.9, -1.0, 0.0, 5.0, 40.0)


def test_branches_on_a_low_noise_model():
    """s2 = 1e-8: a candidate at a training row (sigma about 3e-3) and one far from the data (sigma about sqrt(c)), y* placed as
    mu - gamma sigma for each gamma on its own (S = 1) and for all eight together."""
    dtype = np.float64
    X, y, theta = FC.inputs(2, 40, dtype)
    theta = theta.copy()
    theta[0] = math.log(1e-8)
    fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
    for name, x in (("at a training row", X[7:8]), ("far from the data", np.array([[4.0, -3.0]]))):
        mean, var, dmean, dvar, _ = fk.predict_with_gradient(x)
        sd = math.sqrt(var[0])
        assert sd > 1e-4
        ys_all = mean[0] - np.array(GAMMAS) * sd
        for ys in [ys_all[k:k + 1] for k in range(len(GAMMAS))] + [ys_all]:
            val, best, grad, m2, v2 = fk.mes(x, ys, want_grad=True, want_posterior=True)
            assert m2.tobytes() == mean.tobytes() and v2.tobytes() == var.tobytes() and best == 0
            assert math.isfinite(val[0]) and val[0] >= 0.0 and np.isfinite(grad).all()
            r = _compare(dtype, val, grad, mean, var, dmean, dvar, ys)
            _, rg, _ = R.mes_grad_x(mean, var, dmean, dvar, ys)
            assert ((grad != 0) | (rg == 0)).all(), (ys, grad, rg)  # non-zero wherever the reference's is
            g = (mean[0] - ys) / sd
            print(f"{name}: sigma = {sd:.3g} gamma = {g if len(g) > 1 else g[0]:}: mes = {val[0]:.6g}, |grad| = {np.abs(grad).max():.3g}, "
                  f"deviation / bar: {r[0]:.1e}, {r[1]:.1e}")
    fk.release()


def test_clamped_variance_gives_exactly_zero():
    """The f32 amplitude-1e4 model of tests/test_gpu_lcei.py at its own training rows: about half of the variances clamp to 0."""
    g = np.stack(np.meshgrid(np.linspace(0, 1, 8), np.linspace(0, 1, 8)), axis=-1).reshape(-1, 2)
    dtype, theta = np.float32, np.log([1e-4, 1e4, 0.05, 0.05])
    X, y = g.astype(dtype), (np.sin(3 * g).sum(axis=1) * 100.0).astype(dtype)
    fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
    ys = np.array([40.0, 90.0, 150.0])  # inside the targets' range: gamma of either sign
    val, best, grad, mean, var = fk.mes(X, ys, want_grad=True, want_posterior=True)
    zero = var == 0
    assert 0 < zero.sum() < len(X)
    assert not np.isnan(val).any() and np.isfinite(grad).all()
    assert not val[zero].any() and not grad[zero].any()
    assert (val >= 0).all() and val[~zero].any() and best == R.argmax_last(val)
    _, _, dmean, dvar, _ = fk.predict_with_gradient(X)
    _compare(dtype, val, grad, mean, var, dmean, dvar, ys)
    print(f"{int(zero.sum())} clamped variances among 64")
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=lambda t: np.dtype(t).name)
def test_nan_row_and_no_rows(dtype):
    fk = _model(40, 3, 2.5, dtype)
    Xs, ys = _candidates(9, 3, 31, dtype), _ystar(fk, 7, 5)
    clean = fk.mes(Xs, ys, want_grad=True)
    bad = Xs.copy()
    bad[5, 1] = math.nan
    val, best, grad = fk.mes(bad, ys, want_grad=True)
    keep = np.arange(9) != 5
    assert math.isnan(val[5]) and np.isnan(grad[5]).all()
    assert val[keep].tobytes() == clean[0][keep].tobytes() and grad[keep].tobytes() == clean[2][keep].tobytes()
    assert best == R.argmax_last(val) and best != 5
    val0, best0 = fk.mes(np.zeros((0, 3), dtype), ys)
    assert val0.shape == (0,) and best0 == -1
    fk.release()


def _same(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def test_bits_batch_position_gradient_repeat_and_threads():
    dtype = np.float64
    fk = _model(130, 2, 2.5, dtype)
    pool, ys = _candidates(9, 2, 21, dtype), _ystar(fk, 130, 6)
    full = fk.mes(pool, ys, want_grad=True, want_posterior=True)
    assert _same(full, fk.mes(pool, ys, want_grad=True, want_posterior=True))  # the same call twice
    nograd = fk.mes(pool, ys)
    assert nograd[0].tobytes() == full[0].tobytes() and nograd[1] == full[1]
    for j in (0, 4, 8):  # a row alone, with and without a gradient
        for want_grad in (False, True):
            alone = fk.mes(pool[j:j + 1], ys, want_grad=want_grad)
            assert alone[0][0] == full[0][j] and alone[1] == 0
            if want_grad:
                assert alone[2].tobytes() == full[2][j].tobytes()
    moved = fk.mes(np.vstack([pool[5:9], pool[2:3], pool[:2]]), ys, want_grad=True)  # row 2 at position 4: another wave, another workgroup
    assert moved[0][4] == full[0][2] and moved[2][4].tobytes() == full[2][2].tobytes()
    assert moved[0][:4].tobytes() == full[0][5:9].tobytes()
    # a permuted ystar: the same quantity by other additions
    perm = fk.mes(pool, ys[np.random.default_rng(1).permutation(len(ys))], want_grad=True)
    assert (np.abs(perm[0] - full[0]) <= R.value_bar(dtype, full[0])).all()
    got = [None, None]

    def run(i):
        for _ in range(5):
            got[i] = fk.mes(pool, ys, want_grad=True, want_posterior=True)

    ts = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "two concurrent MES calls on one model did not return"
    assert _same(full, got[0]) and _same(full, got[1])
    fk.release()


def test_wrong_arguments_on_a_real_model():
    lib = _lib.load()
    fk, fk32 = _model(40, 2, 2.5, np.float64), _model(40, 2, 2.5, np.float32)
    x, val, best, ys = np.full((2, 2), 0.5), np.full(2, 7.0), C.c_int(5), np.zeros(1025)

    def call(h=None, fn=lib.hbegp_mes_f64, xs=x, m=2, y=ys, S=3, out=val):
        return fn(h or fk._h, _lib.aptr(xs), m, _lib.dptr(y), S, _lib.dptr(out), None, C.byref(best), None, None)

    for kw, what in ((dict(h=fk32._h), "model holds f32 data"), (dict(fn=lib.hbegp_mes_f32, xs=x.astype(np.float32)), "model holds f64 data"),
                     (dict(m=-1), "m must be >= 0"), (dict(xs=None), "Xs/mes is NULL"), (dict(out=None), "Xs/mes is NULL"),
                     (dict(S=0), "S must lie in"), (dict(S=1025), "S must lie in"), (dict(y=None), "ystar is NULL"),
                     (dict(y=np.array([0.0, math.nan, 0.0])), "ystar[1] is not finite"), (dict(y=np.array([0.0, 0.0, -math.inf])), "ystar[2]")):
        assert call(**kw) == _lib.EINVAL and what in _lib.last_error(), (kw, _lib.last_error())
    assert val.tolist() == [7.0, 7.0] and best.value == 5  # a refused call writes nothing
    assert call(S=1024) == _lib.OK and best.value in (0, 1) and (val != 7.0).all()
    lo, hi = np.zeros(2), np.ones(2)
    for kw, what in ((dict(ystar=np.zeros(0)), "S must lie in"), (dict(ystar=[math.nan]), "not finite"), (dict(maxeval=0), "maxeval"),
                     (dict(starts=np.full((1, 2), 1.5)), "outside the box"), (dict(hi=-hi), "lo[0] > hi[0]")):
        args = dict(starts=x, lo=lo, hi=hi, ystar=ys[:3], maxeval=5)
        args.update(kw)
        with pytest.raises(_lib.HbegpError, match=what.replace("[", r"\[").replace("]", r"\]")):
            fk.maximize_mes(**args)
    fk.release()
    fk32.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=lambda t: np.dtype(t).name)
def test_pool_hygiene_of_the_two_new_calls(dtype):
    """tests/test_gpu_pool_hygiene.py's method: the bytes of a run on fresh blocks against runs under HBEGP_POOL_POISON = 1 and 2,
    the switch set in-process around the model's creation and the calls."""
    import test_gpu_pool_hygiene as H

    def evaluate(fk, case, m, dt):
        Xs, ys = H._candidates(m, fk.d, 26 + m, dt), _ystar(fk, 130, 8)
        out = list(fk.mes(Xs, ys, want_grad=True, want_posterior=True)) + list(fk.mes(Xs[:9], ys[:5], want_posterior=True))
        return out + list(fk.maximize_mes(Xs[:4], np.full(fk.d, -0.5), np.full(fk.d, 1.5), ys[:16], maxeval=8))

    H._check(lambda: H._on_model(evaluate, (100, 4, 2.5), 70, dtype), 8, 1)  # at least the two calls' four borrowed blocks each


def _maximiser_case(dtype):
    fk = _model(60, 2, 2.5, dtype)
    starts = np.random.default_rng(17).uniform(0, 1, (6, 2)).astype(dtype)
    return fk, starts, _ystar(fk, 16, 9), np.zeros(2), np.ones(2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=lambda t: np.dtype(t).name)
def test_maximiser(dtype):
    fk, starts, ys, lo, hi = _maximiser_case(dtype)
    s_val, _ = fk.mes(starts, ys)
    x, val, nevals = fk.maximize_mes(starts, lo, hi, ys, maxeval=40)
    assert x.dtype == dtype and x.shape == (6, 2) and (x >= 0).all() and (x <= 1).all()  # f32 results lie in the box too
    assert (val >= s_val).all(), (val, s_val)
    assert (nevals >= 1).all() and (nevals <= 40).all()
    again, _ = fk.mes(x, ys)
    assert again.tobytes() == val.tobytes()
    for r in (0, 3, 5):  # a run alone
        x1, v1, n1 = fk.maximize_mes(starts[r:r + 1], lo, hi, ys, maxeval=40)
        assert x1.tobytes() == x[r].tobytes() and v1[0] == val[r] and n1[0] == nevals[r]
    print(f"{np.dtype(dtype).name}: starts {s_val}, maximised {val}, evaluations {nevals}")
    fk.release()


def test_maximiser_moves_where_every_gamma_lies_below_minus_38():
    """y* from 50 sigma above the start's mean upwards: phi(gamma) underflows for every sample, a naive form has no slope there
    (tests/test_mes_cpu.py shows the reference's gradient is an ordinary number)."""
    dtype = np.float64
    fk, starts, _, lo, hi = _maximiser_case(dtype)
    start = starts[2:3]
    mean, var, _, _, _ = fk.predict_with_gradient(start)
    sd = math.sqrt(var[0])
    ys = mean[0] + sd * np.linspace(50.0, 80.0, 16)
    s_val, _, s_grad = fk.mes(start, ys, want_grad=True)
    assert ((mean[0] - ys) / sd < -38.0).all() and math.isfinite(s_val[0]) and s_grad.any() and np.isfinite(s_grad).all()
    x, val, nevals = fk.maximize_mes(start, lo, hi, ys, maxeval=40)
    print(f"start mes = {s_val[0]:.6g} |grad| = {np.abs(s_grad).max():.3g} -> mes = {val[0]:.6g} at x = {x[0]} after {nevals[0]} evaluations")
    assert nevals[0] > 1 and val[0] > s_val[0] and nevals[0] <= 40
    assert fk.mes(x, ys)[0].tobytes() == val.tobytes()
    fk.release()


def test_debug_mes_phases():
    lib = _lib.load()
    fk = _model(130, 2, 2.5, np.float64)
    Xs, ys = _candidates(70, 2, 5, np.float64), _ystar(fk, 64, 2)
    ph, ph2 = np.full(2, -1.0), np.full(2, -2.0)
    assert lib.hbegp_debug_mes_phases(1, None) == _lib.OK
    timed = fk.mes(Xs, ys, want_grad=True)
    assert lib.hbegp_debug_mes_phases(0, _lib.dptr(ph)) == _lib.OK  # reading switches timing off
    print(f"phases: the predict {ph[0]:.3f} ms, the MES kernel and the arg-max {ph[1]:.3f} ms")
    assert np.isfinite(ph).all() and (ph > 0).all()
    untimed = fk.mes(Xs, ys, want_grad=True)
    assert lib.hbegp_debug_mes_phases(0, _lib.dptr(ph2)) == _lib.OK
    assert ph2.tobytes() == ph.tobytes()  # an untimed call stores nothing
    assert _same(timed, untimed)  # timing changes no bit
    fk.release()


def test_estimator_layer_through_real_sample_paths():
    dtype, S, R_, F = np.float64, 8, 4, 256
    fk = _model(60, 2, 2.5, dtype)
    model = E.SurrogateModelGPR(fk, None, None, None, E.YNormalize(1.0, 0.0, "linear"), dtype)
    bounds = [(0.0, 1.0)] * 2
    starts = np.random.default_rng(23).uniform(0, 1, (S, R_, 2))
    ys = model.sample_min_values(S, E.RNG.new_with_seed(11), bounds, n_features=F, n_restarts=R_, maxeval=30, starts=starts)
    assert ys.dtype == np.float64 and ys.shape == (S,) and np.isfinite(ys).all()
    paths = model.sample_paths_a(S, F, E.RNG.new_with_seed(11))  # the same draws: the starts were given, so the paths come first
    try:
        f, _ = paths.evaluate(starts, want_grad=False)
    finally:
        paths.release()
    assert (ys <= f.min(axis=1)).all(), (ys, f.min(axis=1))
    drawn = model.sample_min_values(S, E.RNG.new_with_seed(12), bounds, n_features=F, n_restarts=R_, maxeval=30)
    assert drawn.shape == (S,) and np.isfinite(drawn).all()
    val, best = model.mes_a(starts[0], ys)
    assert val.shape == (R_,) and (val >= 0).all() and best == R.argmax_last(val)
    x, v = E.acquire_by_max_value_entropy(model, 3, E.RNG.new_with_seed(13), bounds, n_samples=S, n_starts=6, n_features=F, n_restarts=R_,
                                          maxeval=30)
    assert x.shape == (3, 2) and len(np.unique(x, axis=0)) == 3 and (x >= 0).all() and (x <= 1).all()
    assert (np.diff(v) <= 0).all() and (v >= 0).all()
    cand = np.random.default_rng(29).uniform(0, 1, (40, 2))
    idx, cv = E.acquire_by_max_value_entropy(model, 3, E.RNG.new_with_seed(13), bounds, n_samples=S, candidates=cand, grid=cand)
    assert len(set(idx.tolist())) == 3 and (np.diff(cv) <= 0).all()
    print(f"y* = {ys}; maximiser picks {x.tolist()} mes {v}; candidate picks {idx.tolist()} mes {cv}")
    fk.release()


def test_cpp_mirror_mes(tmp_path):
    exe = str(tmp_path / "test_mes")
    lib_dir = os.path.join(ROOT, "hbetune_rs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_mes.cpp"),
                           "-L", lib_dir, "-lhbegp", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0 threw=1" in out.stdout
