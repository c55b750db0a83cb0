"""GPU: posterior sample paths (hbegp_paths_*) -- draws of the posterior that are functions, their gradients and minimisers.

The device against the NumPy restatement (tests/paths_ref.py) over the Matern orders, both element types, n = 200 and 4096,
shared and per-path points inside and slightly outside the unit box, including a nu = 1/2 draw with max |omega0| >= 1e4 (what the
fp64 phase is for); the fitted config-M model through parity_rules.Judge; the antithetic identity against hbegp_predict's mean;
eps = NULL against zeros; the three kinds of model; bits (repeat, threads, a point alone vs in a batch, shared vs per path); the
minimiser's contract and its quality against a grid; the estimator's opt-in acquire_by_path_thompson; handle lifetimes.

Bars: parity_rules.TOL64 = 1e-8 and TOL32 = 1e-4, relative to max(1, scale of the reference)."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import parity_rules as PRU
import paths_ref as PR
from hbetune_rs_amd import _lib, gpr, synth
from hbetune_rs_amd import estimator as E
from oracle import referee as R

pytestmark = pytest.mark.gpu

NUS = [0.5, 1.5, 2.5, math.inf]
D = 4
AMP = 1.3
F32_NOISE = 1.0  # f32: a noise of the amplitude's size keeps cond(K) <= n + 1 (tests/test_gpu_posterior_cov.py)


def _tol(dtype):
    return PRU.TOL64 if dtype == np.float64 else PRU.TOL32


def _data(n, dtype, seed=1, d=D):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    X, y = X.astype(dtype), y.astype(dtype)
    ratio = 1e-2 if dtype == np.float64 else F32_NOISE
    theta = np.log(np.concatenate([[ratio * AMP, AMP], np.linspace(0.3, 0.9, d)]))
    return X, y, theta


def _model(n, nu, dtype, seed=1, d=D):
    X, y, theta = _data(n, dtype, seed, d)
    return gpr.FittedKernel.extend(X, y, theta, nu=nu), X, y


def _draws(fk, F, S, seed, noise_draw=True, big_omega=False):
    rng = E.RNG(seed)
    om0, ph = gpr.draw_spectral(fk.nu, F, fk.d, rng)
    if big_omega:  # a Cauchy tail made certain: one frequency of 3e4, as F ~ 1e5 draws of nu = 1/2 would hold
        om0[F // 3] *= 3e4 / np.abs(om0[F // 3]).max()
        assert np.abs(om0).max() >= 1e4
    w = rng.standard_normal((S, F))
    eps = rng.standard_normal((S, fk.n)) if noise_draw else None
    c = lambda a: None if a is None else np.asarray(a, dtype=fk.dtype)  # noqa: E731
    return c(om0), c(ph), c(w), c(eps)


def _ref(fk, X, y, draws, solve=None):
    noise, amp, ell = fk.device_params()
    return PR.Paths(X, y, amp, ell, fk.nu, noise, *draws, solve=solve)


def _points(m, seed, dtype, d=D, S=None):
    shape = (m, d) if S is None else (S, m, d)
    return np.random.default_rng(seed).uniform(-0.1, 1.1, shape).astype(dtype)  # inside and slightly outside [0, 1]^d


def _devs(got, want):
    return PRU.dev(got, want)


def _compare(paths, ref, x, tol, what):
    f, df = paths.evaluate(x)
    rf, rdf = ref.evaluate(x)
    d_f, d_g = _devs(f, rf), _devs(df, rdf)
    print(f"{what}: f off by {d_f:.2e}, df by {d_g:.2e} (scales {np.abs(rf).max():.3g}, {np.abs(rdf).max():.3g}; bar {tol:g})")
    assert d_f <= tol, (what, d_f)
    assert d_g <= tol, (what, d_g)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [200, 4096])
@pytest.mark.parametrize("nu", NUS)
def test_device_matches_restatement(nu, n, dtype):
    fk, X, y = _model(n, nu, dtype, seed=n)
    S, F = (5, 1000) if n == 200 else (3, 700)  # F not a multiple of the chunk, S not of the path block
    draws = _draws(fk, F, S, seed=n + 3)
    paths = fk.sample_paths(*draws)
    ref = _ref(fk, X, y, draws)
    tol = _tol(dtype)
    _compare(paths, ref, _points(37, 5, dtype), tol, f"nu={nu} n={n} {np.dtype(dtype).name} shared")
    _compare(paths, ref, _points(6, 6, dtype, S=S), tol, f"nu={nu} n={n} {np.dtype(dtype).name} per path")
    f_only, none = paths.evaluate(_points(37, 5, dtype), want_grad=False)
    assert none is None and np.array_equal(f_only, paths.evaluate(_points(37, 5, dtype))[0])
    paths.release()
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cauchy_tail_needs_the_fp64_phase(dtype):
    """nu = 1/2 with max |omega0| >= 1e4: |omega . x + b| ~ 1e5, where an f32 phase is off by 1e-2 rad before the cosine."""
    fk, X, y = _model(200, 0.5, dtype, seed=2)
    draws = _draws(fk, 512, 4, seed=9, big_omega=True)
    paths = fk.sample_paths(*draws)
    ref = _ref(fk, X, y, draws)
    _compare(paths, ref, _points(64, 7, dtype), _tol(dtype), f"Cauchy tail {np.dtype(dtype).name} shared")
    _compare(paths, ref, _points(5, 8, dtype, S=4), _tol(dtype), f"Cauchy tail {np.dtype(dtype).name} per path")
    paths.release()
    fk.release()


def test_many_paths_many_features_and_a_wide_model():
    """S beyond one projection pass (64) and one GEMM tile (128), F at several chunks, d beyond one gradient pass (8)."""
    fk, X, y = _model(300, 2.5, np.float64, seed=4, d=11)
    draws = _draws(fk, 2100, 130, seed=5)
    paths = fk.sample_paths(*draws)
    ref = _ref(fk, X, y, draws)
    _compare(paths, ref, _points(9, 1, np.float64, d=11), PRU.TOL64, "S=130 F=2100 d=11 shared")
    _compare(paths, ref, _points(2, 2, np.float64, d=11, S=130), PRU.TOL64, "S=130 F=2100 d=11 per path")
    paths.release()
    fk.release()


def test_fitted_config_m_through_the_judge():
    """cond(K) ~ 7e11: where the plain bar fails, v's truth comes from the referee's refined solve of the same residual and the
    rule is |gpu - truth| <= max(1e-8 scale, 2 |lapack - truth|)."""
    w = synth.make_workload("M")
    X, y = w["X"], w["y"]
    fk = gpr.FittedKernel.new(X, y, w["theta0"], w["lo"], w["hi"], synth.restart_points("M", w["lo"], w["hi"], 2))
    draws = _draws(fk, 1024, 3, seed=21)
    paths = fk.sample_paths(*draws)
    lap = _ref(fk, X, y, draws)
    noise, amp, ell = fk.device_params()
    ref = R.Referee(X, y, noise, amp, ell, fk.nu)

    def solve(r):
        xh, xl = ref.solve(r)
        return xh + xl

    truth = {}

    def truth_paths():
        if "p" not in truth:
            truth["p"] = _ref(fk, X, y, draws, solve=solve)
        return truth["p"]

    xs = synth.candidates("M", 100, w["d"])
    f, df = paths.evaluate(xs)
    lf, ldf = lap.evaluate(xs)
    judge = PRU.Judge(PRU.TOL64)
    judge.check("f", f, lf, lambda: truth_paths().evaluate(xs)[0])
    judge.check("df", df, ldf, lambda: truth_paths().evaluate(xs)[1])
    print("config M:", judge.summary())
    assert judge.n_nodigits == 0 and judge.n_plain + judge.n_refereed == 2, judge.summary()  # both were judged, none waved through
    ref.close()
    paths.release()
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nu", NUS)
def test_antithetic_pair_is_the_predicted_mean(nu, dtype):
    fk, X, y = _model(500, nu, dtype, seed=3)
    om0, ph, w, eps = _draws(fk, 900, 4, seed=8)
    a = fk.sample_paths(om0, ph, w, eps)
    b = fk.sample_paths(om0, ph, -w, -eps)
    xs = _points(200, 4, dtype)
    mean, _, _ = fk.predict(xs, want_variance=False)
    mid = 0.5 * (a.evaluate(xs, False)[0].astype(np.float64) + b.evaluate(xs, False)[0].astype(np.float64))
    dev = np.abs(mid - mean.astype(np.float64)[None, :]).max() / max(1.0, np.abs(mean).max())
    print(f"nu={nu} {np.dtype(dtype).name}: antithetic pair off the predicted mean by {dev:.2e}")
    assert dev <= _tol(dtype)
    a.release(); b.release(); fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_no_noise_draw_is_a_zero_noise_draw(dtype):
    fk, X, y = _model(300, 2.5, dtype)
    om0, ph, w, _ = _draws(fk, 300, 3, seed=1, noise_draw=False)
    a = fk.sample_paths(om0, ph, w, None)
    b = fk.sample_paths(om0, ph, w, np.zeros((3, fk.n), dtype=dtype))
    xs = _points(50, 2, dtype)
    fa, ga = a.evaluate(xs)
    fb, gb = b.evaluate(xs)
    assert np.array_equal(fa, fb) and np.array_equal(ga, gb)
    a.release(); b.release(); fk.release()


# ------------------------------------------------------------------------------------------------------ the kinds of model
def _kind_fitted(dtype):
    w = synth.make_workload("C2", n=300)
    lo = w["lo"].copy()
    if dtype == np.float32:
        lo[0] = 1e-2 * w["amplitude"]
    X, y = w["X"].astype(dtype), w["y"].astype(dtype)
    th0 = np.clip(w["theta0"], np.log(lo), np.log(w["hi"]))
    return gpr.FittedKernel.new(X, y, th0, lo, w["hi"], None, maxeval=20), X, y


def _kind_small(dtype):
    w = synth.make_workload("C2", n=100)
    lo = w["lo"].copy()
    if dtype == np.float32:
        lo[0] = 1e-2 * w["amplitude"]
    X, y = w["X"].astype(dtype), w["y"].astype(dtype)
    th0 = np.clip(w["theta0"], np.log(lo), np.log(w["hi"]))
    return gpr.FittedKernel.new(X, y, th0, lo, w["hi"], None, maxeval=10), X, y


def _kind_incremental(dtype):
    fk0, X, y = _model(300, 2.5, dtype, seed=6)
    X2, y2, _ = _data(420, dtype, seed=6)
    assert np.array_equal(X2[:300], X)
    fk = fk0.extend_with(X2, y2)
    fk0.release()
    return fk, X2, y2


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", [_kind_fitted, _kind_small, _kind_incremental])
def test_every_kind_of_model(kind, dtype):
    """The kinds of model whose y, L^-1 and padding come from different code than extend()'s.  Both element types: the antithetic
    identity against hbegp_predict's mean at the plain bar (it needs no reference solve).  f64 also against the restatement through
    the Judge; an f32 fit's cond(K) is beyond what an f64-LAPACK comparison of v at 1e-4 can decide, so f32 stops at the identity."""
    fk, X, y = kind(dtype)
    om0, ph, w, eps = _draws(fk, 600, 3, seed=12)
    paths = fk.sample_paths(om0, ph, w, eps)
    mirror = fk.sample_paths(om0, ph, -w, -eps)
    xs = np.random.default_rng(3).uniform(X.min(axis=0) - 0.05, X.max(axis=0) + 0.05, (40, fk.d)).astype(dtype)
    f, df = paths.evaluate(xs)
    assert np.isfinite(f).all() and np.isfinite(df).all()
    mean, _, _ = fk.predict(xs, want_variance=False)
    mid = 0.5 * (f.astype(np.float64) + mirror.evaluate(xs, False)[0].astype(np.float64))
    dev = np.abs(mid - mean.astype(np.float64)[None, :]).max() / max(1.0, np.abs(mean).max())
    print(f"{kind.__name__} {np.dtype(dtype).name}: n = {fk.n}, antithetic pair off the predicted mean by {dev:.2e} (bar {_tol(dtype):g})")
    assert dev <= _tol(dtype)
    mirror.release()
    if dtype == np.float64:
        draws = (om0, ph, w, eps)
        lap = _ref(fk, X, y, draws)
        noise, amp, ell = fk.device_params()
        ref = R.Referee(X, y, noise, amp, ell, fk.nu)
        truth = {}

        def tp():
            if "p" not in truth:
                truth["p"] = _ref(fk, X, y, draws, solve=lambda r: sum(ref.solve(r)))
            return truth["p"]

        judge = PRU.Judge(PRU.TOL64)
        judge.check("f", f, lap.evaluate(xs)[0], lambda: tp().evaluate(xs)[0])
        judge.check("df", df, lap.evaluate(xs)[1], lambda: tp().evaluate(xs)[1])
        print(kind.__name__, judge.summary())
        assert judge.n_nodigits == 0 and judge.n_plain + judge.n_refereed == 2, judge.summary()
        ref.close()
    paths.release()
    fk.release()


def _einval(rc, what):
    assert rc == _lib.EINVAL, rc
    assert what in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_refusals_that_need_a_model_or_a_handle(dtype):
    """Every argument check of hbegp_paths_* that tests/test_paths_cpu.py cannot reach without a device.  (d > 66, the optimiser's
    state, is refused too but cannot be provoked: a model has at most 64 features.)"""
    lib = _lib.load()
    other_t = np.float32 if dtype == np.float64 else np.float64
    sfx, osfx = ("f64", "f32") if dtype == np.float64 else ("f32", "f64")
    holds, oholds = f"holds {sfx} data", f"holds {osfx} data"
    fk, X, y = _model(200, 2.5, dtype)
    S, F, Rn = 3, 64, 2
    om0, ph, w, eps = _draws(fk, F, S, seed=1)
    p, op = _lib.aptr, _lib.aptr
    h = C.c_void_p()
    create = getattr(lib, f"hbegp_paths_create_{sfx}")
    for args in ((None, p(ph), p(w)), (p(om0), None, p(w)), (p(om0), p(ph), None)):
        _einval(create(fk._h, args[0], args[1], args[2], p(eps), F, S, C.byref(h)), "is NULL")
    _einval(create(fk._h, p(om0), p(ph), p(w), p(eps), F, S, None), "is NULL")
    # the other element type on this model: the only guard against reading X and y with the wrong element size
    oc = lambda a: np.asarray(a, dtype=other_t)  # noqa: E731
    _einval(getattr(lib, f"hbegp_paths_create_{osfx}")(fk._h, op(oc(om0)), op(oc(ph)), op(oc(w)), None, F, S, C.byref(h)), "model " + holds)
    assert not h.value
    paths = fk.sample_paths(om0, ph, w, eps)
    lo, hi = np.zeros(D), np.ones(D)
    starts = np.full((S, Rn, D), 0.5, dtype=dtype)
    xb, fb = np.zeros((S, D), dtype=dtype), np.zeros(S)
    mini = getattr(lib, f"hbegp_paths_minimize_{sfx}")
    d_ = _lib.dptr
    ok = [p(starts), Rn, d_(lo), d_(hi), 5, p(xb), d_(fb), None]
    for i in (0, 2, 3, 5, 6):
        a = list(ok)
        a[i] = None
        _einval(mini(paths._h, *a), "is NULL")
    so, xo = oc(starts), oc(xb)
    _einval(getattr(lib, f"hbegp_paths_minimize_{osfx}")(paths._h, op(so), Rn, d_(lo), d_(hi), 5, op(xo), d_(fb), None), "paths handle " + holds)
    bad_lo = lo.copy()
    bad_lo[1] = 2.0
    _einval(mini(paths._h, p(starts), Rn, d_(bad_lo), d_(hi), 5, p(xb), d_(fb), None), "lo[1] > hi[1]")
    _einval(mini(paths._h, p(starts), 0, d_(lo), d_(hi), 5, p(xb), d_(fb), None), "R must be >= 1")
    _einval(mini(paths._h, p(starts), Rn, d_(lo), d_(hi), 0, p(xb), d_(fb), None), "maxeval must be >= 1")
    out = np.zeros((S, 1), dtype=dtype)
    ev = getattr(lib, f"hbegp_paths_eval_{sfx}")
    _einval(ev(paths._h, p(starts), 1, 0, None, None), "is NULL")
    _einval(ev(paths._h, None, 1, 0, p(out), None), "is NULL")
    _einval(ev(paths._h, p(starts), -1, 0, p(out), None), "m must be >= 0")
    _einval(ev(paths._h, p(starts), 1, 3, p(out), None), "per_path must be 0 or 1")
    _einval(getattr(lib, f"hbegp_paths_eval_{osfx}")(paths._h, op(so), 1, 0, op(oc(out)), None), "paths handle " + holds)
    assert mini(paths._h, *ok) == _lib.OK  # ... and the same arguments intact are accepted
    assert oholds != holds
    paths.release()
    fk.release()


# ---------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_same_bits_again_alone_in_a_batch_and_across_threads(dtype):
    fk, X, y = _model(700, 1.5, dtype)
    draws = _draws(fk, 800, 5, seed=4)
    paths = fk.sample_paths(*draws)
    xs = _points(33, 11, dtype)
    f0, g0 = paths.evaluate(xs)
    f1, g1 = paths.evaluate(xs)
    assert np.array_equal(f0, f1) and np.array_equal(g0, g1)
    # a point alone, and the same points handed over per path
    fa, ga = paths.evaluate(xs[7:8])
    assert np.array_equal(fa[:, 0], f0[:, 7]) and np.array_equal(ga[:, 0], g0[:, 7])
    fp, gp = paths.evaluate(np.ascontiguousarray(np.broadcast_to(xs, (5,) + xs.shape)))
    assert np.array_equal(fp, f0) and np.array_equal(gp, g0)
    # a second handle from the same draws
    again = fk.sample_paths(*draws)
    f2, g2 = again.evaluate(xs)
    assert np.array_equal(f2, f0) and np.array_equal(g2, g0)
    # four threads on one handle, then on four handles
    handles = [again] + [fk.sample_paths(*draws) for _ in range(3)]
    for hs in ([paths] * 4, handles):
        out = [None] * 4

        def run(i):
            out[i] = hs[i].evaluate(xs)

        ts = [threading.Thread(target=run, args=(i,)) for i in range(4)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        for f, g in out:
            assert np.array_equal(f, f0) and np.array_equal(g, g0)
    for h in handles:
        h.release()
    paths.release()
    fk.release()


def test_nan_stays_in_its_row():
    fk, X, y = _model(200, 2.5, np.float64)
    paths = fk.sample_paths(*_draws(fk, 256, 3, seed=1))
    xs = _points(9, 1, np.float64)
    f0, g0 = paths.evaluate(xs)
    xs[4, 2] = np.nan
    f, g = paths.evaluate(xs)
    keep = np.arange(9) != 4
    assert np.isnan(f[:, 4]).all() and np.isnan(g[:, 4]).all()
    assert np.array_equal(f[:, keep], f0[:, keep]) and np.array_equal(g[:, keep], g0[:, keep])
    paths.release()
    fk.release()


# --------------------------------------------------------------------------------------------------------------- the minimiser
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_minimiser_contract(dtype):
    fk, X, y = _model(300, 2.5, dtype)
    S, Rn = 6, 5
    paths = fk.sample_paths(*_draws(fk, 512, S, seed=2))
    lo, hi = np.full(D, 0.0), np.full(D, 1.0)
    starts = np.random.default_rng(5).uniform(0, 1, (S, Rn, D)).astype(dtype)
    x, fb, nev = paths.minimize(starts, lo, hi, maxeval=60)
    assert ((x >= 0) & (x <= 1)).all() and (nev >= Rn).all() and (nev <= Rn * 60).all()
    at = paths.evaluate(x[:, None, :], want_grad=False)[0][:, 0]
    assert np.array_equal(at.astype(np.float64), fb)  # bit for bit what evaluate gives there
    f_starts = paths.evaluate(starts, want_grad=False)[0].astype(np.float64)
    assert (fb[:, None] <= f_starts).all()
    assert (fb < f_starts.min(axis=1)).any()  # it moved
    # maxeval = 1: the best start (ties to the first)
    x1, fb1, nev1 = paths.minimize(starts, lo, hi, maxeval=1)
    best = f_starts.argmin(axis=1)
    assert np.array_equal(x1, starts[np.arange(S), best]) and np.array_equal(fb1, f_starts.min(axis=1)) and (nev1 == Rn).all()
    # the same starts for every path
    xs, fs, _ = paths.minimize(starts[0], lo, hi, maxeval=30)
    assert xs.shape == (S, D)
    # refusals that need a handle
    lib = _lib.load()
    bad = starts.copy()
    bad[2, 1, 0] = 1.5
    with pytest.raises(gpr.HbegpError, match="outside the box"):
        paths.minimize(bad, lo, hi)
    other = lib.hbegp_paths_eval_f32 if dtype == np.float64 else lib.hbegp_paths_eval_f64
    z = np.zeros(8, dtype=np.float32 if dtype == np.float64 else np.float64)
    assert other(paths._h, _lib.aptr(z), 1, 0, _lib.aptr(z), None) == _lib.EINVAL and "paths handle holds" in _lib.last_error()
    fn = getattr(lib, f"hbegp_paths_eval_{paths._sfx}")
    assert fn(paths._h, None, 1, 0, None, None) == _lib.EINVAL and "NULL" in _lib.last_error()
    assert fn(paths._h, None, 0, 0, None, None) == _lib.OK  # m = 0 is a no-op
    n, d, F, Sg, is32 = (C.c_int() for _ in range(5))
    assert lib.hbegp_paths_info(paths._h, C.byref(n), C.byref(d), C.byref(F), C.byref(Sg), C.byref(is32)) == _lib.OK
    assert (n.value, d.value, F.value, Sg.value, is32.value) == (300, D, 512, S, int(dtype == np.float32))
    paths.release()
    fk.release()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_minimiser_reaches_the_grid_minimum(dtype):
    """n = 200, d = 2, 16 paths, R = 8: f_best <= the path's minimum over a 200 x 200 grid plus the plain bar, for at least all
    but one path (a cap: the restatement driven by SciPy's L-BFGS-B from the same starts stays within it)."""
    fk, X, y = _model(200, 2.5, dtype, seed=5, d=2)
    S, Rn = 16, 8
    paths = fk.sample_paths(*_draws(fk, 1024, S, seed=6))
    g = np.linspace(0, 1, 200)
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2).astype(dtype)
    fgrid = paths.evaluate(grid, want_grad=False)[0].astype(np.float64).min(axis=1)
    # starts: per path the 8 lowest cell centres of a 10 x 10 lattice.  (Checked on the CPU before this choice was committed: the
    # restatement driven by SciPy's L-BFGS-B from these starts misses 1 path of 16 in f64 and none in f32; from 8 uniform random
    # starts per path it missed 1 - 3 over six seeds -- the f64 paths, at a noise of 1e-2 of the amplitude, have many basins.)
    c1 = (np.arange(10) + 0.5) / 10
    lat = np.stack(np.meshgrid(c1, c1, indexing="ij"), axis=-1).reshape(-1, 2).astype(dtype)
    flat = paths.evaluate(lat, want_grad=False)[0]
    starts = lat[np.argsort(flat, axis=1, kind="stable")[:, :Rn]]
    x, fb, nev = paths.minimize(starts, np.zeros(2), np.ones(2))
    bar = _tol(dtype) * np.maximum(1.0, np.abs(fgrid))
    miss = int((fb > fgrid + bar).sum())
    print(f"{np.dtype(dtype).name}: {miss} of {S} paths above their grid minimum; mean gain below the grid {np.mean(fgrid - fb):.3e}; evals {nev.sum()}")
    assert miss <= 1
    paths.release()
    fk.release()


# ------------------------------------------------------------------------------------------------- estimator and lifetimes
def test_acquire_by_path_thompson():
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, (150, 3))
    yv = ((X - 0.37) ** 2).sum(axis=1)
    model = E.EstimatorGPR.new(3).estimate(X, yv, None, E.RNG.new_with_seed(3))
    bounds = [(0.0, 1.0)] * 3
    a = E.acquire_by_path_thompson(model, 6, E.RNG(5), bounds, n_features=512, n_restarts=4)
    b = E.acquire_by_path_thompson(model, 6, E.RNG(5), bounds, n_features=512, n_restarts=4)
    assert a.shape == (6, 3) and np.array_equal(a, b)
    assert ((a >= 0) & (a <= 1)).all()
    assert len({tuple(r) for r in a.tolist()}) == 6  # k distinct points
    # a quadratic bowl with its minimum at 0.37: the paths' minimisers gather around it
    assert np.abs(np.median(a, axis=0) - 0.37).max() < 0.25
    p = model.sample_paths_a(2, 64, E.RNG(1), noise_draw=False)
    assert p.evaluate(X[:5])[0].shape == (2, 5)
    p.release()


def test_handles_outlive_their_model_and_do_not_leak():
    fk, X, y = _model(300, 2.5, np.float64)
    draws = _draws(fk, 256, 3, seed=1)
    paths = fk.sample_paths(*draws)
    xs = _points(10, 1, np.float64)
    f0, _ = paths.evaluate(xs)
    fk.release()  # the handle retains the model
    f1, _ = paths.evaluate(xs)
    assert np.array_equal(f0, f1)
    paths.release()
    paths.release()  # twice is a no-op
    import torch
    fk, X, y = _model(300, 2.5, np.float64)
    free = []
    for i in range(40):
        p = fk.sample_paths(*draws)
        p.evaluate(xs)
        p.release()
        if i in (9, 39):
            free.append(torch.cuda.mem_get_info()[0])
    assert free[0] - free[1] < 8 << 20, free  # the pool recycles the blocks: no growth per handle
    fk.release()
