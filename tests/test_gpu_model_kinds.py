"""GPU: every posterior query on every kind of model against the fp64 oracle and, where the oracle's digits end, the referee.

make_model (csrc/hbegp.cpp) fills a model's L^-1, diag(L), alpha, K^-1 and device parameter block four ways: from the slot of the
evaluation that just ran (extend), through a second factorisation at the captured theta (host-driven fits), from buffer b of the
ping-pong pair of a device-driven small fit (with that run's own parameters), and by an incremental extend from a prior model.
A factor of another evaluation leaves alpha, K^-1 and the lml right and moves only the variance, its gradient, Sigma, the draws
and the batch picks: so every model of the table below is queried through predict (both paths), predict_with_gradient,
predict_cov, sample_posterior, select_batch and maximize_ei, and judged at the parameters the kernels use (device_params()).

Bars (tests/parity_rules.py): f64 the plain 1e-8 against LAPACK, else |gpu - truth| <= max(1e-8 scale, 2 |lapack - truth|); f32
the plain 1e-4 against the f64 oracle on the same rounded inputs.  f32 joint queries (gradient, Sigma, draws, batch) only where
cond(K) <= n + 1 (noise >= amplitude), as tests/test_gpu_posterior_cov.py and tests/test_gpu_batch_select.py keep them."""
import math
import time

import numpy as np
import pytest

import batch_select_ref as BS
import parity_rules as PR
import posterior_cov_ref as PC
import predict_grad_ref as PG
from hbetune_rs_amd import gpr, synth
from oracle import gpr_oracle as O
from oracle import referee as R

pytestmark = pytest.mark.gpu

NUS = [0.5, 1.5, 2.5, math.inf]


# ---------------------------------------------------------------------------------------------------------------- the makers
def captured_buffer(trace):
    """The ping-pong buffer make_model copies L^-1 / diag(L) / alpha / K^-1 from after a device-driven small fit, replayed from the
    fit's trace.  Per run: the first evaluation writes buffer 0, every later one the buffer that does not hold the run's best
    (target = 1 - best), and a finite lml strictly above the run's best makes target the best (kernels.hip:2934, :2986); the model
    takes the best buffer of the slot whose run won (hbegp.cpp:1694, :1707).  Returns (b, winning run, its winning evaluation)."""
    i_win = int(np.argmax(trace["lml"]))  # ties: the lowest (run, eval), as the trace is in (run, eval) order
    run = int(trace["run"][i_win])
    best, best_lml = -1, -math.inf
    idx = np.flatnonzero(trace["run"] == run)
    for e, i in enumerate(idx):
        target = 0 if best < 0 else 1 - best
        lml = trace["lml"][i]
        if math.isfinite(lml) and (best < 0 or lml > best_lml):
            best, best_lml = target, lml
    return best, run, int(i_win - idx[0])


def _data(n, d, seed, dtype):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    return X.astype(dtype), y.astype(dtype)


def _extend(n, d, dtype, nu=2.5, seed=1):
    X, y = _data(n, d, seed, dtype)
    amp = 1.3
    ratio = 1e-2 if dtype == np.float64 else (2.0 if math.isinf(nu) else 1.0)  # f32: the noise of the f32 posterior tests
    ell = np.linspace(0.3, 0.9, d) * math.sqrt(max(d, 4) / 4)  # (the same correlation range in every d)
    fk = gpr.FittedKernel.extend(X, y, np.log(np.concatenate([[ratio * amp, amp], ell])), nu=nu)
    return fk, X, y


def _workload(cfg, n, dtype):
    w = synth.make_workload(cfg, n=n)
    lo = w["lo"].copy()
    if dtype == np.float32:
        lo[0] = 1e-2 * w["amplitude"]  # the f32 noise floor (tests/test_gpu_parity.py::test_f32_path_himmelblau)
    return w["X"].astype(dtype), w["y"].astype(dtype), w, lo


def _theta0(w, lo):
    return np.clip(w["theta0"], np.log(lo), np.log(w["hi"]))


def make_extend_lds(n, d, dtype, nu):
    def make(mp):
        assert n <= 128 and d <= 32  # the single launch in the LDS
        return _extend(n, d, dtype, nu, seed=n + d)
    return make


def make_extend_general(d):
    def make(mp):
        assert d > 32  # beyond SMALL_EVAL_MAXD: the general path at n <= 128
        return _extend(90, d, np.float64, seed=d)
    return make


def make_extend_big(n, dtype):
    def make(mp):
        assert n > 128
        print(f"extend at n = {n}: {'task queue' if (n + 127) // 128 >= 6 else 'launch path'}")
        return _extend(n, 5, dtype, seed=n)
    return make


def make_small_fit(b_want, dtype, host=False):
    """n = 100 and maxeval = 1 (b = 0), or n = 128 and the smallest maxeval whose replay gives b = 1; host: HBEGP_SMALL_FIT=0."""
    def make(mp):
        n = 100 if b_want == 0 else 128
        X, y, w, lo = _workload("C2", 200, dtype)
        if host:
            mp.setenv("HBEGP_SMALL_FIT", "0")
        # host: a fit whose last evaluation is not its best (the model's L^-1 must come from the factorisation at the captured
        # theta, not from the slot's last evaluation)
        for maxeval in ((1,) if b_want == 0 else range(25, 5, -1) if host else (2, 3, 4, 5, 6, 8, 10, 12, 16, 20)):
            fk = gpr.FittedKernel.new(X[:n], y[:n], _theta0(w, lo), lo, w["hi"], None, maxeval=maxeval, trace=True)
            b, run, ev = captured_buffer(fk.trace)
            if (host and ev != len(fk.trace["lml"]) - 1) or (not host and b == b_want):
                break
            fk.release()
        if host:
            mp.delenv("HBEGP_SMALL_FIT")
            assert ev != len(fk.trace["lml"]) - 1, "every maxeval in the list ends on the captured evaluation"
            print(f"host-driven fit at n = {n}, maxeval = {maxeval}: captured evaluation {ev} of {len(fk.trace['lml'])}")
        else:
            assert b == b_want, "no maxeval in the list captures buffer 1"
            print(f"device-driven small fit at n = {n}, maxeval = {maxeval}: captured buffer b = {b} (evaluation {ev})")
        fk.captured_b = None if host else b
        fk.rows = (X, y)  # every generated row (the incremental maker appends the rest)
        return fk, X[:n], y[:n]
    return make


def make_fit(n, dtype, maxeval=25):
    def make(mp):
        X, y, w, lo = _workload("C2", n, dtype)
        starts = np.clip(synth.restart_points("C2", lo, w["hi"], 2), np.log(lo), np.log(w["hi"]))
        fk = gpr.FittedKernel.new(X, y, _theta0(w, lo), lo, w["hi"], starts, maxeval=maxeval, trace=True)
        b, run, ev = captured_buffer(fk.trace)
        n_run = int((fk.trace["run"] == run).sum())
        print(f"fit at n = {n}: run {run} won at its evaluation {ev} of {n_run}")
        return fk, X, y
    return make


def make_sharded(mp):
    n = 300
    X, y, w, lo = _workload("C2", n, np.float64)
    pre = gpr.FittedKernel.new(X, y, _theta0(w, lo), lo, w["hi"], None, maxeval=40)
    corner = np.log(lo) + 0.25 * (np.log(w["hi"]) - np.log(lo))
    ctx = gpr.Context(device_ids=[0, 0])
    # runs r go to device entry r % 2: run 1 starts at an optimum, runs 0 and 2 at a corner with few evaluations
    starts = np.stack([pre.theta, corner])
    pre.release()
    fk = gpr.FittedKernel.new(X, y, corner, lo, w["hi"], starts, maxeval=12, ctx=ctx, trace=True)
    run = int(fk.trace["run"][int(np.argmax(fk.trace["lml"]))])
    assert run % 2 == 1, run
    print(f"sharded fit: the model comes from run {run}, device entry {run % 2}")
    fk.ctx = ctx
    return fk, X, y


def make_incremental(chain):
    def make(mp):
        X, y = _data(chain[-1], 5, 7, np.float64)
        amp = 1.3
        theta = np.log(np.concatenate([[1e-2 * amp, amp], np.linspace(0.3, 0.9, 5)]))
        fk = gpr.FittedKernel.extend(X[:chain[0]], y[:chain[0]], theta)
        for m in chain[1:]:
            nxt = fk.extend_with(X[:m], y[:m])
            assert nxt.incremental
            fk.release()
            fk = nxt
        print(f"incremental chain {' -> '.join(map(str, chain))}: incremental")
        return fk, X, y
    return make


def make_incremental_from_small_fit(mp):
    prior, _, _ = make_small_fit(1, np.float64)(mp)
    assert prior.captured_b == 1
    X, y = prior.rows
    fk = prior.extend_with(X, y)
    assert fk.incremental
    print(f"incremental from the small fit (prior buffer {prior.captured_b}) to n = {len(X)}: incremental")
    prior.release()
    return fk, X, y


def make_incremental_fallback(mp):
    X, y = _data(300, 5, 9, np.float64)
    amp = 1.3
    theta = np.log(np.concatenate([[1e-2 * amp, amp], np.linspace(0.3, 0.9, 5)]))
    prior = gpr.FittedKernel.extend(X[:256], y[:256], theta)
    X = X.copy()
    X[17, 2] += 1e-3
    fk = prior.extend_with(X, y)
    assert not fk.incremental
    prior.release()
    return fk, X, y


KINDS = {}
for i, (n, d) in enumerate([(n, d) for n in (1, 17, 100, 128) for d in (1, 7, 32)]):
    for dt in (np.float64, np.float32):
        KINDS[f"extend-lds-n{n}-d{d}-{np.dtype(dt).name}"] = make_extend_lds(n, d, dt, NUS[i % 4])
for d in (33, 64):
    KINDS[f"extend-general-n90-d{d}"] = make_extend_general(d)
for n in (300, 1100):
    for dt in (np.float64, np.float32):
        KINDS[f"extend-n{n}-{np.dtype(dt).name}"] = make_extend_big(n, dt)
for dt in (np.float64, np.float32):
    KINDS[f"small-fit-b0-{np.dtype(dt).name}"] = make_small_fit(0, dt)
    KINDS[f"small-fit-b1-{np.dtype(dt).name}"] = make_small_fit(1, dt)
KINDS["host-fit-n128"] = make_small_fit(None, np.float64, host=True)
KINDS["fit-launch-n300"] = make_fit(300, np.float64)
KINDS["fit-queue-n1100-float64"] = make_fit(1100, np.float64)
KINDS["fit-queue-n1100-float32"] = make_fit(1100, np.float32)
KINDS["fit-sharded-entry1"] = make_sharded
KINDS["incremental-256-300"] = make_incremental((256, 300))
KINDS["incremental-256-266-300"] = make_incremental((256, 266, 300))
KINDS["incremental-from-small-fit"] = make_incremental_from_small_fit
KINDS["incremental-fallback"] = make_incremental_fallback


# ---------------------------------------------------------------------------------------------------------------- the checks
class Ctx:
    """One model's references: the LAPACK oracle at the device's parameters (built at once), the referee (on first use)."""

    def __init__(self, fk, X, y):
        self.fk, self.dtype = fk, np.dtype(X.dtype)
        self.X, self.y = X.astype(np.float64), y.astype(np.float64)
        self.n, self.d = X.shape
        self.noise, self.amp, self.ell = fk.device_params()
        self.nu = fk.nu
        self.ref = O.extend(self.X, self.y, self.noise, self.amp, self.ell, self.nu)
        ev = np.linalg.eigvalsh(self.ref["kernel_matrix"])
        self.cond = float(ev[-1] / ev[0])
        self._rf = None
        self.tol = PR.TOL64 if self.dtype == np.float64 else PR.TOL32
        self.judge = PR.Judge(self.tol)

    @property
    def rf(self):
        if self._rf is None:
            self._rf = R.Referee(self.X, self.y, self.noise, self.amp, self.ell, self.nu)
        return self._rf

    def kinv_lapack(self):
        """K^-1 from LAPACK potri (the reference's own form of the variance, test_gpu_posterior_cov.py): the oracle's k_inv."""
        return self.ref["k_inv"]

    def check(self, what, got, lapack, truth_fn, scale=None):
        self.judge.check(what, got, lapack, truth_fn, scale=scale)

    def check_rows(self, what, got, lapack, truth_fn):
        """Gradients: PG.row_dev (relative to each row's largest entry); beyond the plain bar the rule of parity_rules.Judge row by
        row (relative to max(1, the row's largest entry of the truth))."""
        got = np.asarray(got, np.float64)
        d = PG.row_dev(got, lapack)
        j = self.judge
        if d <= self.tol:
            j.n_plain += 1
            j.worst_plain = max(j.worst_plain, d)
            return
        truth = truth_fn()
        for i in range(len(got)):
            s = max(1.0, float(np.abs(truth[i]).max()))
            e_gpu = float(np.abs(got[i] - truth[i]).max())
            e_lap = float(np.abs(lapack[i] - truth[i]).max())
            allowed = max(self.tol * s, 2.0 * e_lap)
            j.n_refereed += 1
            j.worst_ratio = max(j.worst_ratio, e_gpu / allowed)
            assert e_gpu <= allowed, f"{what} row {i}: |gpu - truth| = {e_gpu:.3e} > max({self.tol:g} * {s:.3g}, 2 * {e_lap:.3e})"

    def close(self):
        if self._rf is not None:
            self._rf.close()


def _pool(m, d, seed, dtype):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (m, d)).astype(dtype)


def _check_arrays(c):
    fk = c.fk
    alpha, kinv = fk.arrays()
    c.check("alpha", alpha, c.ref["alpha"], lambda: sum(c.rf.alpha()))
    if c.n <= 300:
        c.check("K^-1", kinv, c.ref["k_inv"], lambda: sum(c.rf.kinv()))
    else:
        cols = np.linspace(0, c.n - 1, 24).astype(int)
        c.check("K^-1 (columns)", kinv[:, cols], c.ref["k_inv"][:, cols], lambda: c.rf.kinv_columns(cols))
    c.check("lml", [fk.lml], [c.ref["lml"]], lambda: np.array([c.rf.lml()]))


def _lapack_predict(c, Xs):
    mean, var, _ = O.predict(Xs.astype(np.float64), c.X, c.ref["alpha"], c.ref["k_inv"], c.amp, c.ell, c.nu)
    return mean, var


def _check_predict(c, pool):
    for m in (1, 8, 9, 129):
        Xs = pool[:m]
        mean, var, _ = c.fk.predict(Xs)
        lm, lv = _lapack_predict(c, Xs)
        tr = []

        def truth(k, Xs=Xs, tr=tr):
            if not tr:
                tr.append(c.rf.predict(Xs.astype(np.float64)))
            return tr[0][k]

        c.check(f"predict mean m={m}", mean, lm, lambda: truth(0))
        c.check(f"predict var m={m}", var, lv, lambda: truth(1), scale=c.amp)


def _check_gradient(c, pool):
    for m in (1, 129):
        Xs = pool[:m]
        mean, var, dmean, dvar, _ = c.fk.predict_with_gradient(Xs)
        X64 = Xs.astype(np.float64)
        lm, lv = _lapack_predict(c, Xs)
        c.check(f"grad-path mean m={m}", mean, lm, lambda: c.rf.predict(X64)[0])
        c.check(f"grad-path var m={m}", var, lv, lambda: c.rf.predict(X64)[1], scale=c.amp)
        tr = []

        def truth(k, tr=tr):
            if not tr:
                tr.append(c.rf.predict_grad(X64))
            return tr[0][k]

        c.check_rows(f"dmean m={m}", dmean, PG.dmean_ref(X64, c.X, c.ref["alpha"], c.amp, c.ell, c.nu), lambda: truth(0))
        c.check_rows(f"dvar m={m}", dvar, PG.dvar_ref(X64, c.X, c.amp, c.ell, c.nu, c.noise, var=var), lambda: truth(1))


def _check_cov(c, pool):
    Xs = pool[:64]
    X64 = Xs.astype(np.float64)
    mean, cov = c.fk.predict_cov(Xs)
    lm, _ = _lapack_predict(c, Xs)
    c.check("Sigma mean", mean, lm, lambda: c.rf.predict(X64)[0])
    lapack = PC.sigma_ref_kinv(X64, c.X, c.kinv_lapack(), c.amp, c.ell, c.nu)
    c.check("Sigma", cov, lapack, lambda: c.rf.sigma(X64), scale=c.amp)


def _check_draws(c, pool):
    Xs = pool[:32]
    X64 = Xs.astype(np.float64)
    S0 = PC.sigma_ref(X64, c.X, c.amp, c.ell, c.nu, c.noise)
    ev = np.linalg.eigvalsh(S0)
    target = 1e6 if c.dtype == np.float64 else 1e2
    jitter = max(0.0, (ev[-1] - target * ev[0]) / (target - 1)) * 1.01
    cs = (ev[-1] + jitter) / (ev[0] + jitter)
    z = np.random.default_rng(5).standard_normal((16, 32)).astype(c.dtype)
    samples, argmin = c.fk.sample_posterior(Xs, z, jitter=jitter)
    lm, _ = _lapack_predict(c, Xs)
    lapack = PC.draws_ref(lm, PC.sigma_ref_kinv(X64, c.X, c.kinv_lapack(), c.amp, c.ell, c.nu, jitter=jitter), z)
    tr = []

    def truth():
        if not tr:
            tr.append(PC.draws_ref(c.rf.predict(X64)[0], c.rf.sigma(X64, jitter=jitter), z))
        return tr[0]

    c.check("draws", samples, lapack, truth)
    ref = tr[0] if tr else lapack
    bar = c.tol * max(1.0, float(np.abs(ref).max()))
    srt = np.sort(ref, axis=1)
    clear = (srt[:, 1] - srt[:, 0]) > 2 * bar
    assert np.array_equal(argmin[clear], np.argmin(ref, axis=1)[clear]), (argmin, np.argmin(ref, axis=1))
    return cs, jitter, int(clear.sum())


def _check_select(c, pool):
    Xs = pool[:64]
    X64 = Xs.astype(np.float64)
    pick_bar = 1e-12 if c.dtype == np.float64 else 1e-5
    fmin = float(np.min(c.y))
    for lie in (None, float(np.median(c.y))):
        idx, ei, mean, var = c.fk.select_batch(Xs, 4, fmin, lie=lie)
        assert len(set(idx.tolist())) == 4
        lm, _ = _lapack_predict(c, Xs)
        rl = BS.select(lm, PC.sigma_ref_kinv(X64, c.X, c.kinv_lapack(), c.amp, c.ell, c.nu), c.noise, fmin, 4, lie=lie, picks=idx)
        tr = []

        def truth(k):
            if not tr:
                tr.append(BS.select(c.rf.predict(X64)[0], c.rf.sigma(X64), c.noise, fmin, 4, lie=lie, picks=idx))
            return tr[0][k]

        c.check(f"select ei lie={lie}", ei, rl["ei"], lambda: truth("ei"))
        c.check(f"select mean lie={lie}", mean, rl["mean"], lambda: truth("mean"))
        c.check(f"select var lie={lie}", var, rl["var"], lambda: truth("var"), scale=c.amp)
        gap = float(np.max((rl["best"] - rl["ei"]) / np.maximum(1.0, rl["best"])))
        if gap > pick_bar:  # the pick against the truth's maxima, with the allowance of LAPACK's own error in them
            best_t, ei_t = truth("best"), truth("ei")
            gap_t = float(np.max((best_t - ei_t) / np.maximum(1.0, best_t)))
            e_lap = float(np.max(np.abs(rl["best"] - best_t) / np.maximum(1.0, best_t)))
            assert gap_t <= max(pick_bar, 2 * e_lap), (lie, gap_t, e_lap, idx)


def _check_maximizer(c):
    lo, hi = np.zeros(c.d), np.ones(c.d)
    starts = np.random.default_rng(3).uniform(0, 1, (4, c.d)).astype(c.dtype)
    fmin = float(np.min(c.y))
    x, ei, _ = c.fk.maximize_ei(starts, lo, hi, fmin, maxeval=40)
    assert ((x >= lo) & (x <= hi)).all()
    X64 = x.astype(np.float64)
    lm, lv = _lapack_predict(c, x)
    c.check("maximize_ei: EI at its x", ei, BS.expected_improvement(lm, lv, fmin),
            lambda: BS.expected_improvement(*c.rf.predict(X64)[:2], fmin))


@pytest.mark.parametrize("kind", list(KINDS))
def test_posterior_queries_on_every_kind_of_model(kind, monkeypatch):
    t0 = time.perf_counter()
    fk, X, y = KINDS[kind](monkeypatch)
    t1 = time.perf_counter()
    c = Ctx(fk, X, y)
    # the parameters the kernels use are exp(theta) of the model's theta up to the rounding of that theta (a device-driven fit's
    # are its own exp / clamp, theta is their log: an ulp of theta moves exp(theta) by |theta| eps relative)
    want = np.exp(fk.theta)
    got = np.concatenate([[c.noise, c.amp], c.ell])
    assert (np.abs(got - want) <= (np.abs(fk.theta) + 2) * np.finfo(float).eps * want).all(), (got, want)
    joint = c.dtype == np.float64 or c.noise >= c.amp  # f32: the range the f32 posterior tests keep (cond(K) <= n + 1)
    pool = _pool(129, c.d, 11 + c.n, c.dtype)
    _check_arrays(c)
    _check_predict(c, pool)
    extra = ""
    if joint:
        _check_gradient(c, pool)
        _check_cov(c, pool)
        cs, jitter, clear = _check_draws(c, pool)
        _check_select(c, pool)
        extra = f"; draws at jitter {jitter:.1e} (cond(Sigma) {cs:.1e}), argmin checked on {clear} of 16"
    else:
        extra = "; f32 joint queries gated (noise < amplitude)"
    _check_maximizer(c)
    print(f"{kind}: n = {c.n}, d = {c.d}, nu = {c.nu}, cond(K) = {c.cond:.2e}{extra}\n    {c.judge.summary()}\n"
          f"    wall: model {t1 - t0:.2f} s, checks {time.perf_counter() - t1:.2f} s")
    if c.dtype == np.float64:
        assert c.judge.n_nodigits == 0
    c.close()
    fk.release()


def test_device_params_refuses_a_null_out():
    fk, _, _ = _extend(17, 3, np.float64)
    from hbetune_rs_amd import _lib

    assert _lib.load().hbegp_model_debug_params(fk._h, None) == _lib.EINVAL
    assert "NULL out" in _lib.last_error()
    noise, amp, ell = fk.device_params()
    assert ell.shape == (3,) and noise > 0 and amp > 0
    fk.release()
