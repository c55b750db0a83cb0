"""GPU: the incremental extend (hbegp_extend_from_*, FittedKernel.extend_with) over block geometries, chains, fitted priors,
changed targets, its fall-back, its failures, recycled pool blocks and two threads.

Reference: oracle.gpr_oracle.extend / predict in fp64 from scratch on the same rounded inputs.  Bars: parity_rules.TOL64 /
TOL32 through parity_rules.dev -- lml and alpha relative to max(1, scale), K^-1 relative to its largest entry and reported per
region (kept x kept, new x kept, new x new: a failure names the region), the variance relative to the amplitude c.  The
full-path model of the same data is measured beside the incremental one; no bar is put on their ratio.  Models that come out of a
fit are judged by parity_rules.Judge at the fitted theta: the plain bar first, the referee only where that fails.

The cases and their data are tests/incremental_cases.py's; tests/test_incremental_cpu.py shows on the CPU that every term the
path adds or subtracts is at least 10 x the bar, so a dropped or misplaced term fails here."""
import math
import threading

import numpy as np
import pytest

import incremental_cases as IC
import parity_rules as PR
import test_gpu_model_kinds as MK
import test_gpu_pool_hygiene as PH
from hbetune_rs_amd import estimator as E
from hbetune_rs_amd import gpr, synth
from oracle import gpr_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = IC.DTYPES


def _dt(t):
    return np.dtype(t).name


_ORACLE = {}


def _oracle(key, X, y, theta, nu):
    """O.extend on the rounded inputs in fp64, computed once per key and left unchanged."""
    if key not in _ORACLE:
        noise, c, ell = IC.params(theta)
        _ORACLE[key] = O.extend(X.astype(np.float64), y.astype(np.float64), noise, c, ell, nu)
    return _ORACLE[key]


def _measure(fk, X, theta, nu, ref, w):
    """Every deviation of model fk from the oracle's `ref`, by name; w: the first row that is not kept."""
    noise, c, ell = IC.params(theta)
    alpha, kinv = fk.arrays()
    out = {"lml": PR.dev([fk.lml], [ref["lml"]]), "alpha": PR.dev(alpha, ref["alpha"])}
    s = float(np.abs(ref["k_inv"]).max())
    for name, (ri, ci) in IC.regions(w).items():
        if kinv[ri, ci].size:
            out["K^-1 " + name] = PR.dev(kinv[ri, ci].astype(np.float64) / s, ref["k_inv"][ri, ci] / s, 1.0)
    out["symmetric"] = 0.0 if np.array_equal(kinv, kinv.T) else math.inf
    pool = IC.query_points(X.shape[1], X.dtype)
    X64 = X.astype(np.float64)
    for m in IC.M_QUERY:
        mean, var, _ = fk.predict(pool[:m])
        rm, rv, _ = O.predict(pool[:m].astype(np.float64), X64, ref["alpha"], ref["k_inv"], c, ell, nu)
        out[f"mean m={m}"] = PR.dev(mean, rm)
        out[f"var m={m}"] = PR.dev(var, np.maximum(rv, 0.0), c)
    return out


def _judge(tag, fk, X, y, theta, nu, ref, n_kept, full=None):
    """Measures fk (and, for the record, the full-path model `full`), prints both side by side and asserts fk's bars."""
    dtype = X.dtype
    w = IC.geometry(n_kept, len(X))[0] * IC.NB
    got = _measure(fk, X, theta, nu, ref, w)
    beside = _measure(full, X, theta, nu, ref, w) if full is not None else {}
    for k, v in got.items():
        print(f"\nINC|{tag}|{_dt(dtype)}|{k}|{v:.2e}|" + (f"{beside[k]:.2e}" if k in beside else "-"))
    tol = IC.tol_of(dtype)
    bad = {k: v for k, v in got.items() if not v <= tol}
    assert not bad, f"{tag} {_dt(dtype)}: beyond {tol:g}: {bad}"
    return got


def _bytes(fk):
    alpha, kinv = fk.arrays()
    return [np.array([fk.lml]), alpha, kinv]


def _same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. the geometry grid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("case", IC.CASES, ids=IC.case_id)
def test_geometry_grid(case, dtype):
    n0, n, d, nu = case[:4]
    X, y, theta = IC.inputs(case, dtype)
    prior = gpr.FittedKernel.extend(X[:n0], y[:n0], theta, nu=nu)
    inc = prior.extend_with(X, y)
    assert inc.incremental
    full = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    ref = _oracle((IC.case_id(case), _dt(dtype)), X, y, theta, nu)
    _judge(IC.case_id(case), inc, X, y, theta, nu, ref, n0, full)
    again = prior.extend_with(X, y)
    assert again.incremental and _same_bytes(_bytes(inc), _bytes(again))
    for fk in (prior, inc, full, again):
        fk.release()


# ---- 2. chains --------------------------------------------------------------------------------------------------------------------
def _chain(tag, sizes, compare_at, d, nu, dtype):
    n_last = sizes[-1]
    X, y = IC.data(n_last, d, dtype)
    theta = IC.theta_of(d, nu, dtype)
    fk = gpr.FittedKernel.extend(X[:sizes[0]], y[:sizes[0]], theta, nu=nu)
    prev = sizes[0]
    for m in sizes[1:]:
        nxt = fk.extend_with(X[:m], y[:m])
        assert nxt.incremental, m
        fk.release()
        fk = nxt
        if m in compare_at:
            ref = _oracle((tag, m, _dt(dtype)), X[:m], y[:m], theta, nu)
            _judge(f"{tag} at n={m}", fk, X[:m], y[:m], theta, nu, ref, prev)
        prev = m
    fk.release()


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("nu", [0.5, 2.5])
def test_chain_of_single_rows_across_a_block_edge(nu, dtype):
    """250 -> 290, one row at a time: q0 goes 1 -> 2 at n = 256 and the fix comes (prior 250..255), goes (prior 256) and comes
    back (prior 257..).  The lml at every compared step is the only check of the diag(L) the chain hands on."""
    _chain(f"chain 250..290 nu={nu}", list(range(250, 291)), {251, 256, 257, 258, 270, 290}, 5, nu, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_chain_in_steps_of_17(dtype):
    sizes = list(range(128, 401, 17))
    assert sizes[-1] == 400
    _chain("chain 128..400 by 17", sizes, set(sizes[1:]), 5, 2.5, dtype)


# ---- 3. fitted priors -------------------------------------------------------------------------------------------------------------
MORE = (10, 140)


def _fit_inputs(n, dtype):
    """tests/test_gpu_model_kinds.py's fit workload with n + 140 rows; the noise floor is 1e-2 c in both element types."""
    w = synth.make_workload("C2", n=n + max(MORE))
    lo, hi = w["lo"].copy(), w["hi"].copy()
    # noise >= 1e-2 c at whatever the fit ends on: the floor is 1e-2 x the largest amplitude of the box (with the workload's own
    # upper bound a leave-one-out fit raised c far above its start value, cond(K) = 2.4e5: the f32 extension's alpha was 8.0e-4
    # from the oracle and the f64 one's 1.2e-11, rounding in proportion to cond(K) in both -- DESIGN.md section 25)
    hi[1] = w["amplitude"]
    lo[0] = 1e-2 * hi[1]
    return w["X"].astype(dtype), w["y"].astype(dtype), w, lo, hi


def _starts(w, lo, hi, count=2):
    return np.clip(synth.restart_points("C2", lo, hi, count), np.log(lo), np.log(hi))


def _prior_fit(n, dtype, by_loo=False, maxeval=25, tight=False):
    def make():
        X, y, w, lo, hi = _fit_inputs(n, dtype)
        if tight:
            hi[-1] = 0.05  # far below any length scale the data asks for: the fit ends on this bound
        theta0 = np.clip(w["theta0"], np.log(lo), np.log(hi))
        new = gpr.FittedKernel.new_by_loo if by_loo else gpr.FittedKernel.new
        fk = new(X[:n], y[:n], theta0, lo, hi, _starts(w, lo, hi), maxeval=maxeval)
        if tight:
            assert abs(math.exp(fk.theta[-1]) - hi[-1]) <= 1e-12 * hi[-1], (np.exp(fk.theta), hi)
        return fk, X, y
    return make


def _prior_small_fit(b_want, dtype):
    """The device-driven small fit at n = 128 whose model comes from ping-pong buffer b_want (test_gpu_model_kinds.make_small_fit)."""
    def make():
        n = 128
        X, y, w, lo, hi = _fit_inputs(n, dtype)
        theta0 = np.clip(w["theta0"], np.log(lo), np.log(hi))
        for maxeval in ((1,) if b_want == 0 else (2, 3, 4, 5, 6, 8, 10, 12, 16, 20)):
            fk = gpr.FittedKernel.new(X[:n], y[:n], theta0, lo, hi, None, maxeval=maxeval, trace=True)
            b, run, ev = MK.captured_buffer(fk.trace)
            if b == b_want:
                break
            fk.release()
        assert b == b_want, f"no maxeval in the list captures buffer {b_want}"
        return fk, X, y
    return make


def _prior_incremental(dtype):
    def make():
        X, y, w, lo, hi = _fit_inputs(300, dtype)
        theta = w["theta"]
        first = gpr.FittedKernel.extend(X[:200], y[:200], theta)
        fk = first.extend_with(X[:300], y[:300])
        assert fk.incremental
        first.release()
        return fk, X, y
    return make


PRIORS = {}
for _t in DTYPES:
    PRIORS[f"fit-launch-n300-{_dt(_t)}"] = (300, _prior_fit(300, _t))
    PRIORS[f"fit-queue-n700-{_dt(_t)}"] = (700, _prior_fit(700, _t, maxeval=8))
    PRIORS[f"fit-loo-n300-{_dt(_t)}"] = (300, _prior_fit(300, _t, by_loo=True))
    PRIORS[f"fit-on-a-bound-n300-{_dt(_t)}"] = (300, _prior_fit(300, _t, tight=True))
    PRIORS[f"incremental-200-300-{_dt(_t)}"] = (300, _prior_incremental(_t))
PRIORS["small-fit-b0-n128-float32"] = (128, _prior_small_fit(0, np.float32))
PRIORS["small-fit-b1-n128-float32"] = (128, _prior_small_fit(1, np.float32))


def _check_arrays(c, full=None):
    """alpha, the whole K^-1 and the lml of c.fk by parity_rules.Judge: the plain bar, then the referee; in f32 with the rule's
    third term, 8 sigma of what storing K in f32 costs (parity_rules.sigma32).  Returns the plain deviations of c.fk and, for
    the record, of the full-path model `full`."""
    sig = []

    def sigma(kind):
        if not sig:
            theta = np.log(np.concatenate([[c.noise, c.amp], c.ell]))
            sig.append(PR.sigma32(c.X, c.y, theta, [(0.0, math.inf)] * len(theta), c.nu))
        return sig[0][kind]

    def sfn(kind):
        return (lambda: sigma(kind)) if c.dtype == np.float32 else None

    alpha, kinv = c.fk.arrays()
    c.judge.check("alpha", alpha, c.ref["alpha"], lambda: sum(c.rf.alpha()), sigma_fn=sfn("alpha"))
    c.judge.check("K^-1", kinv, c.ref["k_inv"], lambda: sum(c.rf.kinv()), sigma_fn=sfn("kinv"))
    c.judge.check("lml", [c.fk.lml], [c.ref["lml"]], lambda: np.array([c.rf.lml()]), sigma_fn=sfn("lml"))
    assert np.array_equal(kinv, kinv.T)
    out = []
    for fk in (c.fk, full):
        if fk is not None:
            a, k = fk.arrays()
            out.append(f"alpha {PR.dev(a, c.ref['alpha']):.2e} K^-1 {PR.dev(k, c.ref['k_inv']):.2e} lml {PR.dev([fk.lml], [c.ref['lml']]):.2e}")
    return " | full path: ".join(out)


@pytest.mark.parametrize("kind", list(PRIORS))
def test_fitted_priors(kind):
    n0, make = PRIORS[kind]
    prior, X, y = make()
    for more in MORE:
        n = n0 + more
        ext = prior.extend_with(X[:n], y[:n])
        assert ext.incremental, (kind, more)
        assert np.array_equal(ext.theta, prior.theta)
        c = MK.Ctx(ext, X[:n], y[:n])  # the oracle at the parameters the extended model's kernels use
        want = np.exp(prior.theta)
        assert (np.abs(np.concatenate([[c.noise, c.amp], c.ell]) - want) <= (np.abs(prior.theta) + 2) * np.finfo(float).eps * want).all()
        full = gpr.FittedKernel.extend(X[:n], y[:n], prior.theta)
        devs = _check_arrays(c, full)
        full.release()
        MK._check_predict(c, MK._pool(129, c.d, 11 + n, c.dtype))
        print(f"\nINC|prior {kind} +{more}|{c.dtype.name}|cond(K) {c.cond:.2e}|{devs}|{c.judge.summary()}")
        if c.dtype == np.float64:
            assert c.judge.n_nodigits == 0
        c.close()
        ext.release()
    prior.release()


# ---- 4. targets -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_every_kept_target_may_change(dtype):
    case = IC.CASES[1]  # 255 -> 257: the fix runs
    n0, n, d, nu = case[:4]
    X, y, theta = IC.inputs(case, dtype)
    prior = gpr.FittedKernel.extend(X[:n0], y[:n0], theta, nu=nu)
    y2 = y.astype(np.float64)
    y2[:n0] = 0.5 * y2[:n0] - 1.0 + 0.1 * np.random.default_rng(3).standard_normal(n0)
    y2 = y2.astype(dtype)
    inc = prior.extend_with(X, y2)
    assert inc.incremental
    ref = _oracle(("targets", _dt(dtype)), X, y2, theta, nu)
    _judge("changed targets " + IC.case_id(case), inc, X, y2, theta, nu, ref, n0)
    prior.release()
    inc.release()


@pytest.mark.parametrize("projection", ["linear", "logarithmic"])
def test_estimator_extend_renormalises_every_target(projection):
    """EstimatorGPR.extend: the prior is a general-path fit and the y projection is taken over the enlarged set.  The box keeps
    noise >= 1e-2 c, the regime of every other fit of this module (the normalised targets have mean 1 under either projection):
    with the estimator's default box the fit of these noise-free targets ends at noise / c = 4.5e-9 under the linear projection,
    cond(K) = 3.9e10, where LAPACK's own alpha is 3.4e-5 from the truth and nothing is left for a 1e-8 bar to judge (the
    incremental and the full path give the same numbers there: DESIGN.md section 25)."""
    rng = np.random.default_rng(21)
    X = rng.random((230, 2))
    y = synth.goldstein_price(X * 4.0 - 2.0)
    est = E.EstimatorGPR.new(2).y_projection(projection).noise_bounds(2e-2, 1e5).amplitude_bounds((0.5, 2.0))
    model = est.estimate(X[:200], y[:200], None, E.RNG.new_with_seed(5))
    ext = est.extend(X, y, model)
    assert ext.fitted.incremental
    yn, norm = E.YNormalize.new_project_into_normalized(y, projection, None)
    assert ext.y_norm.expected == norm.expected and ext.y_norm.amplitude == norm.amplitude
    # every kept target moved, but the smallest: both projections send the minimum to a constant
    assert int((np.asarray(ext.fitted.y_train)[:200] == np.asarray(model.fitted.y_train)).sum()) <= 1
    c = MK.Ctx(ext.fitted, X, yn)
    devs = _check_arrays(c)
    MK._check_predict(c, MK._pool(129, 2, 11, np.float64))
    print(f"\nINC|estimator {projection}|float64|cond(K) {c.cond:.2e}|{devs}|{c.judge.summary()}")
    assert c.judge.n_nodigits == 0
    c.close()


# ---- 5. the fall-back -------------------------------------------------------------------------------------------------------------
def _alpha(fk):
    return fk.arrays(False)[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_fallback_when_the_prior_prefix_differs(dtype):
    n0, n, d, nu = 300, 330, 5, 2.5
    X, y = IC.data(n, d, dtype)
    theta = IC.theta_of(d, nu, dtype)
    tol = IC.tol_of(dtype)
    prior = gpr.FittedKernel.extend(X[:n0], y[:n0], theta, nu=nu)
    # the first entry, and the last entry of the prior's prefix (row 299: in the trailing block, compared but not kept)
    for r, k in ((0, 0), (n0 - 1, d - 1)):
        X2 = X.copy()
        X2[r, k] += 1e-3
        res = prior.extend_with(X2, y)
        assert not res.incremental, (r, k)
        full = gpr.FittedKernel.extend(X2, y, theta, nu=nu)
        assert np.array_equal(_alpha(res), _alpha(full)) and res.lml == full.lml, (r, k)
        res.release()
        full.release()
    # the first appended row is no part of the prefix
    X2 = X.copy()
    X2[n0, 2] += 1e-3
    res = prior.extend_with(X2, y)
    assert res.incremental
    _judge("changed first appended row", res, X2, y, theta, nu, _oracle(("appended", _dt(dtype)), X2, y, theta, nu), n0)
    res.release()
    # a NaN in the kept prefix: falls back, then fails as the full path fails
    X2 = X.copy()
    X2[17, 3] = np.nan
    codes = []
    for call in (lambda: prior.extend_with(X2, y), lambda: gpr.FittedKernel.extend(X2, y, theta, nu=nu)):
        with pytest.raises(gpr.HbegpError) as e:
            call()
        codes.append(e.value.code)
    assert codes == [gpr.NOT_PD, gpr.NOT_PD]
    # a prior on another feature count
    with pytest.raises((AssertionError, gpr.HbegpError)):
        prior.extend_with(X[:, :4], y)
    prior.release()
    # 128 -> 128: q0 = 0, nothing is kept
    n0, n, d, nu = IC.FALLBACK_128
    X, y = IC.data(n, d, dtype)
    theta = IC.theta_of(d, nu, dtype)
    prior = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    res = prior.extend_with(X, y)
    assert not res.incremental
    assert _same_bytes(_bytes(res), _bytes(prior))
    ref = _oracle(("128-128", _dt(dtype)), X, y, theta, nu)
    assert PR.dev(_alpha(res), ref["alpha"]) <= tol and PR.dev([res.lml], [ref["lml"]]) <= tol
    prior.release()
    res.release()


def test_fallback_sees_a_change_past_the_first_trip_of_the_comparison():
    """n = 4224, d = 64, f32: 270 336 prefix elements, more than the 1024 x 256 threads of the comparison's launch; only the
    second trip of its stride loop reads element 262 144 + 5."""
    n, d, nu = 4224, 64, 2.5
    X, y = IC.data(n, d, np.float32)
    theta = IC.theta_of(d, nu, np.float32)
    prior = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    same = prior.extend_with(X, y)
    assert same.incremental  # the unchanged rows are recognised
    same.release()
    X2 = X.copy()
    assert X2.size > 1024 * 256 + 5
    X2.reshape(-1)[1024 * 256 + 5] += np.float32(1e-3)
    res = prior.extend_with(X2, y)
    assert not res.incremental
    full = gpr.FittedKernel.extend(X2, y, theta, nu=nu)
    assert PR.dev(_alpha(res), _alpha(full)) <= PR.TOL32
    for fk in (prior, res, full):
        fk.release()


# ---- 6. failures ------------------------------------------------------------------------------------------------------------------
def _outcome(call):
    """What a call did: the status it raised with, or the NaN pattern of what it returned."""
    try:
        fk = call()
    except gpr.HbegpError as e:
        return ("raised", e.code, "Kernel matrix must be invertible." in str(e))
    alpha, kinv = fk.arrays()
    out = ("returned", math.isnan(fk.lml), np.isnan(alpha).tobytes(), np.isnan(kinv).tobytes())
    fk.release()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_failures_leave_the_prior_intact(dtype):
    n0, n, d, nu = 300, 330, 5, 2.5
    X, y = IC.data(n, d, dtype)
    theta = IC.theta_of(d, nu, dtype)
    prior = gpr.FittedKernel.extend(X[:n0], y[:n0], theta, nu=nu)
    pool = IC.query_points(d, dtype)
    before = [prior.predict(pool[:m]) for m in IC.M_QUERY]
    # a NaN feature in an appended row: the status of the full path, the reference's message
    X2 = X.copy()
    X2[n0 + 7, 1] = np.nan
    got = _outcome(lambda: prior.extend_with(X2, y))
    assert got == ("raised", gpr.NOT_PD, True), got
    assert got == _outcome(lambda: gpr.FittedKernel.extend(X2, y, theta, nu=nu))
    after = [prior.predict(pool[:m]) for m in IC.M_QUERY]
    for b, a in zip(before, after):
        assert b[0].tobytes() == a[0].tobytes() and b[1].tobytes() == a[1].tobytes() and b[2] == a[2]
    # the next call on the same prior is as good as the first
    inc = prior.extend_with(X, y)
    assert inc.incremental
    _judge("after a failed call", inc, X, y, theta, nu, _oracle(("after-failure", _dt(dtype)), X, y, theta, nu), n0)
    inc.release()
    # a NaN target: whatever the full path does with the same data
    for row in (5, n0 + 7):
        y2 = y.copy()
        y2[row] = np.nan
        want = _outcome(lambda: gpr.FittedKernel.extend(X, y2, theta, nu=nu))
        got = _outcome(lambda: prior.extend_with(X, y2))
        assert got == want, (row, got[:2], want[:2])
    inc = prior.extend_with(X, y)
    assert inc.incremental and PR.dev(_alpha(inc), _oracle(("after-failure", _dt(dtype)), X, y, theta, nu)["alpha"]) <= IC.tol_of(dtype)
    inc.release()
    prior.release()


# ---- 7. recycled pool blocks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("n0,n", [(300, 330), (128, 500), (256, 257)])
def test_recycled_blocks(n0, n, dtype):
    """The kept x new part of the slot's W2 and the upper part of its K^-1 buffer are never written by this path."""
    d, nu = 5, 2.5
    X, y = IC.data(n, d, dtype)
    theta = IC.theta_of(d, nu, dtype)

    def subject():
        prior = gpr.FittedKernel.extend(X[:n0], y[:n0], theta, nu=nu)
        fk = prior.extend_with(X, y)
        assert fk.incremental
        out = [fk.lml, *fk.arrays(), *fk.predict(IC.query_points(d, dtype)[:5]), *fk.predict(IC.query_points(d, dtype))]
        fk.release()
        prior.release()
        return out

    PH._check(subject, 15, 6 * PH._mat_bytes(n, dtype))


# ---- 8. two threads on one prior --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_two_threads_extend_one_prior(dtype):
    n0, d, nu = 300, 5, 2.5
    X, y = IC.data(n0, d, dtype)
    theta = IC.theta_of(d, nu, dtype)
    ctx = gpr.Context(device_ids=[0])
    prior = gpr.FittedKernel.extend(X, y, theta, nu=nu, ctx=ctx)
    jobs = []
    for k, more in enumerate((20, 150)):
        Xa, ya = IC.data(more, d, dtype, seed=1000 + k)
        jobs.append((np.vstack([X, Xa]), np.concatenate([y, ya])))

    def build(job):
        fk = prior.extend_with(job[0], job[1], ctx=ctx)
        out = [np.array([fk.incremental]), *_bytes(fk), *fk.predict(IC.query_points(d, dtype))[:2]]
        fk.release()
        return out

    solo = [build(j) for j in jobs]
    assert all(s[0][0] for s in solo)
    errors, bad = [], []

    def work(i):
        try:
            for rep in range(4):
                if not _same_bytes(build(jobs[i]), solo[i]):
                    bad.append((i, rep))
        except Exception as e:  # noqa: BLE001 -- the assertion below reports it
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    [t.start() for t in ts]
    [t.join(timeout=120) for t in ts]
    assert not any(t.is_alive() for t in ts), "a thread did not finish within 120 s"
    prior.release()
    ctx.close()
    assert not errors, errors
    assert not bad, bad
