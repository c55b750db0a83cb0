"""GPU: input warping -- hbegp_problem_eval_xgrad and hbegp_problem_eval_warped on every evaluation path
against the NumPy restatement tests/warp_ref.py, which tests/test_warp_cpu.py checks against central differences and whose inputs
it guards (every group of eight feature columns of G and every warp gradient entry far above the bars).

Bars, none of them new: parity_rules.TOL64 = 1e-8 and TOL32 = 1e-4, relative to max(1, largest reference entry) of the quantity."""
import ctypes as C
import math

import numpy as np
import pytest

import feature_count_cases as FC
import parity_rules as PRU
import warp_cases as WC
import warp_ref as WR
from hbetune_rs_amd import _lib, gpr

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_groups(what, got, ref, tol):
    """Per group of eight feature columns (one register pass of xgrad_kernel), relative to max(1, max |G|): a failure names the
    chunk."""
    scale = max(1.0, float(np.abs(ref).max()))
    worst = 0.0
    for sl in FC.groups(ref.shape[1], FC.GROUP_LOO):
        v = float(np.abs(got[:, sl] - ref[:, sl]).max()) / scale
        assert v <= tol, f"{what}: columns {sl.start}:{sl.stop} of G off by {v:.2e} of its scale (bar {tol:g})"
        worst = max(worst, v)
    assert worst == PRU.dev(got, ref)
    return worst


@pytest.mark.parametrize("case", WC.CASES, ids=[c.id for c in WC.CASES])
def test_x_gradient_and_warped_evaluation(case, monkeypatch):
    if case.kind == "queue":
        monkeypatch.setenv("HBEGP_DAG", "1")  # read when the problem is created
    X, y, theta = WC.inputs(case)
    rv = WC.row_variance(case)
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    tol, d, p = case.tol, case.d, case.d + 2
    prob = gpr.Problem(X, y, nu=case.nu, row_variance=rv)

    # ---- eval_xgrad: the plain evaluation's bits, the slot's state, G
    plain = prob.lml_with_gradient(theta)
    state = prob.results()
    lml, grad, gx = prob.lml_with_x_gradient(theta)
    assert lml == plain[0] and _bits_equal(grad, plain[1])
    for a, b in zip(prob.results(), state):
        assert _bits_equal(a, b)
    again = prob.lml_with_x_gradient(theta)
    assert again[0] == lml and _bits_equal(again[1], grad) and _bits_equal(again[2], gx)
    ref = WR.evaluate(X64, y64, *WR.params_of(theta), case.nu, rv)
    assert PRU.dev(lml, ref["lml"]) <= tol and PRU.dev(grad, ref["grad"]) <= tol
    d_g = _check_groups(f"{case.id} G", gx, ref["G"], tol)
    assert gx.dtype == np.float64 and gx.shape == (case.n, d)
    lml_only = prob.lml_with_x_gradient(theta, want_grad=False)  # grad = NULL: the evaluation without its gradient pass
    assert lml_only[1] is None and PRU.dev(lml_only[0], ref["lml"]) <= tol
    _check_groups(f"{case.id} G without the theta gradient", lml_only[2], ref["G"], tol)
    if case.kind == "dup":
        assert np.isfinite(gx).all() and np.abs(ref["G"][[3, 100]]).max() > 0

    # ---- eval_warped at a, b in [0.4, 2.5]
    ab = WC.warp_ab(case)
    before = prob.lml_with_gradient(theta)
    assert before[0] == plain[0] and _bits_equal(before[1], plain[1])
    wl, wg = prob.warped_lml_with_gradient(theta, ab)
    assert _bits_equal(prob.debug_rows(), X)  # the caller's rows are back
    after = prob.lml_with_gradient(theta)
    assert after[0] == plain[0] and _bits_equal(after[1], plain[1])
    rl, rg, _ = WR.warped_objective(X64, y64, theta, ab, case.nu, rv=rv)
    d_l, d_wg = PRU.dev(wl, rl), PRU.dev(wg, rg)
    assert wg.shape == (p + 2 * d,) and d_l <= tol, (case.id, d_l)
    gscale = max(1.0, float(np.abs(rg).max()))
    for name, sl in (("theta", slice(0, p)), ("ln a", slice(p, p + d)), ("ln b", slice(p + d, p + 2 * d))):
        v = float(np.abs(wg[sl] - rg[sl]).max()) / gscale
        assert v <= tol, f"{case.id}: the {name} entries of the warped gradient off by {v:.2e} of its scale (bar {tol:g})"
    wl2, wg2 = prob.warped_lml_with_gradient(theta, gpr.Warp(ab))
    assert wl2 == wl and _bits_equal(wg2, wg)
    only = prob.warped_lml_with_gradient(theta, ab, want_grad=False)
    assert only[1] is None and PRU.dev(only[0], rl) <= tol
    # the rows the device evaluated are the host warp's, rounded once
    monkeypatch.setenv("HBEGP_WARP_DEBUG_KEEP", "1")
    kept = prob.warped_lml_with_gradient(theta, ab)
    U = prob.debug_rows()
    monkeypatch.delenv("HBEGP_WARP_DEBUG_KEEP")
    assert kept[0] == wl and _bits_equal(kept[1], wg)
    assert _bits_equal(U, gpr.Warp(ab).apply(X64).astype(case.dtype))
    assert not _bits_equal(U, X)
    assert prob.warped_lml_with_gradient(theta, ab)[0] == wl and _bits_equal(prob.debug_rows(), X)
    final = prob.lml_with_gradient(theta)
    assert final[0] == plain[0] and _bits_equal(final[1], plain[1])
    # the identity warp: the plain evaluation up to the rounding of 1 - (1 - x)
    il, ig = prob.warped_lml_with_gradient(theta, np.ones(2 * d))
    assert PRU.dev(il, plain[0]) <= tol and PRU.dev(ig[:p], plain[1]) <= tol
    prob.close()
    print(f"WARP {case.id}: G {d_g:.2e}, warped lml {d_l:.2e}, warped gradient {d_wg:.2e} (bar {tol:g})")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_warped_evaluation_needs_one_slot_and_unit_features(dtype):
    case = WC.Case(64, 9, 2.5, dtype)
    X, y, theta = WC.inputs(case)
    prob = gpr.Problem(X, y, nu=case.nu, n_slots=2)
    with pytest.raises(_lib.HbegpError) as e:
        prob.warped_lml_with_gradient(theta, np.ones(2 * case.d))
    assert e.value.code == _lib.EINVAL and "n_slots == 1" in str(e.value)
    assert prob.lml_with_x_gradient(theta, slot=1) is not None  # the x gradient works on every slot
    prob.close()
    prob = gpr.Problem((X * 1.5).astype(dtype), y, nu=case.nu)
    with pytest.raises(_lib.HbegpError) as e:
        prob.warped_lml_with_gradient(theta, np.ones(2 * case.d))
    assert e.value.code == _lib.EINVAL and "[0, 1]" in str(e.value)
    prob.close()
    prob = gpr.Problem(X, y, nu=case.nu)
    lib = _lib.load()
    bad = np.ones(2 * case.d)
    bad[3] = 0.0
    lml = C.c_double(7.0)
    assert lib.hbegp_problem_eval_warped(prob._h, 0, 0, _lib.dptr(theta), None, None, _lib.dptr(bad), C.byref(lml), None) == _lib.EINVAL
    assert lml.value == 7.0
    prob.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_not_positive_definite(dtype):
    """144 copies of one row and vanishing noise (the input of tests/test_gpu_big128.py's E cases at n = 144): -inf and zero
    gradients from both calls, and the next evaluation is finite."""
    n, d = 144, 3
    rng = np.random.default_rng(5)
    X = np.tile(rng.random((1, d)), (n, 1)).astype(dtype)
    y = rng.random(n).astype(dtype)
    prob = gpr.Problem(X, y)
    lib = _lib.load()
    bad = np.array([math.log(1e-300), 0.0, 0.0, 0.0, 0.0])
    good = np.array([math.log(1e-2), 0.0, 0.0, 0.0, 0.0])
    p = d + 2
    lml = C.c_double(0.0)
    grad, gx = np.full(p, 7.0), np.full((n, d), 7.0)
    rc = lib.hbegp_problem_eval_xgrad(prob._h, 0, 0, _lib.dptr(bad), None, None, C.byref(lml), _lib.dptr(grad), _lib.dptr(gx))
    assert rc == _lib.NOT_PD and lml.value == -math.inf and (grad == 0).all() and (gx == 0).all()
    out = prob.lml_with_x_gradient(good)
    assert out is not None and np.isfinite(out[0]) and np.isfinite(out[1]).all() and np.isfinite(out[2]).all()
    wgrad = np.full(p + 2 * d, 7.0)
    ab = np.full(2 * d, 1.5)
    lml = C.c_double(0.0)
    rc = lib.hbegp_problem_eval_warped(prob._h, 0, 0, _lib.dptr(bad), None, None, _lib.dptr(ab), C.byref(lml), _lib.dptr(wgrad))
    assert rc == _lib.NOT_PD and lml.value == -math.inf and (wgrad == 0).all()
    assert _bits_equal(prob.debug_rows(), X)  # the rows went back although the evaluation failed
    out = prob.warped_lml_with_gradient(good, ab)
    assert out is not None and np.isfinite(out[0]) and np.isfinite(out[1]).all()
    assert prob.lml_with_gradient(good) is not None
    prob.close()


# ---- the warped fit --------------------------------------------------------------------------------------------------------------
_REFERENCE_FITS = {}


def _reference(n):
    """scipy's L-BFGS-B on the restated objectives (tests/test_warp_cpu.py checks that its gain exceeds 1 nat), once per size."""
    if n not in _REFERENCE_FITS:
        X, y = WC.fit_data(n)
        _REFERENCE_FITS[n] = WR.reference_fits(X, y, WC.FIT_THETA0, WC.FIT_LO, WC.FIT_HI, WC.FIT_NU)
    return _REFERENCE_FITS[n]


def _warped_fit(n, dtype, trace=False):
    X, y = WC.fit_data(n, dtype)
    lo, hi = WC.fit_box(dtype)
    wk = gpr.FittedKernel.new_warped(X, y, WC.FIT_THETA0, lo, hi, nu=WC.FIT_NU, trace=trace)
    return X, y, wk


@pytest.fixture(scope="module")
def fit96():
    X, y, wk = _warped_fit(96, np.float64, trace=True)
    yield X, y, wk
    wk.release()


def _check_fit(n, X, y, wk, tol):
    d, p = 2, 4
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    ab, theta = wk.warp.ab, wk.inner.theta_best
    lo, hi = WC.fit_box(X.dtype)
    assert (ab >= 0.2).all() and (ab <= 5.0).all() and (np.exp(theta) >= lo * (1 - 1e-12)).all() and (np.exp(theta) <= hi * (1 + 1e-12)).all()
    # (a) the returned lml is the objective at the returned point
    rl, _, _ = WR.warped_objective(X64, y64, theta, ab, WC.FIT_NU, lo, hi)
    d_a = PRU.dev(wk.lml_best, rl)
    assert d_a <= tol, (n, d_a)
    # (b) never worse than the plain fit it starts from
    assert wk.lml_best >= wk.plain_lml - 1e-9 * max(1.0, abs(wk.plain_lml)), (wk.lml_best, wk.plain_lml)
    # (d) the model is `extend` on the warped rows at theta_best, bit for bit
    U = wk.warp.apply(X64).astype(X.dtype)
    assert _bits_equal(U, wk.inner.x_train)
    fresh = gpr.FittedKernel.extend(U, y, theta, nu=WC.FIT_NU)
    assert fresh.lml == wk.inner.lml == wk.lml and _bits_equal(fresh.theta, wk.inner.theta)
    for a, b in zip(fresh.arrays(), wk.inner.arrays()):
        assert _bits_equal(a, b)
    # (e) the model carries its warp; a plain model carries none
    assert _bits_equal(wk.inner.warp_parameters, ab) and fresh.warp_parameters is None
    assert _lib.load().hbegp_model_warp(fresh._h, None) == 0 and _lib.load().hbegp_model_warp(wk.inner._h, None) == 1
    fresh.release()
    return d_a


@pytest.mark.parametrize("n", WC.FIT_SIZES)
def test_warped_fit_f64(n, fit96):
    X, y, wk = fit96 if n == 96 else _warped_fit(n, np.float64)
    d_a = _check_fit(n, X, y, wk, PRU.TOL64)
    # (c) at least half of what scipy gains on the restated objective from the plain optimum
    ref = _reference(n)
    gain = wk.lml_best - wk.plain_lml
    print(f"WARP fit n={n} f64: lml plain {wk.plain_lml:.4f} -> warped {wk.lml_best:.4f} (gain {gain:.4f}; reference {ref['lml_plain']:.4f} -> "
          f"{ref['lml_warped']:.4f}, gain {ref['gain']:.4f}); a, b = {wk.warp.ab}; lml vs the restatement {d_a:.2e}; "
          f"{wk.inner.n_evals} evaluations, {wk.inner.n_not_pd} not PD")
    assert ref["gain"] > 1.0 and gain >= 0.5 * ref["gain"], (gain, ref["gain"])
    if n != 96:
        wk.release()


def test_warped_fit_trace_replays_against_the_restatement(fit96):
    """(f) every evaluation of the traced fit against the restatement at the plain bar; evaluations at cond(K) > 1e8, where the
    restatement's own LAPACK arithmetic runs out of digits, are skipped, counted, and may be at most 5 % of the fit."""
    X, y, wk = fit96
    tr = wk.trace
    k, p = len(tr["lml"]), 4
    assert k == wk.inner.n_evals and k > 5 and tr["theta"].shape == (k, p + 4) and (tr["run"] == 0).all()
    skipped, worst = 0, np.zeros(2)
    for v, lml, grad in zip(tr["theta"], tr["lml"], tr["grad"]):
        ab = np.clip(np.exp(v[p:]), 0.2, 5.0)
        rl, rg, ev = WR.warped_objective(X, y, v[:p], ab, WC.FIT_NU, WC.FIT_LO, WC.FIT_HI)
        if np.linalg.cond(ev["K"]) > 1e8:
            skipped += 1
            continue
        dl, dg = PRU.dev(lml, rl), PRU.dev(grad, rg)
        worst = np.maximum(worst, [dl, dg])
        assert dl <= PRU.TOL64 and dg <= PRU.TOL64, (v, dl, dg, np.linalg.cond(ev["K"]))
    print(f"WARP fit trace: {k} evaluations, {skipped} skipped at cond(K) > 1e8 ({100.0 * skipped / k:.1f} %); worst lml {worst[0]:.2e}, "
          f"gradient {worst[1]:.2e} (bar {PRU.TOL64:g})")
    assert skipped <= 0.05 * k, (skipped, k)
    assert max(tr["lml"]) == wk.lml_best  # the capture is the trace's best


def test_warped_fit_f32():
    """(a) at TOL32 and (b), in the f32 box of warp_cases.fit_box (the suite's f32 noise floor).  In the f64 box the fit ends at
    cond(K) = 4.5e5 and the device's lml is 2.4e-4 |lml| from the restatement: beyond what f32 holds, not a property of the fit."""
    X, y, wk = _warped_fit(96, np.float32)
    d_a = _check_fit(96, X, y, wk, PRU.TOL32)
    print(f"WARP fit n=96 f32: lml plain {wk.plain_lml:.4f} -> warped {wk.lml_best:.4f}; a, b = {wk.warp.ab}; lml vs the restatement {d_a:.2e}")
    assert wk.lml_best - wk.plain_lml > 1.0
    wk.release()


def test_warped_fit_refuses_bad_input():
    X, y = WC.fit_data(96)
    with pytest.raises(_lib.HbegpError) as e:
        gpr.FittedKernel.new_warped(X * 1.2, y, WC.FIT_THETA0, WC.FIT_LO, WC.FIT_HI, nu=WC.FIT_NU)
    assert e.value.code == _lib.EINVAL and "[0, 1]" in str(e.value)
    plain = gpr.FittedKernel.extend(X, y, WC.FIT_THETA0, nu=WC.FIT_NU)
    with pytest.raises(_lib.HbegpError) as e:
        gpr.FittedKernel.new_warped(X, y, WC.FIT_THETA0, WC.FIT_LO, WC.FIT_HI, nu=WC.FIT_NU, warp_bounds=(0.0, 5.0), plain=plain)
    assert e.value.code == _lib.EINVAL
    plain.release()


# ---- the Python wrapper ------------------------------------------------------------------------------------------------------------
def test_warped_kernel_predicts_through_the_warp(fit96):
    X, y, wk = fit96
    rng = np.random.default_rng(8)
    x = rng.uniform(0.02, 0.98, (37, 2))
    u = wk.warp.apply(x)
    for got, ref in zip(wk.predict(x), wk.inner.predict(u)):
        assert _bits_equal(got, ref)
    for got, ref in zip(wk.predict_cov(x), wk.inner.predict_cov(u)):
        assert _bits_equal(got, ref)
    cb = wk.confidence_bound(x, -2.0, want_grad=True)
    assert _bits_equal(cb[0], wk.inner.confidence_bound(u, -2.0)[0])
    # gradients with respect to x: central differences of predict / confidence_bound in x
    mean, var, dmean, dvar, _ = wk.predict_with_gradient(x)
    h = 1e-6
    for k in range(2):
        e = np.zeros(2)
        e[k] = h
        mp, vp, _ = wk.predict(x + e)
        mm, vm, _ = wk.predict(x - e)
        cp, cm = wk.confidence_bound(x + e, -2.0)[0], wk.confidence_bound(x - e, -2.0)[0]
        for name, got, fd in (("dmean", dmean[:, k], (mp - mm) / (2 * h)), ("dvar", dvar[:, k], (vp - vm) / (2 * h)),
                              ("dcb", cb[2][:, k], (cp - cm) / (2 * h))):
            dev = float(np.abs(got - fd).max()) / max(1.0, float(np.abs(fd).max()))
            assert dev <= 1e-5, (name, k, dev)
    with pytest.raises(NotImplementedError) as e:
        wk.knowledge_gradient(x)
    assert ".inner" in str(e.value) and ".warp" in str(e.value)
    z = rng.standard_normal((3, len(x)))
    assert _bits_equal(wk.sample_posterior(x, z, jitter=1e-6)[0], wk.inner.sample_posterior(u, z, jitter=1e-6)[0])
    fmin = float(y.min())
    for got, ref in zip(wk.select_batch(x, 3, fmin), wk.inner.select_batch(u, 3, fmin)):
        assert _bits_equal(got, ref)


def test_warped_kernel_maximisers_work_in_u_space(fit96):
    X, y, wk = fit96
    rng = np.random.default_rng(9)
    lo, hi = np.array([0.05, 0.1]), np.array([0.9, 0.95])
    starts = rng.uniform(lo, hi, (6, 2))
    fmin = float(y.min())
    ulo, uhi = wk.warp.apply(lo[None, :])[0], wk.warp.apply(hi[None, :])[0]
    x, ei, nev = wk.maximize_ei(starts, lo, hi, fmin, maxeval=40)
    u, uei, unev = wk.inner.maximize_ei(wk.warp.apply(starts), ulo, uhi, fmin, maxeval=40)
    assert (x >= lo).all() and (x <= hi).all() and _bits_equal(ei, uei) and _bits_equal(nev, unev)
    assert np.abs(wk.warp.apply(x) - u).max() <= 1e-12 and (ei > 0).any()
    # the value at the returned x-space point is the maximiser's, up to the round trip of the point
    m, v, _ = wk.predict(x)
    from hbetune_rs_amd.estimator import expected_improvement
    again = np.array([expected_improvement(float(a), float(math.sqrt(b)), fmin) for a, b in zip(m, v)])
    assert np.abs(again - ei).max() <= 1e-8 * max(1.0, float(np.abs(ei).max()))
    xl, lei, _ = wk.maximize_log_ei(starts, lo, hi, fmin, maxeval=40)
    xc, cb, _ = wk.minimize_confidence_bound(starts, lo, hi, -2.0, maxeval=40)
    assert (xl >= lo).all() and (xl <= hi).all() and (xc >= lo).all() and (xc <= hi).all()
    assert _bits_equal(cb, wk.inner.minimize_confidence_bound(wk.warp.apply(starts), ulo, uhi, -2.0, maxeval=40)[1])
    assert np.isfinite(lei).all()


@pytest.mark.parametrize("n", WC.FIT_SIZES)
def test_warped_kernel_extends_with_the_fixed_warp(n, fit96):
    """One more row through the fixed warp: n = 96 takes the full path (the prior is shorter than a 128-block), n = 200 the
    incremental one; both against a fresh `extend` on all the warped rows at the bars of tests/test_gpu_incremental.py."""
    X, y, wk = fit96 if n == 96 else _warped_fit(n, np.float64)
    rng = np.random.default_rng(10)
    X2 = np.vstack([X, rng.uniform(0, 1, (1, 2))])
    y2 = np.concatenate([y, [0.3]])
    ext = wk.extend_with(X2, y2)
    assert isinstance(ext, gpr.WarpedKernel) and ext.warp is wk.warp and ext.inner.incremental == (n >= 128)
    U2 = wk.warp.apply(X2)
    assert _bits_equal(ext.inner.x_train, U2) and _bits_equal(U2[:n], wk.inner.x_train)
    fresh = gpr.FittedKernel.extend(U2, y2, wk.inner.theta, nu=WC.FIT_NU)
    full = wk.extend(X2, y2)
    assert full.inner.lml == fresh.lml
    (a1, k1), (a0, k0) = ext.inner.arrays(), fresh.arrays()
    devs = dict(lml=PRU.dev(ext.inner.lml, fresh.lml), alpha=PRU.dev(a1, a0), kinv=float(np.abs(k1 - k0).max() / np.abs(k0).max()))
    print(f"WARP extend n={n}: incremental {ext.inner.incremental}, against a fresh extend {devs}")
    assert all(v <= PRU.TOL64 for v in devs.values()), devs
    for m in (ext, full, fresh):
        m.release()
    if n != 96:
        wk.release()


def test_estimator_input_warping_is_opt_in():
    from hbetune_rs_amd import estimator as E

    X, y = WC.fit_data(96)
    est = E.EstimatorGPR.new(2).length_scale_bounds([(0.05, 5.0)] * 2).noise_bounds(1e-4, 1.0).n_restarts_optimizer(0)
    plain = est.estimate(X, y, None, E.RNG(3))
    assert isinstance(plain.fitted, gpr.FittedKernel)
    model = est.input_warping(True).estimate(X, y, None, E.RNG(3))
    assert isinstance(model.fitted, gpr.WarpedKernel) and model.lml >= plain.lml - 1e-9 * max(1.0, abs(plain.lml))
    assert model.lml - plain.lml > 1.0
    x = np.random.default_rng(4).uniform(0, 1, (5, 2))
    mean = model.predict_mean_a(x)
    assert mean.shape == (5,) and np.isfinite(mean).all()
    stats = model.predict_statistics(x[0])
    assert np.isfinite(stats.mean())
    grown = est.extend(np.vstack([X, x[:1]]), np.concatenate([y, [0.1]]), model)
    assert isinstance(grown.fitted, gpr.WarpedKernel) and grown.fitted.warp is model.fitted.warp
    plain.fitted.release(); model.fitted.release(); grown.fitted.release()
