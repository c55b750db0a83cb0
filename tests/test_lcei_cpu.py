"""CPU checks of the log-space constrained expected improvement (hbegp_log_constrained_ei_*): the NumPy / scipy restatement
(tests/lcei_ref.py, the kernel's branches) against a 60-digit table (tests/golden/logei_table.json), against the logarithm of the
plain-space restatement (tests/cei_ref.py) where that is normal, its partials against central differences, the identities and
limits of the definition, the dead zone where plain space gives exactly 0, the dead-zone search of tests/test_gpu_lcei.py with the
reference and the library's host L-BFGS alone, and the new symbols against the header with the refusals that need no device."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import cei_ref as CR
import lcei_cases as S
import lcei_ref as R
from hbetune_rs_amd import _lib, gpr
from test_cei_cpu import FMIN, LIMITS, MU, SD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hbegp_log_constrained_ei_f64", "hbegp_log_constrained_ei_f32", "hbegp_maximize_log_constrained_ei_f64",
       "hbegp_maximize_log_constrained_ei_f32", "hbegp_debug_lcei_phases")
U = 2.0 ** -53  # unit roundoff
POS = [0, 1, 2]  # the rows of MU / SD without a sigma = 0


def _table():
    with open(os.path.join(ROOT, "tests", "golden", "logei_table.json")) as f:
        t = json.load(f)
    z = np.array([float.fromhex(r["z"]) for r in t["rows"]])
    return t, z


def test_table_holds_the_stated_points():
    t, z = _table()
    want = list(np.linspace(-40.0, 10.0, 201)) + list(-(10.0 ** np.linspace(0.0, 8.0, 81)))
    for b in R.BRANCH_POINTS:
        want += [b - 1e-6, b + 1e-6]
    want += [38.0, -38.0, 50.0, 1e3]
    assert z.tolist() == [float(v) for v in want]
    assert t["functions"] == ["log_h", "cdf_over_h", "pdf_over_h", "log_cdf", "pdf_over_cdf"]
    for r in t["rows"]:  # the nearest double of each decimal string is the stored double
        for name in t["functions"]:
            assert float(r[name]["decimal"]) == float.fromhex(r[name]["double"]), (r["z"], name)


def test_restatement_against_the_table():
    """|dev| <= 1e-11 max(1, |true|) for log h, Phi / h, phi / h, log Phi and phi / Phi at all 292 z of the table.  Where the bar
    comes from: below the switch point a = 25 the form b = 1 - a u loses a^2 eps to cancellation, at most 625 * 1.1e-16 = 7e-14
    times the few ulp of erfcx; everywhere else every form is a few ulp.  Measured here: 1.5e-13 (Phi / h and phi / h at z = -24),
    8.5e-16 for log h, 3.1e-16 / 6.0e-16 for log Phi and phi / Phi.  The bar is about 60 times the worst.  The deviation is taken
    against the stored nearest double, which is within u |true| of the 60-digit value."""
    t, z = _table()
    got = R.scalar_parts(z)
    for i, name in enumerate(t["functions"]):
        true = np.array([float.fromhex(r[name]["double"]) for r in t["rows"]])
        dev = np.abs(got[i] - true) / np.maximum(1.0, np.abs(true))
        j = int(np.argmax(dev))
        print(f"{name}: worst deviation {dev[j]:.1e} at z = {z[j]:.6g}")
        assert np.isfinite(got[i]).all()
        assert dev[j] <= 1e-11, (name, z[j], dev[j])


def _kappa(mu, sd, fmin):
    """The cancellation factor of the PLAIN form h = phi(a) - a Phi(-a) that cei_ref evaluates for z_0 = -a < 0:
    (phi + a Phi(-a)) / h = q + a r; 1 for z_0 >= 0."""
    z = (fmin - mu[:, 0]) / sd[:, 0]
    _, r, q, _, _ = R.scalar_parts(z)
    return np.where(z < 0, q + np.abs(z) * r, 1.0)


@pytest.mark.parametrize("fmin", [FMIN, math.inf])
def test_agrees_with_the_logarithm_of_plain_space_where_that_is_normal(fmin):
    """Rows of test_cei_cpu.py without a sigma = 0.  Bar for the value: 16 u (1 + |log cei|) kappa.  cei_ref's cei is a product of
    1 + C factors, each from erfc and exp (2 u each) and, for EI with z_0 = -a < 0, the difference phi - a Phi(-a), which amplifies
    them by kappa = (phi + a Phi(-a)) / h (22 at z_0 = -3): a relative error of at most (4 kappa + 4 C + C) u <= 8 u kappa for
    C = 3, which is the absolute error of log(cei_ref).  The log side adds u per term and per addition relative to the partial sums,
    <= 8 u (1 + |log cei|).  The partials equal cei_ref's divided by cei within 32 u kappa (the same errors once more for the
    partial and for the division), relative to the larger of the row's partials.  Measured: values 2.3e-14 against a bar of
    5.2e-13 and partials 2.2e-14 of the row's largest at the row with kappa = 22, 2e-16 elsewhere."""
    mu, sd = MU[POS], SD[POS]
    val, lei, lpof, pm, ps = R.lcei(mu, sd * sd, fmin, LIMITS)
    cv, cei_, cpof, cpm, cps = CR.cei(mu, sd * sd, fmin, LIMITS)
    assert (cv > 1e-300).all()
    kap = np.ones(len(mu)) if math.isinf(fmin) else _kappa(mu, sd, fmin)
    bar = 16 * U * (1.0 + np.abs(np.log(cv))) * kap
    dev = np.abs(val - np.log(cv))
    print(f"fmin={fmin}: lcei against log(cei_ref): worst {dev.max():.1e}, bars {bar}, kappa {kap}")
    assert (dev <= bar).all(), (dev, bar)
    assert (np.abs(lei - np.log(cei_)) <= bar).all() and (np.abs(lpof - np.log(cpof)) <= bar).all()
    want_m, want_s = cpm / cv[:, None], cps / cv[:, None]
    size = np.maximum(np.abs(want_m), np.abs(want_s)).max(axis=1)
    pdev = np.maximum(np.abs(pm - want_m), np.abs(ps - want_s)).max(axis=1)
    print(f"fmin={fmin}: partials against cei_ref's / cei: worst {(pdev / size).max():.1e} of the row's largest partial")
    assert (pdev <= 32 * U * kap * size).all(), (pdev, size)


@pytest.mark.parametrize("z", [-300.0, -30.0, -5.0, 0.0, 3.0])
def test_partials_against_central_differences(z):
    """Both terms' partials w.r.t. mu and sigma at sigma = 0.7, t = mu + z sigma, step 1e-6: relative to the larger partial of the
    term.  Bar 1e-6: the truncation h^2 f''' / 6 is below 1e-11, the rounding u |f| / h is 5e-6 |f| u / u = at most
    1.1e-16 * 4.5e4 / 1e-6 = 5e-6 absolute at z = -300 where the partials are about 430 and 1.3e5 (1.2e-8 relative), and smaller
    elsewhere.  Measured: 2.9e-10 at worst."""
    h, sd, mu = 1e-6, 0.7, 0.3
    t = mu + z * sd

    def terms(m, s):
        v, _, _, _ = R.parts(np.array([[m, m]]), np.array([[s * s, s * s]]), t, [t])
        return v[0]

    _, dmu, dsd, _ = R.parts(np.array([[mu, mu]]), np.array([[sd * sd, sd * sd]]), t, [t])
    fd_mu = (terms(mu + h, sd) - terms(mu - h, sd)) / (2 * h)
    fd_sd = (terms(mu, sd + h) - terms(mu, sd - h)) / (2 * h)
    for k in range(2):
        size = max(abs(dmu[0, k]), abs(dsd[0, k]))
        rel = max(abs(dmu[0, k] - fd_mu[k]), abs(dsd[0, k] - fd_sd[k])) / size
        print(f"z={z}: term {k}: partials {dmu[0, k]:.6e} {dsd[0, k]:.6e}, central differences deviate by {rel:.1e}")
        assert rel <= 1e-6


def test_identities():
    var = SD * SD
    # n_con = 0: lcei is lei, lpof is 0.0
    val, lei, lpof, _, _ = R.lcei(MU[:, :1], var[:, :1], FMIN, None)
    assert val.tobytes() == lei.tobytes() and not lpof.any()
    # fmin = +inf: lcei is lpof, the objective drops out
    val, lei, lpof, pm, ps = R.lcei(MU, var, math.inf, LIMITS)
    assert val.tobytes() == lpof.tobytes() and not lei.any() and not pm[:, 0].any() and not ps[:, 0].any()
    # permuting the constraints: three additions in another order, each within u of a partial sum that is at most sum_k |lF_k|:
    # 2 * 3 u sum_k |lF_k| covers both orders
    v0, _, p0, pm0, ps0 = R.lcei(MU[POS], var[POS], FMIN, LIMITS)
    terms = np.abs(R.parts(MU[POS], var[POS], FMIN, LIMITS)[0])
    for perm in ([2, 0, 1], [1, 2, 0], [2, 1, 0]):
        cols = [0] + [1 + p for p in perm]
        v, _, p, pm, ps = R.lcei(MU[POS][:, cols], var[POS][:, cols], FMIN, LIMITS[perm])
        assert (np.abs(p - p0) <= 6 * U * terms[:, 1:].sum(axis=1)).all()
        assert (np.abs(v - v0) <= 8 * U * terms.sum(axis=1)).all()
        assert pm.tobytes() == pm0[:, cols].tobytes() and ps.tobytes() == ps0[:, cols].tobytes()  # a term's partials are its own


def test_sigma_zero_and_minus_infinity_rules():
    var = SD * SD
    v, dmu, dsd, _ = R.parts(MU, var, FMIN, LIMITS)
    # row 3: sigma_2 = 0 with t_2 = 0.5 = mu_2: not below the limit -> -inf, both partials 0
    assert v[3, 2] == -math.inf and dmu[3, 2] == 0.0 and dsd[3, 2] == 0.0
    # row 4: sigma_0 = 0 with fmin - mu_0 = 0.05 > 0: log of the gap, -1 / gap, 0
    assert v[4, 0] == math.log(FMIN - 0.6) and dmu[4, 0] == -1.0 / (FMIN - 0.6) and dsd[4, 0] == 0.0
    val, lei, lpof, pm, ps = R.lcei(MU, var, FMIN, LIMITS)
    assert val[3] == -math.inf and lpof[3] == -math.inf and math.isfinite(lei[3])
    assert np.isfinite(pm[3]).all() and np.isfinite(ps[3]).all() and pm[3, 0] != 0.0  # the gradient is the sum of the finite partials
    assert np.isfinite(val[[0, 1, 2, 4]]).all()
    # sigma_0 = 0 at or above fmin: -inf with zero partials; a sigma_k = 0 below the limit: exactly 0
    v, dmu, dsd, _ = R.parts(np.array([[0.7, 0.1], [0.65, 0.1]]), np.zeros((2, 2)), FMIN, [0.35])
    assert (v[:, 0] == -math.inf).all() and not dmu.any() and not dsd.any() and (v[:, 1] == 0.0).all()
    # -inf wins the arg-max only where nothing finite exists; a NaN never does
    assert R.argmax_last(np.array([-math.inf, -3.0, math.nan, -math.inf])) == 1
    assert R.argmax_last(np.array([-math.inf, math.nan, -math.inf])) == 2


def test_nan_stays_in_its_row():
    mu = MU.copy()
    mu[1, 2] = math.nan
    val, lei, lpof, pm, ps = R.lcei(mu, SD * SD, FMIN, LIMITS)
    assert all(math.isnan(x[1]) for x in (val, lei, lpof)) and np.isnan(pm[1]).all() and np.isnan(ps[1]).all()
    keep = np.arange(len(MU)) != 1
    clean = R.lcei(MU, SD * SD, FMIN, LIMITS)
    assert val[keep].tobytes() == clean[0][keep].tobytes() and pm[keep].tobytes() == clean[3][keep].tobytes()
    assert not np.isnan(val[keep]).any()


def test_far_ends_are_never_nan():
    """|z| up to 1e150 gives finite values; beyond, -inf on the far side and a finite value on the near side, never NaN."""
    z = np.array([-1.7e308, -1e200, -1e150, -1e100, 1e100, 1e150, 1e200, 1.7e308, -math.inf, math.inf])
    parts = R.scalar_parts(z)
    for p in parts:
        assert not np.isnan(p).any()
    lh, _, _, lphi, _ = parts
    assert np.isfinite(lh[2:6]).all() and np.isfinite(lphi[2:6]).all()
    assert (lh[:2] == -math.inf).all() and (lphi[:2] == -math.inf).all() and np.isfinite(lh[6:8]).all() and (lphi[4:8] == 0.0).all()


def test_dead_zone_has_values_and_gradients_where_plain_space_has_none():
    """z_0 and every z_k between -50 and -1e4: cei_ref gives exactly 0 with zero partials, the restatement finite values and
    nonzero finite partials for every model."""
    zs = -np.array([50.0, 80.0, 200.0, 1e3, 3e3, 1e4])
    sd = np.array([0.3, 0.05, 0.8, 0.01])
    mu = np.array([0.2, -0.4, 1.0, 0.5])
    for fmin_on in (True, False):
        for z in zs:
            fmin = float(mu[0] + z * sd[0]) if fmin_on else math.inf
            limits = mu[1:] + z * np.array([1.0, 0.7, 1.3]) * sd[1:]
            cv, _, _, cpm, cps = CR.cei(mu[None], (sd * sd)[None], fmin, limits)
            assert cv[0] == 0.0 and not cpm.any() and not cps.any()
            val, lei, lpof, pm, ps = R.lcei(mu[None], (sd * sd)[None], fmin, limits)
            assert math.isfinite(val[0]) and val[0] < -1000 and np.isfinite(pm).all() and np.isfinite(ps).all()
            first = 0 if fmin_on else 1
            assert (pm[0, first:] != 0).all() and (ps[0, first:] != 0).all()
            assert (pm[0, first:] < 0).all() and (ps[0, first:] > 0).all()  # a lower mean and a wider sigma both help


def test_dead_zone_search_with_the_reference_and_the_host_lbfgs():
    """The inputs of tests/test_gpu_lcei.py's dead-zone search (tests/lcei_cases.py), with the oracle's posterior, the restatement
    and the library's host L-BFGS (gpr.minimize_by_gradient) alone -- no device.  The posterior's gradient w.r.t. x is a central
    difference (step 1e-6) of the oracle's predict.  Conditions, the ones the device has to meet: every start has plain-space
    pof exactly 0; every run ends at a strictly larger lcei than its start; at least one ends at pof >= 0.5.  Measured: z between
    -54 and -198 at the starts, six of six runs improve, three of six end at pof = 1.000."""
    from oracle import gpr_oracle as O

    X = S.training_rows()
    g = S.constraint_targets(X)
    th = S.thetas()[1]
    noise, amp, ell = math.exp(th[0]), math.exp(th[1]), np.exp(th[2:])
    res = O.extend(X, g, noise, amp, ell, S.NU)

    def post(x):
        m, v, _ = O.predict(np.atleast_2d(x), X, res["alpha"], res["k_inv"], amp, ell, S.NU)
        return m[0], v[0]

    def pof_plain(x):
        m, v = post(x)
        return CR.cei(np.array([[0.0, m]]), np.array([[1.0, v]]), math.inf, [S.LIMIT])[0][0]

    def objective(x):
        h = 1e-6
        m, v = post(x)
        dmean, dvar = np.zeros((1, 2, S.D)), np.zeros((1, 2, S.D))
        for i in range(S.D):
            e = np.zeros(S.D)
            e[i] = h
            (mp, vp), (mm, vm) = post(x + e), post(x - e)
            dmean[0, 1, i], dvar[0, 1, i] = (mp - mm) / (2 * h), (vp - vm) / (2 * h)
        val, _, _, grad, _ = R.lcei_grad_x(np.array([[0.0, m]]), np.array([[1.0, v]]), dmean, dvar, math.inf, [S.LIMIT])
        return -val[0], -grad[0]

    reached = 0
    for s in S.starts():
        m, v = post(s)
        z = (S.LIMIT - m) / math.sqrt(v)
        start = -objective(s)[0]
        assert pof_plain(s) == 0.0 and z < -38.0 and math.isfinite(start)
        f, x = gpr.minimize_by_gradient(objective, s, S.BOUNDS, maxeval=S.MAXEVAL)
        end_pof = pof_plain(x)
        print(f"start z = {z:8.1f} lcei = {start:10.2f} -> lcei = {-f:9.3f} pof = {end_pof:.4f} at x = {x}")
        assert -f > start
        reached += end_pof >= 0.5
    assert reached >= 1


# ---- ABI -----------------------------------------------------------------------------------------------------------------------


def test_lcei_symbols_are_exported_with_the_headers_argument_counts():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "hbegp.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    for old, new in (("hbegp_constrained_ei_f64", "hbegp_log_constrained_ei_f64"), ("hbegp_constrained_ei_f32", "hbegp_log_constrained_ei_f32"),
                     ("hbegp_maximize_constrained_ei_f64", "hbegp_maximize_log_constrained_ei_f64"),
                     ("hbegp_maximize_constrained_ei_f32", "hbegp_maximize_log_constrained_ei_f32")):
        assert _lib.SIGNATURES[old] == _lib.SIGNATURES[new]  # the argument list of the plain-space call
    assert "There is no log-space form" not in header
    assert lib.hbegp_version() == 200


def test_lcei_calls_are_refused_before_any_device_call():
    lib = _lib.load()
    x, lim = np.zeros((1, 2)), np.zeros(9)
    none9 = (C.c_void_p * 9)(*([None] * 9))

    def call(n_con, fmin, m=1, fn=None, val=None):
        fn = fn or lib.hbegp_log_constrained_ei_f64
        return fn(None, none9, n_con, _lib.aptr(x.astype(np.float32) if fn is lib.hbegp_log_constrained_ei_f32 else x), m, fmin,
                  _lib.dptr(lim), _lib.dptr(val), None, None, None, None, None, None)

    for fn in (lib.hbegp_log_constrained_ei_f64, lib.hbegp_log_constrained_ei_f32):
        val = np.full(1, 7.0)
        assert call(0, 0.5, fn=fn, val=val) == _lib.EINVAL and "NULL objective" in _lib.last_error()
        assert call(9, 0.5, fn=fn, val=val) == _lib.EINVAL and "n_con must lie in [0, 8]" in _lib.last_error()
        assert call(-1, 0.5, fn=fn, val=val) == _lib.EINVAL and "n_con must lie in [0, 8]" in _lib.last_error()
        assert call(0, math.inf, fn=fn, val=val) == _lib.EINVAL and "nothing to compute" in _lib.last_error()
        assert call(1, math.nan, fn=fn, val=val) == _lib.EINVAL and "fmin_normalized" in _lib.last_error()
        assert call(1, -math.inf, fn=fn, val=val) == _lib.EINVAL and "fmin_normalized" in _lib.last_error()
        assert call(1, 0.5, m=-1, fn=fn, val=val) == _lib.EINVAL and "m must be >= 0" in _lib.last_error()
        assert val[0] == 7.0  # a refused call writes nothing
    lo, hi, xo, vo = np.zeros(2), np.ones(2), np.zeros((1, 2)), np.full(1, 7.0)
    for n_con, fmin, what in ((0, 0.5, "NULL objective"), (9, 0.5, "n_con must lie"), (-1, 0.5, "n_con must lie"),
                              (0, math.inf, "nothing to compute"), (2, math.nan, "fmin_normalized")):
        rc = lib.hbegp_maximize_log_constrained_ei_f64(None, none9, n_con, _lib.dptr(x), 1, _lib.dptr(lo), _lib.dptr(hi), fmin,
                                                       _lib.dptr(lim), 10, _lib.dptr(xo), _lib.dptr(vo), None)
        assert rc == _lib.EINVAL and what in _lib.last_error(), _lib.last_error()
    rc = lib.hbegp_maximize_log_constrained_ei_f32(None, none9, 0, None, 0, None, None, 0.5, None, 10, None, None, None)
    assert rc == _lib.EINVAL and "S must be >= 1" in _lib.last_error()
    assert vo[0] == 7.0 and not xo.any()
    assert lib.hbegp_debug_lcei_phases(0, None) == _lib.OK
