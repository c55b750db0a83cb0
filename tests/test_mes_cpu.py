"""CPU checks of max-value entropy search (hbegp_mes_* / hbegp_maximize_mes_*): the NumPy / scipy restatement (tests/mes_ref.py,
the kernel's branches) against a 60-digit table (tests/golden/mes_table.npy), the signs, the sigma = 0 and NaN rules, the
arg-max rule, a non-zero reference gradient where every gamma lies below -38, the new symbols against the header with the
refusals that need no device, and the estimator's layer with the model calls stubbed by the oracle's posterior."""
import ctypes as C
import math
import os
import re

import numpy as np

import mes_ref as R
from hbetune_rs_amd import _lib
from hbetune_rs_amd import estimator as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hbegp_mes_f64", "hbegp_mes_f32", "hbegp_maximize_mes_f64", "hbegp_maximize_mes_f32", "hbegp_debug_mes_phases")
POINTS = (-1e150, -1e7, -25.001, -25.0, -24.999, -1.0, -0.999999, 0.0, 1e-300, 8.0, 37.9, 38.5)


def _table():
    g, t, dt = np.load(os.path.join(ROOT, "tests", "golden", "mes_table.npy"))
    return g, t, dt


def test_table_holds_the_stated_points():
    g, t, dt = _table()
    want = list(np.linspace(-40.0, 8.0, 4801)) + list(-(10.0 ** np.linspace(0.0, 7.0, 400)))
    for b in R.BRANCH_POINTS:
        want += [np.nextafter(b, -np.inf), np.nextafter(b, np.inf)]
    want += list(POINTS)
    assert g.tolist() == [float(v) for v in want]
    assert len(t) == len(g) and len(dt) == len(g) and np.isfinite(t).all() and np.isfinite(dt).all()


def test_restatement_against_the_table():
    """Value: |err| <= 1e-12 max(1, |t|) or <= 1e-300 absolute.  Derivative: 1e-9 relative or 1e-290 absolute.  Measured with the
    committed restatement: the value 4.4e-14 max(1, |t|) at worst (g = -23.29, where w = a^2 (1 - au) / au cancels about
    a^2 eps), the derivative 9.2e-11 relative (g = -24.89, just below the series switch, where 1 - w cancels about a^4 eps):
    the bars are 20 and 10 times the worst cases.  The deviation is taken against the stored nearest double."""
    g, t, dt = _table()
    got_t, got_dt = R.scalar_parts(g)
    assert np.isfinite(got_t).all() and np.isfinite(got_dt).all()
    dev = np.abs(got_t - t)
    rel = dev / np.maximum(1.0, np.abs(t))
    j = int(np.argmax(rel))
    print(f"t: worst deviation {rel[j]:.1e} max(1, |t|) at g = {g[j]:.6g}")
    assert ((rel <= 1e-12) | (dev <= 1e-300)).all(), (g[j], rel[j])
    ddev = np.abs(got_dt - dt)
    with np.errstate(all="ignore"):
        drel = np.where(ddev <= 1e-290, 0.0, ddev / np.abs(dt))
    j = int(np.argmax(drel))
    print(f"t': worst relative deviation {drel[j]:.1e} at g = {g[j]:.6g}")
    assert (drel <= 1e-9).all(), (g[j], drel[j])


def test_signs_on_the_table():
    g, t, dt = _table()
    got_t, got_dt = R.scalar_parts(g)
    assert (t >= 0).all() and (dt <= 0).all()
    assert (got_t >= 0).all() and (got_dt <= 0).all()


def test_far_ends_are_finite():
    g = np.array([-1.7e308, -1e300, -1e200, 1e200, 1.7e308, -math.inf, math.inf])
    t, dt = R.scalar_parts(g)
    assert np.isfinite(t).all() and np.isfinite(dt).all() and (t >= 0).all() and (dt <= 0).all()
    assert not t[3:5].any() and not dt[3:5].any() and t[6] == 0.0


def test_sigma_zero_and_nan_rules():
    ys = np.array([-0.3, 0.1, -1.0])
    mu = np.array([0.2, 0.5, -0.4, 0.0])
    var = np.array([0.04, 0.0, 1e-33, 0.25])  # rows 1 and 2: sigma <= eps
    val, pm, ps = R.parts(mu, var, ys)
    assert val[1] == 0.0 and pm[1] == 0.0 and ps[1] == 0.0 and val[2] == 0.0 and pm[2] == 0.0 and ps[2] == 0.0
    assert (val[[0, 3]] > 0).all() and (pm[[0, 3]] < 0).all()
    dmean, dvar = np.ones((4, 3)), np.ones((4, 3))
    _, grad, scale = R.mes_grad_x(mu, var, dmean, dvar, ys)
    assert not grad[1].any() and not grad[2].any() and grad[0].all()
    bad = mu.copy()
    bad[3] = math.nan
    val2, grad2, _ = R.mes_grad_x(bad, var, dmean, dvar, ys)
    assert math.isnan(val2[3]) and np.isnan(grad2[3]).all()
    assert val2[:3].tobytes() == val[:3].tobytes() and grad2[:3].tobytes() == grad[:3].tobytes()
    badv = var.copy()
    badv[0] = math.nan
    val3, grad3, _ = R.mes_grad_x(mu, badv, dmean, dvar, ys)
    assert math.isnan(val3[0]) and np.isnan(grad3[0]).all() and val3[1:].tobytes() == val[1:].tobytes()


def test_mean_of_terms_and_one_sample():
    ys = np.array([-0.3, 0.1, -1.0, 0.05])
    mu, var = np.array([0.2, -0.6]), np.array([0.04, 0.5])
    val, pm, ps = R.parts(mu, var, ys)
    each = [R.parts(mu, var, ys[s:s + 1]) for s in range(4)]
    for k, whole in enumerate((val, pm, ps)):
        assert np.allclose(whole, np.mean([e[k] for e in each], axis=0), rtol=1e-14, atol=0)
    h = 1e-6  # the partials against central differences: truncation h^2 f''' / 6 < 1e-11, rounding u |f| / h < 1e-9
    fd_mu = (R.mes(mu + h, var, ys) - R.mes(mu - h, var, ys)) / (2 * h)
    sd = np.sqrt(var)
    fd_sd = (R.mes(mu, (sd + h) ** 2, ys) - R.mes(mu, (sd - h) ** 2, ys)) / (2 * h)
    assert np.allclose(pm, fd_mu, rtol=1e-6, atol=0) and np.allclose(ps, fd_sd, rtol=1e-6, atol=0)


def test_argmax_last():
    assert R.argmax_last(np.array([0.0, 0.3, math.nan, 0.3, 0.1])) == 3
    assert R.argmax_last(np.array([0.0, 0.0, 0.0])) == 2
    assert R.argmax_last(np.array([math.nan, math.nan])) == -1
    assert R.argmax_last(np.zeros(0)) == -1


def test_reference_gradient_is_nonzero_where_every_gamma_lies_below_minus_38():
    """The maximiser test of tests/test_gpu_mes.py starts where y* lies 50 sigma above the mean: gamma = -50 for every sample.
    From the reference alone: phi(-50) is 1e-543, far below the smallest double, yet t = 4.32 and t' = -0.02 are ordinary
    numbers, and so are both partials and the gradient."""
    mu, sd = np.array([0.3]), np.array([0.01])
    ys = mu[0] + sd[0] * np.array([50.0, 55.0, 75.0, 1e3])
    assert math.exp(-0.5 * 50.0 ** 2) == 0.0
    val, pm, ps = R.parts(mu, sd * sd, ys)
    t, dt = R.scalar_parts(np.array([-50.0]))
    assert 4.0 < t[0] < 5.0 and -0.021 < dt[0] < -0.019
    assert math.isfinite(val[0]) and val[0] > 4.0 and pm[0] < 0.0 and ps[0] < 0.0 and math.isfinite(pm[0]) and math.isfinite(ps[0])
    _, grad, _ = R.mes_grad_x(mu, sd * sd, np.array([[1.0, -2.0]]), np.array([[0.0, 0.0]]), ys)
    assert grad.all() and np.isfinite(grad).all()


# ---- ABI -----------------------------------------------------------------------------------------------------------------------


def test_mes_symbols_are_exported_with_the_headers_argument_counts():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "hbegp.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define\s+HBEGP_MES_MAX_SAMPLES\s+1024\b", header) and _lib.MES_MAX_SAMPLES == 1024
    assert _lib.MES_MAX_SAMPLES == _lib.PATHS_MAX_PATHS
    assert lib.hbegp_version() == 200


def test_mes_calls_are_refused_before_any_device_call():
    """The library looks at S and ystar before it looks at the model, so each of their refusals shows without a device."""
    lib = _lib.load()
    x, val, best = np.zeros((1, 2)), np.full(1, 7.0), C.c_int(5)
    for ys, S, what in ((np.zeros(4), 4, "NULL model"), (np.zeros(4), 0, "S must lie in [1, 1024]"),
                        (np.zeros(1025), 1025, "S must lie in [1, 1024]"), (np.array([0.0, math.nan]), 2, "ystar[1] is not finite"),
                        (np.array([math.inf]), 1, "ystar[0] is not finite"), (np.array([-math.inf]), 1, "ystar[0] is not finite"),
                        (None, 3, "ystar is NULL")):
        for fn, xs in ((lib.hbegp_mes_f64, x), (lib.hbegp_mes_f32, x.astype(np.float32))):
            rc = fn(None, _lib.aptr(xs), 1, _lib.dptr(ys), S, _lib.dptr(val), None, C.byref(best), None, None)
            assert rc == _lib.EINVAL and what in _lib.last_error(), _lib.last_error()
        lo, hi, xo, vo = np.zeros(2), np.ones(2), np.zeros((1, 2)), np.full(1, 7.0)
        rc = lib.hbegp_maximize_mes_f64(None, _lib.dptr(x), 1, _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(ys), S, 10, _lib.dptr(xo),
                                        _lib.dptr(vo), None)
        assert rc == _lib.EINVAL and what in _lib.last_error(), _lib.last_error()
        assert vo[0] == 7.0 and not xo.any()
    rc = lib.hbegp_maximize_mes_f32(None, None, 0, None, None, None, 1, 10, None, None, None)
    assert rc == _lib.EINVAL and "R must be >= 1" in _lib.last_error()
    assert val[0] == 7.0 and best.value == 5  # a refused call writes nothing
    assert lib.hbegp_debug_mes_phases(0, None) == _lib.OK


# ---- the estimator's layer over a stubbed model ------------------------------------------------------------------------------------


class _OracleFitted:
    """What SurrogateModelGPR needs of a FittedKernel for MES, from the CPU oracle: the joint posterior draws and mes()."""

    def __init__(self, X, y, noise, amp, ell, nu):
        from oracle import gpr_oracle as O

        self.O, self.X, self.amp, self.ell, self.nu = O, X, amp, ell, nu
        self.res = O.extend(X, y, noise, amp, ell, nu)
        self.d, self.n, self.lml = X.shape[1], X.shape[0], 0.0
        self.calls = []

    def _post(self, x):
        mean, var, _ = self.O.predict(x, self.X, self.res["alpha"], self.res["k_inv"], self.amp, self.ell, self.nu)
        return mean, np.maximum(var, 0.0)

    def sample_posterior(self, x, z, jitter=0.0, want_samples=True):
        x = np.asarray(x, np.float64)
        ks = self.O.product_kernel(x, self.X, self.amp, self.ell, self.nu)
        cov = self.O.product_kernel(x, x, self.amp, self.ell, self.nu) + (1e-5 + jitter) * np.eye(len(x)) - ks @ self.res["k_inv"] @ ks.T
        samples = self._post(x)[0][None, :] + np.asarray(z, np.float64) @ np.linalg.cholesky(cov).T
        self.calls.append(("sample_posterior", x.shape, np.shape(z)))
        return samples, samples.argmin(axis=1).astype(np.int32)

    def mes(self, x, ystar, want_grad=False, want_posterior=False):
        mean, var = self._post(np.asarray(x, np.float64))
        val = R.mes(mean, var, ystar)
        self.calls.append(("mes", np.shape(x), np.shape(ystar)))
        return val, R.argmax_last(val)


def _stub_model():
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 1, (40, 2))
    y = np.sin(3 * X).sum(axis=1)
    y = (y - y.mean()) / y.std()
    fk = _OracleFitted(X, y, 1e-4, 1.0, np.array([0.5, 0.5]), 2.5)
    return E.SurrogateModelGPR(fk, None, None, None, None, np.float64), fk


def test_sample_min_values_over_a_grid_with_a_stubbed_model():
    model, fk = _stub_model()
    grid = np.random.default_rng(6).uniform(0, 1, (50, 2))
    ys = model.sample_min_values(7, E.RNG.new_with_seed(3), [(0.0, 1.0)] * 2, grid=grid)
    assert ys.dtype == np.float64 and ys.shape == (7,) and np.isfinite(ys).all()
    assert fk.calls == [("sample_posterior", (50, 2), (7, 50))]
    z = E.RNG.new_with_seed(3).standard_normal((7, 50))
    samples, _ = fk.sample_posterior(grid, z)
    assert ys.tobytes() == samples.min(axis=1).tobytes()  # the row minima of the draws its own rng gives
    mean, _ = fk._post(grid)
    assert (ys <= samples.max(axis=1)).all() and ys.mean() < mean.mean()


def test_acquire_by_max_value_entropy_over_candidates_with_a_stubbed_model():
    model, fk = _stub_model()
    grid = np.random.default_rng(6).uniform(0, 1, (50, 2))
    cand = np.random.default_rng(8).uniform(0, 1, (30, 2))
    cand[11] = cand[4]  # equal rows: equal MES, the LATER index comes first
    idx, val = E.acquire_by_max_value_entropy(model, 30, E.RNG.new_with_seed(3), [(0.0, 1.0)] * 2, n_samples=7, candidates=cand, grid=grid)
    assert [c[0] for c in fk.calls] == ["sample_posterior", "mes"] and fk.calls[1][1:] == ((30, 2), (7,))
    ys = model.sample_min_values(7, E.RNG.new_with_seed(3), None, grid=grid)
    ref, _ = model.mes_a(cand, ys)
    assert idx.dtype == np.int64 and sorted(idx.tolist()) == list(range(30)) and val.tobytes() == ref[idx].tobytes()
    assert (np.diff(val) <= 0).all() and (val >= 0).all() and val[0] > val[-1]
    rest = list(range(30))
    for i in idx:  # every pick is the last index of the maximum among the rows not yet picked
        assert i == rest[R.argmax_last(ref[rest])]
        rest.remove(i)
    assert idx.tolist().index(11) + 1 == idx.tolist().index(4)
    top3, v3 = E.acquire_by_max_value_entropy(model, 3, E.RNG.new_with_seed(3), [(0.0, 1.0)] * 2, n_samples=7, candidates=cand, grid=grid)
    assert top3.tolist() == idx[:3].tolist() and v3.tobytes() == val[:3].tobytes()
