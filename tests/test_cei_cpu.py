"""CPU checks of the constrained expected improvement (hbegp_constrained_ei_*): the NumPy restatement (tests/cei_ref.py) against
the definition cEI = E[(fmin - Y_0)^+] prod_k P[Y_k <= t_k] by quadrature and by Monte Carlo, its 2 K partials against central
differences, the n_con = 0 / fmin = +inf / permutation identities, the estimator's feasible_fmin, and the new symbols against the
header with the refusals that need no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
from scipy.special import erfc

import cei_ref as R
from hbetune_rs_amd import _lib
from hbetune_rs_amd import estimator as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hbegp_constrained_ei_f64", "hbegp_constrained_ei_f32", "hbegp_maximize_constrained_ei_f64",
       "hbegp_maximize_constrained_ei_f32", "hbegp_debug_cei_phases")
U = 2.0 ** -53  # unit roundoff

# rows (mu_0, mu_1, mu_2, mu_3), the standard deviations, fmin and the limits: improvement likely / unlikely, constraints that
# almost surely hold, hold with probability about one half, and almost surely fail
MU = np.array([[0.2, 0.1, -0.4, 1.0], [1.4, 0.9, 0.3, -2.0], [-0.5, 0.35, 0.8, 0.2], [0.7, -3.0, 0.5, 0.45], [0.6, 2.4, 0.1, 0.0]])
SD = np.array([[0.3, 0.5, 0.2, 1.1], [0.25, 0.4, 0.7, 0.3], [1.2, 0.05, 0.6, 0.9], [0.4, 0.8, 0.0, 0.35], [0.0, 0.3, 0.5, 0.2]])
FMIN = 0.65
LIMITS = np.array([0.35, 0.5, 0.4])


def _trapz(f, step, axis):
    return step * (f.sum(axis=axis) - 0.5 * (np.take(f, 0, axis=axis) + np.take(f, -1, axis=axis)))


def _ei_by_trapezoid(mu, sd, fmin, n=400001):
    """E[(fmin - Y)^+], Y ~ N(mu, sd^2), by the trapezoid rule on mu +- 8 sd (tests/test_ehvi_cpu.py's rule for G); sd = 0: the
    integrand at the point mass."""
    if sd == 0.0:
        return max(fmin - mu, 0.0)
    z = np.linspace(-8.0, 8.0, n)
    w = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return float(_trapz(np.maximum(fmin - (mu + sd * z), 0.0) * w, z[1] - z[0], 0))


_GL_X, _GL_W = np.polynomial.legendre.leggauss(64)


def _phi_by_gauss_legendre(z):
    """Phi(z) as the integral of the density over [-12, z]: 64 Gauss-Legendre nodes on each of 48 panels."""
    edges = np.linspace(-12.0, z, 49)
    half = 0.5 * (edges[1:] - edges[:-1])
    x = 0.5 * (edges[1:] + edges[:-1])[:, None] + half[:, None] * _GL_X[None, :]
    return float((half[:, None] * _GL_W[None, :] * np.exp(-0.5 * x * x)).sum() / math.sqrt(2.0 * math.pi))


def test_gauss_legendre_phi_against_erfc():
    """Tolerance 3.5e-13 = 3072 u + Phi(-12): the quadrature's own error is nil (a 64-point rule on a panel of width <= 0.44 has
    the error width^129 (64!)^4 / (129 (128!)^3) max|f^(128)| < 1e-100), the part of the integral below -12 is Phi(-12) = 1.8e-33,
    so what is left is the rounding of a sum of 3072 positive terms, each good to a few u: at most 3072 u = 3.4e-13 times the sum
    <= 1.  Measured: 3.3e-16 over 73 points of [-9, 9]."""
    worst = 0.0
    for z in np.linspace(-9.0, 9.0, 73):
        worst = max(worst, abs(_phi_by_gauss_legendre(z) - 0.5 * erfc(-z / math.sqrt(2.0))))
    print(f"Gauss-Legendre Phi against erfc: {worst:.1e}")
    assert worst <= 3072 * U + 1.8e-33 + 1e-14


@pytest.mark.parametrize("fmin", [FMIN, math.inf])
def test_restatement_against_the_definition_by_quadrature(fmin):
    """cEI = E[(fmin - Y_0)^+] prod_k Phi(z_k) with the expectation by the trapezoid and every Phi by Gauss-Legendre: no formula of
    cEI's enters.  Tolerance per row: dEI + EI * C * dPhi with
      dEI  = sigma_0 (0.399 h^2 / 8 + 1e-13), h = 16 / 400000 = 4e-5 -- the trapezoid's error at the integrand's one kink (jump of
             the slope sigma_0 times the density <= 0.399, times h^2 / 8 = 8e-11 sigma_0; the tails beyond 8 sigma hold
             sigma_0 h(-8) = 8e-17 sigma_0) plus the rounding of a 400,001-term sum;
      dPhi = 3.5e-13, test_gauss_legendre_phi_against_erfc's bound.
    The worst row has sigma_0 = 1.2: 9.6e-11 + 1e-12.  Measured: 2.0e-12 (finite fmin), 1.7e-16 (fmin = +inf, no trapezoid)."""
    val, ei, pof, _, _ = R.cei(MU, SD * SD, fmin, LIMITS)
    worst = 0.0
    for j in range(len(MU)):
        q_ei = 1.0 if math.isinf(fmin) else _ei_by_trapezoid(MU[j, 0], SD[j, 0], fmin)
        q_pof = 1.0
        for k in range(3):
            if SD[j, k + 1] == 0.0:
                q_pof *= 1.0 if LIMITS[k] > MU[j, k + 1] else 0.0
            else:
                q_pof *= _phi_by_gauss_legendre((LIMITS[k] - MU[j, k + 1]) / SD[j, k + 1])
        d_ei = 0.0 if math.isinf(fmin) else SD[j, 0] * (0.399 * (16.0 / 400000) ** 2 / 8.0 + 1e-13)
        tol = d_ei + max(q_ei, 1.0) * 3 * 3.5e-13
        worst = max(worst, abs(val[j] - q_ei * q_pof))
        assert abs(val[j] - q_ei * q_pof) <= tol, (j, val[j], q_ei * q_pof, tol)
        assert abs(pof[j] - q_pof) <= 3 * 3.5e-13 and abs(ei[j] - q_ei) <= d_ei + 1e-300
    print(f"fmin={fmin}: restatement against quadrature {worst:.1e}")


def test_monte_carlo_sanity():
    """C = 3, 4e6 independent draws of the four posteriors with a fixed seed: the mean of (fmin - y_0)^+ [y_1 <= t_1][y_2 <= t_2]
    [y_3 <= t_3] against the closed form, within 5 standard errors OF THE SAMPLE (its own standard deviation / sqrt(N)).
    Measured at row 0: closed form 0.092862, Monte Carlo 0.092793, standard error 1.1e-4."""
    j, N = 0, 4_000_000
    rng = np.random.default_rng(20141)
    y = MU[j][None, :] + SD[j][None, :] * rng.standard_normal((N, 4))
    sample = np.maximum(FMIN - y[:, 0], 0.0) * (y[:, 1:] <= LIMITS[None, :]).all(axis=1)
    mc, se = float(sample.mean()), float(sample.std(ddof=1) / math.sqrt(N))
    val = R.cei(MU[j:j + 1], (SD * SD)[j:j + 1], FMIN, LIMITS)[0][0]
    print(f"closed form {val:.6f}, Monte Carlo {mc:.6f}, standard error {se:.1e}")
    assert se > 0 and abs(val - mc) <= 5.0 * se


@pytest.mark.parametrize("fmin", [FMIN, math.inf])
def test_partials_against_central_differences(fmin):
    """The 2 K partials at the rows without a sigma = 0, step 1e-6: relative to the largest partial of the row (a partial that is 0
    up to rounding has no relative error).  Bar 1e-6: the truncation h^2 f''' / 6 ~ 1e-12 and the rounding eps f / h ~ 1e-10.
    Measured: 9.9e-11."""
    h, worst = 1e-6, 0.0
    for j in range(3):
        mu, sd = MU[j], SD[j]
        _, _, _, pm, ps = R.cei(mu[None], (sd * sd)[None], fmin, LIMITS)
        part = np.concatenate([pm[0], ps[0]])
        for k in range(4):
            for which in ("mu", "sd"):
                f = []
                for sgn in (1.0, -1.0):
                    m2, s2 = mu.copy(), sd.copy()
                    (m2 if which == "mu" else s2)[k] += sgn * h
                    f.append(R.cei(m2[None], (s2 * s2)[None], fmin, LIMITS)[0][0])
                fd = (f[0] - f[1]) / (2 * h)
                got = (pm if which == "mu" else ps)[0, k]
                worst = max(worst, abs(got - fd) / np.abs(part).max())
    print(f"fmin={fmin}: partials against central differences, relative {worst:.1e}")
    assert worst <= 1e-6


def test_gradient_is_finite_where_a_feasibility_is_exactly_zero():
    """F_2 = 0 exactly (z_2 = -40, beyond the |z| = 38 cut): the value is 0 and every partial is finite -- the weights come from
    prefix and suffix products, never from pof / F_k.  The partials of the OTHER models are 0 (their weight holds F_2), and so is
    model 2's (phi(-40) = 0)."""
    mu = np.array([[0.2, 0.1, 40.0 * 0.2 + 0.5, 1.0]])
    sd = np.array([[0.3, 0.5, 0.2, 1.1]])
    val, ei, pof, pm, ps = R.cei(mu, sd * sd, FMIN, LIMITS)
    f, _, _, _ = R.parts(mu, sd * sd, FMIN, LIMITS)
    assert f[0, 2] == 0.0 and val[0] == 0.0 and pof[0] == 0.0 and ei[0] > 0
    assert np.isfinite(pm).all() and np.isfinite(ps).all() and not pm.any() and not ps.any()
    dm = np.random.default_rng(2).standard_normal((1, 4, 5))
    _, _, _, grad, scale = R.cei_grad_x(mu, sd * sd, dm, dm, FMIN, LIMITS)
    assert np.isfinite(grad).all() and np.isfinite(scale).all()
    # one factor 0 and the weights of the others: W_1 = F_2 F_3 = 0, W_2 = F_1 F_3 > 0 (its partial vanishes through phi only)
    f2, dmu, _, _ = R.parts(mu, sd * sd, FMIN, LIMITS)
    assert f2[0, 1] * f2[0, 3] > 0 and dmu[0, 2] == 0.0


def test_without_constraints_it_is_the_expected_improvement():
    for mu, sd, fmin in [(0.4, 0.25, 0.5), (0.9, 0.5, -1.0), (-0.3, 1.0, 0.2), (0.5, 0.0, 0.7), (0.5, 0.0, 0.3), (3.0, 0.1, 0.0)]:
        val, ei, pof, _, _ = R.cei(np.array([[mu]]), np.array([[sd * sd]]), fmin, None)
        want = E.expected_improvement(mu, sd, fmin)
        assert pof[0] == 1.0 and val[0] == ei[0]
        assert abs(val[0] - want) <= 1e-15 * max(1.0, abs(fmin - mu) + sd), (mu, sd, fmin, val[0], want)


def test_infinite_fmin_gives_the_probability_of_feasibility():
    val, ei, pof, pm, ps = R.cei(MU, SD * SD, math.inf, LIMITS)
    assert (ei == 1.0).all() and val.tobytes() == pof.tobytes() and ((pof >= 0) & (pof <= 1)).all()
    assert not pm[:, 0].any() and not ps[:, 0].any()  # the objective drops out
    want = np.ones(len(MU))
    for k in range(3):
        pos = SD[:, k + 1] > 0
        with np.errstate(all="ignore"):
            want *= np.where(pos, 0.5 * erfc(-(LIMITS[k] - MU[:, k + 1]) / np.where(pos, SD[:, k + 1], 1.0) / math.sqrt(2.0)),
                             LIMITS[k] > MU[:, k + 1])
    assert np.abs(pof - want).max() <= 8 * U


def test_permuting_the_constraints_changes_rounding_only():
    v0, _, _, pm0, ps0 = R.cei(MU, SD * SD, FMIN, LIMITS)
    for perm in ([2, 0, 1], [1, 2, 0], [2, 1, 0]):
        cols = [0] + [1 + p for p in perm]
        v, _, _, pm, ps = R.cei(MU[:, cols], (SD * SD)[:, cols], FMIN, LIMITS[perm])
        assert np.abs(v - v0).max() <= 4 * U * np.abs(v0).max()  # three products in another order
        assert np.abs(pm - pm0[:, cols]).max() <= 8 * U * np.abs(pm0).max()
        assert np.abs(ps - ps0[:, cols]).max() <= 8 * U * np.abs(ps0).max()


def test_nan_rows_and_argmax_last():
    mu = MU.copy()
    mu[1, 2] = math.nan
    val, ei, pof, pm, ps = R.cei(mu, SD * SD, FMIN, LIMITS)
    assert all(math.isnan(x[1]) for x in (val, ei, pof)) and np.isnan(pm[1]).all() and np.isnan(ps[1]).all()
    keep = np.arange(len(MU)) != 1
    assert val[keep].tobytes() == R.cei(MU, SD * SD, FMIN, LIMITS)[0][keep].tobytes()
    assert R.argmax_last(np.array([0.0, 2.0, 1.0, 2.0, 0.5])) == 3


def test_feasible_fmin():
    y = np.array([3.0, 1.0, 2.0, 0.5, 2.0])
    g = np.array([[0.1, 5.0], [0.9, 1.0], [0.5, 2.0], [0.2, 9.0], [0.5, 1.5]])
    assert E.feasible_fmin(y, g, [1.0, 3.0]) == 1.0
    assert E.feasible_fmin(y, g, [0.5, 2.0]) == 2.0  # rows 2 and 4 tie; row 2 lies exactly on both limits and counts
    assert E.feasible_fmin(y, g, [0.5, 1.9]) == 2.0  # now row 4 alone
    assert E.feasible_fmin(y, g, [0.05, 100.0]) == math.inf  # no feasible row
    assert E.feasible_fmin(y, g, [1.0, 9.0]) == 0.5
    assert E.feasible_fmin(y, np.zeros((5, 0)), []) == 0.5  # no constraints: the plain minimum
    assert E.feasible_fmin([], np.zeros((0, 2)), [1.0, 1.0]) == math.inf


def test_acquire_by_constrained_ei_needs_fmin_without_shared_training_rows():
    class FK:
        def __init__(self, X):
            self.x_train, self.y_train = X, np.zeros(len(X))

    class Model:
        dtype = np.dtype(np.float64)

        def __init__(self, X):
            self.fitted = FK(X)
            self.y_norm = E.YNormalize(1.0, 0.0, "linear")

    X = np.random.default_rng(1).uniform(0, 1, (5, 2))
    with pytest.raises(ValueError, match="same rows"):
        E.acquire_by_constrained_ei(X, Model(X), [Model(X[:4])], 1, [0.5])
    with pytest.raises(ValueError, match="same rows"):
        E.acquire_by_constrained_ei(X, Model(X), [Model(X), Model(X + 1e-9)], 1, [0.5, 0.5])
    with pytest.raises(ValueError, match="limits"):
        E.acquire_by_constrained_ei(X, Model(X), [Model(X)], 1, [0.5, 0.5], fmin=1.0)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------


def test_cei_symbols_are_exported_with_the_headers_argument_counts():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "hbegp.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define\s+HBEGP_CEI_MAX_CONSTRAINTS\s+8\b", header) and _lib.CEI_MAX_CONSTRAINTS == 8
    assert lib.hbegp_version() == 200


def test_cei_calls_are_refused_before_any_device_call():
    lib = _lib.load()
    x, lim = np.zeros((1, 2)), np.zeros(9)
    none9 = (C.c_void_p * 9)(*([None] * 9))

    def call(n_con, fmin, m=1, fn=None, val=None):
        fn = fn or lib.hbegp_constrained_ei_f64
        return fn(None, none9, n_con, _lib.aptr(x.astype(np.float32) if fn is lib.hbegp_constrained_ei_f32 else x), m, fmin,
                  _lib.dptr(lim), _lib.dptr(val), None, None, None, None, None, None)

    for fn in (lib.hbegp_constrained_ei_f64, lib.hbegp_constrained_ei_f32):
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
        rc = lib.hbegp_maximize_constrained_ei_f64(None, none9, n_con, _lib.dptr(x), 1, _lib.dptr(lo), _lib.dptr(hi), fmin, _lib.dptr(lim),
                                                   10, _lib.dptr(xo), _lib.dptr(vo), None)
        assert rc == _lib.EINVAL and what in _lib.last_error(), _lib.last_error()
    rc = lib.hbegp_maximize_constrained_ei_f32(None, none9, 0, None, 0, None, None, 0.5, None, 10, None, None, None)
    assert rc == _lib.EINVAL and "S must be >= 1" in _lib.last_error()
    assert vo[0] == 7.0 and not xo.any()
    assert lib.hbegp_debug_cei_phases(0, None) == _lib.OK
