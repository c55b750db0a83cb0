"""CPU checks of the two-objective expected hypervolume improvement (hbegp_ehvi_*): the NumPy restatement (tests/ehvi_ref.py)
against direct integration of the exact hypervolume improvement, its partials against central differences, the P = 0 and front
invariance properties, the estimator's pareto_front / hypervolume_2d / default reference point, and the new symbols against
the header."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ehvi_ref as R
from hbetune_rs_amd import _lib
from hbetune_rs_amd import estimator as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hbegp_ehvi_f64", "hbegp_ehvi_f32", "hbegp_maximize_ehvi_f64", "hbegp_maximize_ehvi_f32", "hbegp_debug_ehvi_phases")
REF = np.array([1.0, 1.2])


def _front(P, seed=0):
    """P non-dominated points inside the box below REF, plus nothing else."""
    if P == 0:
        return np.zeros((0, 2))
    rng = np.random.default_rng(seed + P)
    a = np.sort(rng.uniform(0.05, 0.9, P))
    b = np.sort(rng.uniform(0.1, 1.1, P))[::-1]
    return np.stack([a, b], axis=1)


# candidates (mu1, mu2): in the middle of the front, deep in the dominated region, far below the front, outside the box in one or
# both objectives
CANDS = np.array([[0.4, 0.5], [0.95, 1.15], [-1.5, -2.0], [1.6, 0.3], [0.2, 2.0], [1.8, 1.9]])


def _hvi(front, ref, y):
    """The exact hypervolume improvement of the points y [N, 2], each on its own: hypervolume_2d of the front with the point minus
    hypervolume_2d of the front -- no formula of EHVI's enters."""
    y = np.asarray(y, np.float64).reshape(-1, 2)
    fr = np.broadcast_to(front[None], (len(y),) + front.shape)
    with_y = np.concatenate([fr, y[:, None, :]], axis=1)
    return E.hypervolume_2d(with_y, ref) - E.hypervolume_2d(front, ref)


def _trapz(f, step, axis):
    return step * (f.sum(axis=axis) - 0.5 * (np.take(f, 0, axis=axis) + np.take(f, -1, axis=axis)))


@pytest.mark.parametrize("P", [0, 1, 7])
def test_restatement_against_exact_integration_with_one_sigma_zero(P):
    """sigma_1 = 0: a 1-D trapezoid of 400,001 nodes on mu_2 +- 8 sigma_2 of the exact improvement at (mu_1, y_2).  Tolerance 1e-10.
    Measured: 5.2e-11.  The trapezoid's error is that of the integrand's kinks, each at most (jump of the slope) x density x h^2 / 8
    with h the node distance in y: 2.5 x 1.14 x (1.4e-5)^2 / 8 = 7e-11 here (40,001 nodes would leave 7e-9); the tail beyond
    8 sigma is below 1e-14."""
    front = _front(P)
    n, s2 = 400001, 0.35
    z = np.linspace(-8.0, 8.0, n)
    w = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    worst = 0.0
    for mu in CANDS:
        y = np.stack([np.full(n, mu[0]), mu[1] + s2 * z], axis=1)
        quad = _trapz(_hvi(front, REF, y) * w, z[1] - z[0], 0)
        val, _ = R.ehvi(mu[None], np.array([[0.0, s2 * s2]]), front, REF)
        worst = max(worst, abs(val[0] - quad))
        # and with the roles exchanged: sigma_2 = 0 on the transposed problem
        valt, _ = R.ehvi(mu[None, ::-1], np.array([[s2 * s2, 0.0]]), front[:, ::-1], REF[::-1])
        worst = max(worst, abs(valt[0] - quad))
    print(f"P={P}: sigma=0 quadrature deviation {worst:.1e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("P", [0, 1, 7])
def test_restatement_against_exact_integration_in_two_dimensions(P):
    """Both sigma > 0: a 2-D trapezoid of 801 x 801 nodes on +- 8 sigma.  Tolerance 2e-5.  Measured: 7.0e-7, limited by the
    integrand's kinks along the front's edges."""
    front = _front(P)
    n, s1, s2 = 801, 0.25, 0.35
    z = np.linspace(-8.0, 8.0, n)
    w = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    worst = 0.0
    for mu in CANDS:
        y1, y2 = np.meshgrid(mu[0] + s1 * z, mu[1] + s2 * z, indexing="ij")
        imp = np.concatenate([_hvi(front, REF, np.stack([y1[r0:r0 + 100].ravel(), y2[r0:r0 + 100].ravel()], axis=1))
                              for r0 in range(0, n, 100)]).reshape(n, n)
        quad = _trapz(_trapz(imp * w[None, :], z[1] - z[0], 1) * w, z[1] - z[0], 0)
        val, _ = R.ehvi(mu[None], np.array([[s1 * s1, s2 * s2]]), front, REF)
        worst = max(worst, abs(val[0] - quad))
    print(f"P={P}: 2-D quadrature deviation {worst:.1e}")
    assert worst <= 2e-5


@pytest.mark.parametrize("P", [0, 1, 7])
def test_partials_against_central_differences(P):
    front = _front(P)
    h = 1e-6
    worst = 0.0
    for mu in CANDS[:4]:
        sd = np.array([0.25, 0.35])
        val, part = R.ehvi(mu[None], (sd * sd)[None], front, REF)
        for k, (which, o) in enumerate([("mu", 0), ("sd", 0), ("mu", 1), ("sd", 1)]):
            f = []
            for sgn in (1.0, -1.0):
                m2, s2 = mu.copy(), sd.copy()
                (m2 if which == "mu" else s2)[o] += sgn * h
                f.append(R.ehvi(m2[None], (s2 * s2)[None], front, REF)[0][0])
            fd = (f[0] - f[1]) / (2 * h)
            # relative to the size of the partials at this candidate (a partial that is 0 up to rounding has no relative error)
            worst = max(worst, abs(part[0, k] - fd) / np.abs(part[0]).max())
    print(f"P={P}: partials against central differences, relative {worst:.1e}")
    assert worst <= 1e-6


def test_p0_is_the_product_of_two_expected_improvements():
    for mu, sd in [((0.4, 0.5), (0.25, 0.35)), ((0.9, 1.0), (0.5, 0.1)), ((-0.3, 0.2), (1.0, 2.0)), ((0.5, 0.7), (0.0, 0.3))]:
        val, _ = R.ehvi(np.array([mu]), np.array([[sd[0] ** 2, sd[1] ** 2]]), None, REF)
        prod = E.expected_improvement(mu[0], sd[0], REF[0]) * E.expected_improvement(mu[1], sd[1], REF[1])
        assert abs(val[0] - prod) <= 1e-14 * prod, (mu, sd, val[0], prod)


def test_front_invariance_bit_for_bit():
    rng = np.random.default_rng(5)
    front = _front(7)
    mu = rng.uniform(-0.2, 1.3, (20, 2))
    var = rng.uniform(0.0, 0.3, (20, 2)) ** 2
    var[3, 0] = 0.0
    v0, p0 = R.ehvi(mu, var, front, REF)
    dominated = front[[1, 4]] + [0.01, 0.02]
    outside = np.array([[1.0, 0.1], [0.1, 1.2], [3.0, -1.0], [-1.0, 5.0]])  # on the box's edge counts as outside
    for f in (front[rng.permutation(7)], np.vstack([front, dominated]), np.vstack([front[::-1], front[2:5]]),
              np.vstack([outside, front, dominated, front[:1]])[rng.permutation(14)]):
        v, p = R.ehvi(mu, var, f, REF)
        assert v.tobytes() == v0.tobytes() and p.tobytes() == p0.tobytes()
    assert (v0 >= 0).all()


def test_pareto_front_and_hypervolume_on_hand_made_cases():
    pts = np.array([[3.0, 1.0], [1.0, 3.0], [2.0, 2.0], [2.5, 2.5], [1.0, 3.0], [1.0, 4.0], [4.0, 1.0]])
    assert E.pareto_front(pts).tolist() == [[1.0, 3.0], [2.0, 2.0], [3.0, 1.0]]
    assert E.pareto_front(np.zeros((0, 2))).shape == (0, 2)
    assert E.pareto_front([[1.0, 1.0], [2.0, 2.0]]).tolist() == [[1.0, 1.0]]
    ref = [4.0, 4.0]
    assert E.hypervolume_2d(np.zeros((0, 2)), ref) == 0.0
    assert E.hypervolume_2d([[1.0, 1.0]], ref) == 9.0
    # the staircase (1,3), (2,2), (3,1) below (4,4): 3 x 1 + 2 x 1 + 1 x 1 = 6, with or without the dominated points
    assert E.hypervolume_2d([[1.0, 3.0], [2.0, 2.0], [3.0, 1.0]], ref) == 6.0
    assert E.hypervolume_2d(pts, ref) == 6.0
    assert E.hypervolume_2d([[5.0, 0.0], [0.0, 4.0], [4.0, 0.0]], ref) == 0.0  # outside or on the edge of the box
    assert E.hypervolume_2d([[0.0, 5.0], [2.0, 2.0]], ref) == 4.0
    hv = E.hypervolume_2d(np.array([[[1.0, 1.0], [2.0, 2.0]], [[3.0, 3.0], [2.0, 2.0]]]), ref)  # a batch of fronts
    assert hv.tolist() == [9.0, 4.0]
    # the restatement's reduction agrees with pareto_front inside the box
    a, b = R.reduce_front(pts, ref)
    assert np.stack([a, b], axis=1).tolist() == E.pareto_front(pts).tolist()


def test_default_reference_point_rule():
    r = E.default_reference_point([[1.0, 30.0], [2.0, 20.0], [3.0, 10.0]])
    assert np.allclose(r, [3.0 + 0.2, 30.0 + 2.0], rtol=0, atol=1e-15)
    r = E.default_reference_point([[0.5, -20.0]])  # one point: 10 % of max(1, |value|)
    assert np.allclose(r, [0.5 + 0.1, -20.0 + 2.0], rtol=0, atol=1e-15)
    r = E.default_reference_point([[1.0, 7.0], [2.0, 7.0]])  # no range in one objective only
    assert np.allclose(r, [2.1, 7.7], rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        E.default_reference_point(np.zeros((0, 2)))


def test_acquire_by_ehvi_needs_a_front_without_shared_training_rows():
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
        E.acquire_by_ehvi(X, [Model(X), Model(X[:4])], 1)
    with pytest.raises(ValueError, match="same rows"):
        E.acquire_by_ehvi(X, [Model(X), Model(X + 1e-9)], 1)
    with pytest.raises(ValueError, match="two models"):
        E.acquire_by_ehvi(X, [Model(X)], 1, front=[[0.0, 0.0]], ref=[1.0, 1.0])


def test_ehvi_symbols_are_exported_with_the_headers_argument_counts():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "hbegp.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_calls_without_two_models_are_refused_before_any_device_call():
    lib = _lib.load()
    x, val, ref = np.zeros((1, 2)), np.zeros(1), np.array([1.0, 1.0])
    none2 = (C.c_void_p * 2)(None, None)
    for n_obj in (1, 3):
        rc = lib.hbegp_ehvi_f64(none2, n_obj, _lib.dptr(x), 1, None, 0, _lib.dptr(ref), _lib.dptr(val), None, None, None, None)
        assert rc == _lib.EINVAL and "n_obj must be 2" in _lib.last_error()
    rc = lib.hbegp_ehvi_f64(none2, 2, _lib.dptr(x), 1, None, 0, _lib.dptr(ref), _lib.dptr(val), None, None, None, None)
    assert rc == _lib.EINVAL and "NULL model" in _lib.last_error()
    rc = lib.hbegp_ehvi_f32(None, 2, None, 0, None, 0, _lib.dptr(ref), None, None, None, None, None)
    assert rc == _lib.EINVAL and "models is NULL" in _lib.last_error()
    rc = lib.hbegp_ehvi_f64(none2, 2, None, -1, None, 0, _lib.dptr(ref), None, None, None, None, None)
    assert rc == _lib.EINVAL and "m must be >= 0" in _lib.last_error()
    rc = lib.hbegp_ehvi_f64(none2, 2, None, 0, None, -1, _lib.dptr(ref), None, None, None, None, None)
    assert rc == _lib.EINVAL and "P must be >= 0" in _lib.last_error()
    rc = lib.hbegp_maximize_ehvi_f64(none2, 2, _lib.dptr(x), 0, None, None, None, 0, _lib.dptr(ref), 10, None, None, None)
    assert rc == _lib.EINVAL and "S must be >= 1" in _lib.last_error()
    assert lib.hbegp_debug_ehvi_phases(0, None) == _lib.OK
