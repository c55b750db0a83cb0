"""CPU checks of the expected hypervolume improvement of two to four objectives (hbegp_ehvi_nd_*): the box decomposition of the
NumPy restatement (tests/ehvi_nd_ref.py) and of the library (hbegp_debug_ehvi_boxes, host only) against the exact hypervolume
(estimator.hypervolume_nd: slicing, no formula of EHVI's); the restatement against direct integration, against the two-objective
restatement, against central differences and under permutations of the objectives; the estimator's pareto_front_nd /
hypervolume_nd / default_reference_point_nd; the new symbols, the box cap and the refusals that need no device; the spill counts
of the new kernel's instantiations."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import ehvi_nd_ref as R
import ehvi_ref as R2
from test_isa_guards_cpu import _kernel_notes, isa  # noqa: F401  (isa: the fixture that builds the kernels' gfx950 assembly)
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hbegp_ehvi_nd_f64", "hbegp_ehvi_nd_f32", "hbegp_maximize_ehvi_nd_f64", "hbegp_maximize_ehvi_nd_f32",
       "hbegp_debug_ehvi_nd_phases", "hbegp_debug_ehvi_boxes")
REF = np.array([1.0, 1.2, 1.1, 1.05])


def _shell(P, M, seed=0):
    """P mutually non-dominated points inside the box below REF[:M]: the positive part of a sphere shell."""
    if P == 0:
        return np.zeros((0, M))
    x = np.abs(np.random.default_rng(seed + 10 * P + M).standard_normal((P, M))) + 0.05
    return 0.05 + 0.9 * x / np.linalg.norm(x, axis=1, keepdims=True)


def _front(P, M, seed=0):
    """(front, ref): the shell with two points sharing their coordinate in objective 0 (P >= 2), and behind it dominated points, a
    duplicate and points outside the box (one of them on its edge)."""
    ref = REF[:M].copy()
    f = _shell(P, M, seed)
    if P >= 2:  # two neighbours along objective 0 (with two objectives one of them then dominates the other)
        order = np.argsort(f[:, 0])
        f[order[P // 2], 0] = f[order[P // 2 - 1], 0]
    if P == 0:
        return f, ref
    out = np.vstack([f[0], f[0]])
    out[0, 0] = ref[0]  # on the edge: outside
    out[1, M - 1] = ref[M - 1] + 1.0
    return np.vstack([f, f[: min(P, 3)] + 0.01, f[:1], out]), ref


def _scale(front, ref):
    """H = prod_k (r_k - min_k), the minimum over the points inside the box (r_k without any)."""
    return R.box_scale(np.zeros(len(ref)), front, ref)


def _hvi(front, ref, y):
    """The exact hypervolume improvement of the points y [N, M], each on its own: hypervolume_nd of the front with the point minus
    hypervolume_nd of the front."""
    y = np.asarray(y, np.float64).reshape(-1, len(ref))
    fr = np.broadcast_to(front[None], (len(y),) + front.shape)
    return E.hypervolume_nd(np.concatenate([fr, y[:, None, :]], axis=1), ref) - E.hypervolume_nd(front, ref)


def _probe_points(front, ref, n, seed):
    """Random y inside the box, below the front in every objective, and outside the box in one or all objectives."""
    rng = np.random.default_rng(seed)
    M = len(ref)
    inside = rng.uniform(0.0, ref, (n, M))
    below = rng.uniform(-0.5, 0.05, (n // 4, M))
    out_one = rng.uniform(0.0, ref, (n // 4, M))
    out_one[np.arange(n // 4), rng.integers(0, M, n // 4)] += ref.max()
    out_all = ref + rng.uniform(0.0, 0.5, (n // 4, M))
    on_front = front[: min(len(front), 4)] if len(front) else np.zeros((0, M))
    return np.vstack([inside, below, out_one, out_all, on_front])


def _check_boxes(thr, bx, front, ref, what):
    """The three properties of a decomposition; returns the worst deviation over the bar."""
    M = len(ref)
    assert bx.ndim == 3 and bx.shape[1:] == (M, 2) and len(bx) >= 1
    for k in range(M):
        assert thr[k][0] == -math.inf and thr[k][-1] == ref[k] and (np.diff(thr[k]) > 0).all()
        assert (bx[:, k, 0] < bx[:, k, 1]).all() and bx[:, k].min() >= 0 and bx[:, k].max() <= len(thr[k]) - 1
    # 1. pairwise disjoint: two boxes are apart in at least one objective
    apart = np.zeros((len(bx), len(bx)), dtype=bool)
    for k in range(M):
        apart |= (bx[:, None, k, 1] <= bx[None, :, k, 0]) | (bx[None, :, k, 1] <= bx[:, None, k, 0])
    assert (apart | np.eye(len(bx), dtype=bool)).all(), what
    bar = 1e-12 * max(1.0, _scale(front, ref))
    # 2. the boxes clipped to [c, r), c below every point: vol - hypervolume
    inside = front[(front < ref).all(axis=1)] if len(front) else front
    c = (inside.min(axis=0) if len(inside) else ref) - 0.3
    vol = R.hvi_boxes(thr, bx, c[None])[0]
    dev = abs(vol - (np.prod(ref - c) - E.hypervolume_nd(front, ref)))
    # 3. the improvement by the boxes alone against the exact hypervolume difference
    y = _probe_points(inside, ref, 48, 7 + len(front))
    dev = max(dev, float(np.abs(R.hvi_boxes(thr, bx, y) - _hvi(front, ref, y)).max()))
    assert dev <= bar, (what, dev, bar)
    return dev / bar


@pytest.mark.parametrize("M", [2, 3, 4])
def test_boxes_of_both_implementations_tile_the_free_region(M):
    """Bar: 1e-12 x max(1, H), H = prod_k (r_k - min_k).  Measured worst deviation: DESIGN section 28."""
    worst = 0.0
    for P in (0, 1, 2, 7, 30):
        front, ref = _front(P, M)
        thr_r, bx_r = R.boxes(front, ref)
        thr_l, bx_l = gpr.ehvi_boxes(front, ref)
        worst = max(worst, _check_boxes(thr_r, bx_r, front, ref, ("restatement", M, P)))
        worst = max(worst, _check_boxes(thr_l, bx_l, front, ref, ("library", M, P)))
        # the two sweeps go over the objectives in the same order: the same thresholds and the same boxes in the same order
        assert all(a.tobytes() == b.tobytes() for a, b in zip(thr_r, thr_l)) and bx_r.tobytes() == bx_l.tobytes()
        # the front shuffled: the same boxes, byte for byte
        perm = np.random.default_rng(P).permutation(len(front))
        for thr0, bx0, fn in ((thr_r, bx_r, R.boxes), (thr_l, bx_l, gpr.ehvi_boxes)):
            thr_s, bx_s = fn(front[perm], ref)
            assert bx_s.tobytes() == bx0.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(thr_s, thr0))
        print(f"M={M} P={P}: {len(R.reduce_front(front, ref))} points on the front, {len(bx_l)} boxes")
    print(f"M={M}: worst deviation / bar {worst:.1e}")


def test_counts_without_caps_and_too_small_caps():
    lib = _lib.load()
    front, ref = _front(7, 3)
    thr, bx = gpr.ehvi_boxes(front, ref)
    ip = C.POINTER(C.c_int)
    counts, nb = np.zeros(3, np.int32), C.c_int(0)
    assert lib.hbegp_debug_ehvi_boxes(_lib.dptr(front), len(front), 3, _lib.dptr(ref), counts.ctypes.data_as(ip), None, 0, C.byref(nb),
                                      None, 0) == _lib.OK
    assert counts.tolist() == [len(t) for t in thr] and nb.value == len(bx)
    buf, bb = np.zeros(int(counts.sum())), np.zeros((nb.value, 3, 2), np.int32)
    rc = lib.hbegp_debug_ehvi_boxes(_lib.dptr(front), len(front), 3, _lib.dptr(ref), counts.ctypes.data_as(ip), _lib.dptr(buf), len(buf),
                                    C.byref(nb), bb.ctypes.data_as(ip), nb.value - 1)
    assert rc == _lib.EINVAL and "below the counts" in _lib.last_error()


def _trapz(f, step, axis):
    return step * (f.sum(axis=axis) - 0.5 * (np.take(f, 0, axis=axis) + np.take(f, -1, axis=axis)))


# candidates: in the middle of the front, deep in the dominated region, below the front, outside the box in one objective
CANDS = np.array([[0.4, 0.5, 0.45, 0.5], [0.95, 1.15, 1.05, 1.0], [-0.5, -0.6, -0.4, -0.3], [1.6, 0.3, 0.5, 0.4]])


@pytest.mark.parametrize("M,P", [(3, 0), (3, 1), (3, 7), (4, 0), (4, 2)])
def test_restatement_against_exact_integration_with_one_sigma_positive(M, P):
    """sigma > 0 in one objective only (the last, then the first): a 1-D trapezoid of 400,001 nodes on mu +- 8 sigma of the exact
    improvement at the other objectives' means.  Tolerance 1e-9.  The integrand is piecewise linear in the live objective, its
    slope the (M - 1)-volume of the free cross-section beyond y: it falls from at most S = prod_{k != live} (r_k - mu_k) to 0, so its
    kinks' jumps add up to S at the most, and the trapezoid's error is below S x density x h^2 / 8 with h the node distance in
    y (tests/test_ehvi_cpu.py's bound): S <= 4.1 (M = 4, the candidate below the front), density <= 1.14, h = 1.4e-5 give 1.2e-10;
    40,001 nodes would leave 1.2e-8.  The tail beyond 8 sigma is below 1e-14."""
    front, ref = _front(P, M)
    n, s = 400001, 0.35
    z = np.linspace(-8.0, 8.0, n)
    w = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    dec = R.boxes(front, ref)
    exact_front = R.reduce_front(front, ref)  # the same hypervolumes from fewer points
    worst = 0.0
    for mu in CANDS[:, :M]:
        for live in (M - 1, 0):
            S = float(np.prod(np.maximum(np.delete(ref - mu, live), 0.0)))
            assert S * (0.3990 / s) * (16.0 * s / (n - 1)) ** 2 / 8.0 <= 2e-10
            y = np.repeat(mu[None], n, axis=0)
            y[:, live] = mu[live] + s * z
            quad = _trapz(_hvi(exact_front, ref, y) * w, z[1] - z[0], 0)
            var = np.zeros((1, M))
            var[0, live] = s * s
            val, _ = R.ehvi(mu[None], var, front, ref, dec)
            worst = max(worst, abs(val[0] - quad))
    print(f"M={M} P={P}: one-sigma quadrature deviation {worst:.1e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("P", [0, 1, 7, 30])
def test_two_objectives_agree_with_the_strip_sum(P):
    """n_obj = 2 against tests/ehvi_ref.py with both sigma > 0 (and one at 0): 1e-13 x max(1, H)."""
    front, ref = _front(P, 2)
    rng = np.random.default_rng(3)
    mu = np.vstack([CANDS[:, :2], rng.uniform(-0.2, 1.3, (20, 2))])
    var = rng.uniform(0.05, 0.4, mu.shape) ** 2
    var[5, 1] = 0.0
    v2, p2 = R2.ehvi(mu, var, front, ref)
    v, p = R.ehvi(mu, var, front, ref)
    bar = 1e-13 * max(1.0, _scale(front, ref))
    print(f"P={P}: boxes against strips {np.abs(v - v2).max():.1e}, partials {np.abs(p - p2).max():.1e} (bar {bar:.1e})")
    assert np.abs(v - v2).max() <= bar
    assert np.abs(p - p2).max() <= 10 * bar  # (the partials are per unit of mu or sigma: densities up to 1 / sigma = 20 enter)


@pytest.mark.parametrize("M", [2, 3, 4])
@pytest.mark.parametrize("P", [0, 1, 7])
def test_partials_against_central_differences(M, P):
    front, ref = _front(P, M)
    dec = R.boxes(front, ref)
    h = 1e-6
    worst = 0.0
    sd = np.array([0.25, 0.35, 0.3, 0.2])[:M]
    for mu in CANDS[:, :M]:
        val, part = R.ehvi(mu[None], (sd * sd)[None], front, ref, dec)
        for k in range(2 * M):
            f = []
            for sgn in (1.0, -1.0):
                m2, s2 = mu.copy(), sd.copy()
                (s2 if k % 2 else m2)[k // 2] += sgn * h
                f.append(R.ehvi(m2[None], (s2 * s2)[None], front, ref, dec)[0][0])
            fd = (f[0] - f[1]) / (2 * h)
            # relative to the size of the partials at this candidate (a partial that is 0 up to rounding has no relative error)
            worst = max(worst, abs(part[0, k] - fd) / np.abs(part[0]).max())
    print(f"M={M} P={P}: partials against central differences, relative {worst:.1e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("M", [2, 3, 4])
def test_p0_is_the_product_of_expected_improvements(M):
    ref = REF[:M]
    for mu, sd in [((0.4, 0.5, 0.3, 0.6), (0.25, 0.35, 0.3, 0.2)), ((0.9, 1.0, 1.2, 0.1), (0.5, 0.1, 0.2, 1.0)),
                   ((-0.3, 0.2, 0.0, 0.5), (1.0, 2.0, 0.5, 0.7)), ((0.5, 0.7, 0.2, 0.3), (0.0, 0.3, 0.1, 0.0))]:
        mu, sd = np.array(mu[:M]), np.array(sd[:M])
        val, _ = R.ehvi(mu[None], (sd * sd)[None], None, ref)
        prod = math.prod(E.expected_improvement(mu[k], sd[k], ref[k]) for k in range(M))
        assert abs(val[0] - prod) <= 1e-14 * prod, (mu, sd, val[0], prod)


@pytest.mark.parametrize("M", [3, 4])
def test_permuting_the_objectives_keeps_the_value(M):
    """The objectives permuted together with the front's columns: another sweep order, other boxes, the same quantity within
    1e-13 x max(1, H)."""
    front, ref = _front(7, M)
    rng = np.random.default_rng(8)
    mu = np.vstack([CANDS[:, :M], rng.uniform(-0.2, 1.3, (12, M))])
    var = rng.uniform(0.05, 0.4, mu.shape) ** 2
    v0, p0 = R.ehvi(mu, var, front, ref)
    bar = 1e-13 * max(1.0, _scale(front, ref))
    worst = 0.0
    for perm in itertools.permutations(range(M)):
        perm = list(perm)
        v, p = R.ehvi(mu[:, perm], var[:, perm], front[:, perm], ref[perm])
        worst = max(worst, float(np.abs(v - v0).max()))
        cols = [2 * k + i for k in perm for i in (0, 1)]
        assert np.abs(p - p0[:, cols]).max() <= 10 * bar
    print(f"M={M}: value under permutations of the objectives {worst:.1e} (bar {bar:.1e})")
    assert worst <= bar


def test_front_invariance_bit_for_bit():
    rng = np.random.default_rng(5)
    front = _shell(7, 3)
    ref = REF[:3]
    mu = rng.uniform(-0.2, 1.3, (20, 3))
    var = rng.uniform(0.0, 0.3, (20, 3)) ** 2
    var[3, 0] = 0.0
    v0, p0 = R.ehvi(mu, var, front, ref)
    dominated = front[[1, 4]] + [0.01, 0.02, 0.0]
    outside = np.array([[1.0, 0.1, 0.1], [0.1, 1.2, 0.1], [3.0, -1.0, 0.0], [-1.0, 0.0, 5.0]])  # on the box's edge counts as outside
    for f in (front[rng.permutation(7)], np.vstack([front, dominated]), np.vstack([front[::-1], front[2:5]]),
              np.vstack([outside, front, dominated, front[:1]])[rng.permutation(14)]):
        v, p = R.ehvi(mu, var, f, ref)
        assert v.tobytes() == v0.tobytes() and p.tobytes() == p0.tobytes()
    assert (v0 >= 0).all()


def test_pareto_front_nd_and_hypervolume_nd_on_hand_made_cases():
    pts = np.array([[3.0, 1.0, 2.0], [1.0, 3.0, 2.0], [2.0, 2.0, 2.0], [2.5, 2.5, 2.0], [1.0, 3.0, 2.0], [1.0, 4.0, 1.0], [2.0, 2.0, 3.0]])
    assert E.pareto_front_nd(pts).tolist() == [[1.0, 3.0, 2.0], [1.0, 4.0, 1.0], [2.0, 2.0, 2.0], [3.0, 1.0, 2.0]]
    assert E.pareto_front_nd(np.zeros((0, 3))).shape == (0, 3)
    assert E.pareto_front_nd([[1.0, 1.0, 1.0, 1.0], [2.0, 2.0, 1.0, 2.0]]).tolist() == [[1.0, 1.0, 1.0, 1.0]]
    two = np.array([[3.0, 1.0], [1.0, 3.0], [2.0, 2.0], [2.5, 2.5], [1.0, 3.0]])
    assert E.pareto_front_nd(two).tolist() == E.pareto_front(two).tolist()
    ref = [4.0, 4.0, 4.0]
    assert E.hypervolume_nd(np.zeros((0, 3)), ref) == 0.0
    assert E.hypervolume_nd([[1.0, 1.0, 1.0]], ref) == 27.0
    # two cubes of side 2 and 3 that share the corner ref: (1,1,2) dominates 3 x 3 x 2 = 18, (2,2,1) 2 x 2 x 3 = 12, both 2 x 2 x 2 = 8
    assert E.hypervolume_nd([[1.0, 1.0, 2.0], [2.0, 2.0, 1.0]], ref) == 22.0
    assert E.hypervolume_nd([[1.0, 1.0, 2.0], [2.0, 2.0, 1.0], [3.0, 3.0, 3.0], [5.0, 0.0, 0.0], [0.0, 4.0, 0.0]], ref) == 22.0
    assert E.hypervolume_nd([[1.0, 1.0, 2.0, 3.0]], [4.0, 4.0, 4.0, 4.0]) == 18.0
    assert E.hypervolume_nd([[1.0, 3.0], [2.0, 2.0], [3.0, 1.0]], [4.0, 4.0]) == 6.0
    hv = E.hypervolume_nd(np.array([[[1.0, 1.0, 1.0], [2.0, 2.0, 2.0]], [[3.0, 3.0, 3.0], [2.0, 2.0, 2.0]]]), ref)  # a batch of fronts
    assert hv.tolist() == [27.0, 8.0]
    # the restatement's reduction agrees with pareto_front_nd inside the box
    assert R.reduce_front(pts, [5.0, 5.0, 5.0]).tolist() == E.pareto_front_nd(pts).tolist()
    r = E.default_reference_point_nd([[1.0, 30.0, 5.0], [2.0, 20.0, 5.0], [3.0, 10.0, 5.0]])
    assert np.allclose(r, [3.0 + 0.2, 30.0 + 2.0, 5.5], rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        E.default_reference_point_nd(np.zeros((0, 3)))


def test_acquire_by_ehvi_nd_needs_a_front_without_shared_training_rows():
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
        E.acquire_by_ehvi_nd(X, [Model(X), Model(X), Model(X[:4])], 1)
    with pytest.raises(ValueError, match="two, three or four"):
        E.acquire_by_ehvi_nd(X, [Model(X)], 1, front=[[0.0]], ref=[1.0])
    with pytest.raises(ValueError, match="two, three or four"):
        E.acquire_by_ehvi_nd(X, [Model(X)] * 5, 1, front=[[0.0] * 5], ref=[1.0] * 5)


def test_ehvi_nd_symbols_are_exported_with_the_headers_argument_counts():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "hbegp.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    cap = re.search(r"#define\s+HBEGP_EHVI_ND_MAX_BOXES\s+(\d+)", header)
    assert cap and int(cap.group(1)) == _lib.EHVI_ND_MAX_BOXES
    # the index list of a call, 8 n_obj bytes per box, stays at tens of MiB
    assert 8 * 4 * _lib.EHVI_ND_MAX_BOXES <= 32 << 20


def test_calls_are_refused_before_any_device_call():
    lib = _lib.load()
    x, val = np.zeros((1, 2)), np.zeros(1)
    ref = np.ones(5)
    front = np.full((2, 5), 0.5)
    none = (C.c_void_p * 5)(None, None, None, None, None)
    ip = C.POINTER(C.c_int)
    counts, nb = np.zeros(5, np.int32), C.c_int(0)

    def call(n_obj, fr=front, P=1, rf=ref, m=1, models=none):
        return lib.hbegp_ehvi_nd_f64(models, n_obj, _lib.dptr(x), m, _lib.dptr(fr) if fr is not None else None, P,
                                     _lib.dptr(rf) if rf is not None else None, _lib.dptr(val), None, None, None, None)

    def mcall(n_obj, fr=front, P=1, rf=ref, S=1):
        return lib.hbegp_maximize_ehvi_nd_f64(none, n_obj, _lib.dptr(x), S, None, None, _lib.dptr(fr) if fr is not None else None, P,
                                              _lib.dptr(rf) if rf is not None else None, 10, None, None, None)

    def bcall(n_obj, fr=front, P=1, rf=ref):
        return lib.hbegp_debug_ehvi_boxes(_lib.dptr(fr) if fr is not None else None, P, n_obj, _lib.dptr(rf) if rf is not None else None,
                                          counts.ctypes.data_as(ip), None, 0, C.byref(nb), None, 0)

    def einval(rc, what):
        assert rc == _lib.EINVAL and what in _lib.last_error(), (rc, _lib.last_error())

    for fn in (call, mcall, bcall):
        for n_obj in (1, 5, 0, -2):
            einval(fn(n_obj), "n_obj must be 2, 3 or 4")
        einval(fn(3, rf=None), "ref is NULL")
        einval(fn(3, fr=None), "front is NULL")
        einval(fn(3, P=-1), "P must be >= 0")
        for v in (math.nan, math.inf, -math.inf):
            fr = front.copy()
            fr[0, 2] = v
            einval(fn(3, fr=fr), "non-finite front")
            rf = ref.copy()
            rf[2] = v
            einval(fn(3, rf=rf), "non-finite reference")
    einval(call(3, m=-1), "m must be >= 0")
    einval(mcall(3, S=0), "S must be >= 1")
    einval(call(3), "NULL model")
    einval(call(3, models=None), "models is NULL")
    einval(mcall(4), "NULL model")
    assert bcall(3) == _lib.OK and nb.value == 3 and counts[:3].tolist() == [3, 3, 3]
    assert lib.hbegp_debug_ehvi_nd_phases(0, None) == _lib.OK


def test_a_front_past_the_box_cap_is_enomem_before_any_device_call():
    """The lattice shell i + j = N - 1 of two objectives -- N points (i, N - 1 - i), none dominating another -- splits the free region
    into exactly N + 1 strips.  N = cap - 1 is the last front that is accepted, N = cap the first that is refused: by the host-only
    entry, and by hbegp_ehvi_nd_* before it looks at its (NULL) models -- so before it could reach a device."""
    lib = _lib.load()
    for N in (1, 5, 33):  # the count formula, on both implementations
        f = np.stack([np.arange(N), N - 1.0 - np.arange(N)], axis=1)
        assert len(R.boxes(f, [N, N])[1]) == N + 1 and len(gpr.ehvi_boxes(f, [N, N])[1]) == N + 1
    cap = _lib.EHVI_ND_MAX_BOXES
    ip = C.POINTER(C.c_int)
    counts, nb = np.zeros(2, np.int32), C.c_int(0)
    i = np.arange(cap, dtype=np.float64)
    shell = np.ascontiguousarray(np.stack([i, cap - 1.0 - i], axis=1)[np.random.default_rng(0).permutation(cap)])
    ref = np.array([float(cap), float(cap)])
    rc = lib.hbegp_debug_ehvi_boxes(_lib.dptr(shell), cap - 1, 2, _lib.dptr(ref), counts.ctypes.data_as(ip), None, 0, C.byref(nb), None, 0)
    assert rc == _lib.OK and nb.value == cap and counts.tolist() == [cap + 1, cap + 1]
    rc = lib.hbegp_debug_ehvi_boxes(_lib.dptr(shell), cap, 2, _lib.dptr(ref), counts.ctypes.data_as(ip), None, 0, C.byref(nb), None, 0)
    assert rc == _lib.ENOMEM and "boxes" in _lib.last_error()
    x, val = np.zeros((1, 2)), np.zeros(1)
    none = (C.c_void_p * 2)(None, None)
    rc = lib.hbegp_ehvi_nd_f64(none, 2, _lib.dptr(x), 1, _lib.dptr(shell), cap, _lib.dptr(ref), _lib.dptr(val), None, None, None, None)
    assert rc == _lib.ENOMEM and "boxes" in _lib.last_error()
    rc = lib.hbegp_maximize_ehvi_nd_f64(none, 2, _lib.dptr(x), 1, None, None, _lib.dptr(shell), cap, _lib.dptr(ref), 10, None, None, None)
    assert rc == _lib.ENOMEM and "boxes" in _lib.last_error()
    # the accepted front then fails on its models, not on its size
    rc = lib.hbegp_ehvi_nd_f64(none, 2, _lib.dptr(x), 1, _lib.dptr(shell), cap - 1, _lib.dptr(ref), _lib.dptr(val), None, None, None, None)
    assert rc == _lib.EINVAL and "NULL model" in _lib.last_error()


def test_ehvi_nd_kernels_do_not_spill(isa):  # noqa: F811
    """All twelve instantiations (element type x n_obj x table in the LDS or in global scratch): no spilled register, no scratch."""
    notes = {k: v for k, v in _kernel_notes(isa).items() if "ehvi_nd_kernel" in k}
    assert len(notes) == 12, sorted(notes)
    for sym, note in notes.items():
        assert note["vgpr_spill_count"] == 0 and note["sgpr_spill_count"] == 0 and note["private_segment_fixed_size"] == 0, (sym, note)
        assert note["vgpr_count"] <= 128, (sym, note)  # four waves per SIMD
