"""NumPy float64 restatement of the expected hypervolume improvement of M = 2, 3 or 4 objectives (include/hbegp.h, hbegp_ehvi_nd_*),
shared by the CPU and GPU tests.

All objectives are minimised and independent; objective k has the posterior N(mu_k, var_k) at a candidate.  The front is reduced
to its distinct non-dominated points strictly inside the reference box.  The part of (-inf, r) that no front point weakly
dominates is split into disjoint boxes [l_j, u_j) by a sweep over the objectives: the distinct values of objective 0 cut slabs;
the slab above a value holds the points at or below it, which are projected onto the remaining objectives, reduced, and swept in
turn; with one objective left the free region is (-inf, min).  With G_k(t) = E[(t - Y_k)^+] (ehvi_ref.g_parts) and G_k(-inf) = 0:

    hvi(y) = sum_j prod_k (u_jk - max(y_k, l_jk))^+
    ehvi   = sum_j prod_k [G_k(u_jk) - G_k(l_jk)]
    d/dmu_k = -sum_j [Phi_k(u) - Phi_k(l)] prod_{i != k} dG_i,   d/dsigma_k = sum_j [phi_k(u) - phi_k(l)] prod_{i != k} dG_i

The value takes max(dG, 0) (G is monotone: a negative difference is rounding), the products in the partials the differences as
they are."""
import math

import numpy as np

from ehvi_ref import EPS, argmax_last, g_parts  # noqa: F401  (argmax_last is part of this module's interface)


def _nondominated(pts):
    """The distinct rows of pts [n, M] that no other row is <= in every column, sorted lexicographically."""
    pts = np.asarray(pts, np.float64)
    if len(pts) == 0:
        return pts.reshape(0, pts.shape[1])
    if pts.shape[1] == 1:
        return pts.min(axis=0, keepdims=True)
    pts = np.unique(pts, axis=0)  # sorted lexicographically: only an earlier row can dominate a later one
    keep = np.zeros(len(pts), dtype=bool)
    for i in range(len(pts)):
        keep[i] = not (pts[:i][keep[:i]] <= pts[i]).all(axis=1).any()
    return pts[keep]


def reduce_front(front, ref):
    """[P', M]: the distinct non-dominated points of front [P, M] strictly inside the box below ref, sorted lexicographically."""
    ref = np.asarray(ref, np.float64).reshape(-1)
    f = np.asarray(front if front is not None else [], np.float64).reshape(-1, len(ref))
    return _nondominated(f[(f < ref).all(axis=1)])


def _sweep(pts, ref):
    """The free region below ref of the non-dominated points pts [n, M] as a list of (l [M], u [M]) in value space."""
    M = len(ref)
    if M == 1:
        return [([-math.inf], [min([float(ref[0])] + pts[:, 0].tolist())])]
    edges = [-math.inf] + np.unique(pts[:, 0]).tolist() + [float(ref[0])]
    groups = []  # [lower edge, upper edge, reduced projection]: adjacent slabs with the same projection are one
    for s in range(len(edges) - 1):
        proj = _nondominated(pts[pts[:, 0] <= edges[s]][:, 1:])
        if groups and groups[-1][2].tobytes() == proj.tobytes():
            groups[-1][1] = edges[s + 1]
        else:
            groups.append([edges[s], edges[s + 1], proj])
    out = []
    for lo, hi, proj in groups:
        out += [([lo] + l, [hi] + u) for l, u in _sweep(proj, ref[1:])]
    return out


def boxes(front, ref):
    """(thr, bx): thr a list of M arrays -- -inf, the reduced front's distinct k-th coordinates ascending, r_k -- and bx
    [n_boxes, M, 2] int32, per box and objective the indices (l, u) into thr[k] (0 = -inf)."""
    ref = np.asarray(ref, np.float64).reshape(-1)
    f = reduce_front(front, ref)
    M = len(ref)
    thr = [np.concatenate([[-math.inf], np.unique(f[:, k]), [ref[k]]]) for k in range(M)]
    bx = np.array([[[int(np.searchsorted(thr[k], l[k])), int(np.searchsorted(thr[k], u[k]))] for k in range(M)] for l, u in _sweep(f, ref)],
                  dtype=np.int32).reshape(-1, M, 2)
    return thr, bx


def hvi_boxes(thr, bx, y):
    """sum_j prod_k (u_jk - max(y_k, l_jk))^+ at the points y [N, M]: the hypervolume improvement by the boxes alone."""
    y = np.asarray(y, np.float64)
    M = y.shape[1]
    prod = np.ones((len(y), len(bx)))
    for k in range(M):
        l, u = thr[k][bx[:, k, 0]], thr[k][bx[:, k, 1]]
        prod *= np.maximum(u[None, :] - np.maximum(y[:, k:k + 1], l[None, :]), 0.0)
    return prod.sum(axis=1)


def ehvi(mu, var, front, ref, decomposition=None):
    """(ehvi[m], partials[m, 2 M]) at mu [m, M], var [m, M]: the partials w.r.t. mu_0, sigma_0, mu_1, sigma_1, .. (sigma = sqrt(var);
    the partial w.r.t. a sigma that is 0 is reported as 0).  A NaN in a row's posterior gives NaN in that row.  decomposition:
    (thr, bx) of boxes(front, ref), to share it between calls."""
    ref = np.asarray(ref, np.float64).reshape(-1)
    M = len(ref)
    mu = np.asarray(mu, np.float64).reshape(-1, M)
    var = np.asarray(var, np.float64).reshape(-1, M)
    thr, bx = decomposition if decomposition is not None else boxes(front, ref)
    m, nb = len(mu), len(bx)
    val, part = np.zeros(m), np.zeros((m, 2 * M))
    step = max(1, (1 << 21) // max(nb, 1))  # rows per pass: the [rows, boxes] work arrays stay at 16 MiB each
    for r0 in range(0, m, step):
        rows = slice(r0, min(m, r0 + step))
        sd = np.sqrt(var[rows])
        dg, dc, dp = [], [], []
        for k in range(M):
            g, c, p = g_parts(thr[k][None, :], mu[rows, k:k + 1], sd[:, k:k + 1])
            g[:, 0] = c[:, 0] = p[:, 0] = 0.0  # G(-inf) = Phi = phi = 0
            l, u = bx[:, k, 0], bx[:, k, 1]
            dg.append(g[:, u] - g[:, l])
            dc.append(c[:, l] - c[:, u])
            dp.append(p[:, u] - p[:, l])
        v = np.maximum(dg[0], 0.0)
        for k in range(1, M):
            v = v * np.maximum(dg[k], 0.0)
        val[rows] = v.sum(axis=1)
        for k in range(M):
            others = np.ones_like(dg[0])
            for i in range(M):
                if i != k:
                    others = others * dg[i]
            part[rows, 2 * k] = (dc[k] * others).sum(axis=1)
            part[rows, 2 * k + 1] = np.where(sd[:, k] > EPS, (dp[k] * others).sum(axis=1), 0.0)
    bad = np.isnan(mu).any(axis=1) | np.isnan(var).any(axis=1)
    return np.where(bad, np.nan, val), np.where(bad[:, None], np.nan, part)


def ehvi_grad_x(mu, var, dmu, dvar, front, ref, decomposition=None):
    """(ehvi[m], grad[m, d]) by the chain rule through dmu, dvar [m, M, d]: dsigma = dvar / (2 sigma), 0 where sigma is 0."""
    val, part = ehvi(mu, var, front, ref, decomposition)
    M = part.shape[1] // 2
    sd = np.sqrt(np.asarray(var, np.float64).reshape(-1, M))
    dmu = np.asarray(dmu, np.float64)
    dvar = np.asarray(dvar, np.float64)
    with np.errstate(all="ignore"):
        dsd = np.where((sd > EPS)[:, :, None], dvar / (2.0 * np.where(sd > EPS, sd, 1.0))[:, :, None], 0.0)
    grad = np.zeros(dmu[:, 0].shape)
    for k in range(M):
        grad = grad + part[:, 2 * k, None] * dmu[:, k] + part[:, 2 * k + 1, None] * dsd[:, k]
    return val, grad


def box_scale(amps, front, ref):
    """H = prod_k (r_k - min a_k + sqrt(c_k)): the volume of the box the front spans, widened by one prior standard deviation per
    objective (amps [M]: the models' amplitudes c_k; zeros give the plain box).  min a_k over the reduced front (r_k if empty)."""
    ref = np.asarray(ref, np.float64).reshape(-1)
    f = reduce_front(front, ref)
    lo = f.min(axis=0) if len(f) else ref
    return float(np.prod(ref - lo + np.sqrt(np.asarray(amps, np.float64))))


def bars(dtype, amps, front, ref):
    """The project's plain bars (1e-8 for f64, 1e-4 for f32) times max(1, H): EHVI is a volume, a product of M lengths in y units."""
    return (1e-8 if np.dtype(dtype) == np.float64 else 1e-4) * max(1.0, box_scale(amps, front, ref))
