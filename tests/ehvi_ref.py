"""NumPy float64 restatement of the two-objective expected hypervolume improvement (include/hbegp.h, hbegp_ehvi_*), shared by the
CPU and GPU tests.

Both objectives are minimised and independent; objective k has the posterior N(mu_k, var_k) at a candidate.  The front is reduced
to its non-dominated points strictly inside the reference box, a ascending (b descends); with a_0 = -inf, a_{P+1} = r1, b_0 = r2,
G_k(t) = E[(t - Y_k)^+] = sigma_k h((t - mu_k) / sigma_k) and h(z) = z Phi(z) + phi(z):

    ehvi = sum_{i=0..P} [G_1(a_{i+1}) - G_1(a_i)] G_2(b_i)

(strip i spans objective 0 from a_i to a_{i+1}; a draw (y1, y2) with y1 in it adds the area below b_i to the right of y1 up to
the strip's end, and all of the later strips' areas below their own b).  dG/dmu = -Phi(z), dG/dsigma = phi(z)."""
import math

import numpy as np
from scipy.special import erfc

EPS = float(np.finfo(np.float64).eps)


def reduce_front(front, ref):
    """(a[P'], b[P']): the non-dominated points of front [P, 2] strictly inside the box below ref, a ascending, b descending."""
    f = np.asarray(front if front is not None else [], np.float64).reshape(-1, 2)
    f = f[(f[:, 0] < ref[0]) & (f[:, 1] < ref[1])]
    f = f[np.lexsort((f[:, 1], f[:, 0]))]
    a, b, bmin = [], [], float(ref[1])
    for x, y in f.tolist():
        if y < bmin:
            a.append(x), b.append(y)
            bmin = y
    return np.array(a, np.float64), np.array(b, np.float64)


def thresholds(front, ref):
    """(up[ns], hb[ns]), ns = P' + 1: strip i ends at up[i] along objective 0 (the last at r1) below the height hb[i] (hb[0] = r2)."""
    a, b = reduce_front(front, ref)
    return np.concatenate([a, [float(ref[0])]]), np.concatenate([[float(ref[1])], b])


def g_parts(t, mu, sd):
    """(G, Phi, phi) of G(t) = E[(t - Y)^+], Y ~ N(mu, sd^2), elementwise (broadcast).  h(z) for z <= 0 as phi(a) - a Phi(-a),
    a = |z| (no cancellation against z), and z + h(-z) above; sd = 0 (|sd| <= eps): (t - mu)^+, [t > mu], 0."""
    t, mu, sd = np.broadcast_arrays(np.asarray(t, np.float64), np.asarray(mu, np.float64), np.asarray(sd, np.float64))
    pos = sd > EPS
    with np.errstate(all="ignore"):
        z = np.where(pos, (t - mu) / np.where(pos, sd, 1.0), 0.0)
        az = np.minimum(np.abs(z), 38.0)
        near = np.abs(z) < 38.0
        cl = np.where(near, 0.5 * erfc(az / math.sqrt(2.0)), 0.0)
        pdf = np.where(near, np.exp(-0.5 * az * az) / math.sqrt(2.0 * math.pi), 0.0)
        tail = np.maximum(pdf - az * cl, 0.0)
        g = sd * np.where(z > 0, z + tail, tail)
        cdf = np.where(z > 0, 1.0 - cl, cl)
    g = np.where(pos, g, np.maximum(t - mu, 0.0))
    cdf = np.where(pos, cdf, (t > mu).astype(np.float64))
    pdf = np.where(pos, pdf, 0.0)
    return g, cdf, pdf


def ehvi(mu, var, front, ref):
    """(ehvi[m], partials[m, 4]) at mu [m, 2], var [m, 2]: the partials w.r.t. mu_1, sigma_1, mu_2, sigma_2 (sigma = sqrt(var); the
    partial w.r.t. a sigma that is 0 is reported as 0).  A NaN in a row's posterior gives NaN in that row."""
    mu = np.asarray(mu, np.float64).reshape(-1, 2)
    var = np.asarray(var, np.float64).reshape(-1, 2)
    up, hb = thresholds(front, ref)
    sd = np.sqrt(var)
    gu, cu, pu = g_parts(up[None, :], mu[:, :1], sd[:, :1])
    gh, ch, ph = g_parts(hb[None, :], mu[:, 1:], sd[:, 1:])
    z = np.zeros((len(mu), 1))
    gl, cl, pl = (np.concatenate([z, x[:, :-1]], axis=1) for x in (gu, cu, pu))  # G_1(-inf) = Phi = phi = 0
    dg = gu - gl
    val = (np.maximum(dg, 0.0) * gh).sum(axis=1)
    part = np.stack([((cl - cu) * gh).sum(axis=1), ((pu - pl) * gh).sum(axis=1), -(dg * ch).sum(axis=1), (dg * ph).sum(axis=1)], axis=1)
    part[:, 1] = np.where(sd[:, 0] > EPS, part[:, 1], 0.0)
    part[:, 3] = np.where(sd[:, 1] > EPS, part[:, 3], 0.0)
    bad = np.isnan(mu).any(axis=1) | np.isnan(var).any(axis=1)
    val = np.where(bad, np.nan, val)
    part = np.where(bad[:, None], np.nan, part)
    return val, part


def ehvi_grad_x(mu, var, dmu, dvar, front, ref):
    """(ehvi[m], grad[m, d]) by the chain rule through dmu, dvar [m, 2, d]: dsigma = dvar / (2 sigma), 0 where sigma is 0."""
    val, part = ehvi(mu, var, front, ref)
    sd = np.sqrt(np.asarray(var, np.float64).reshape(-1, 2))
    dmu = np.asarray(dmu, np.float64)
    dvar = np.asarray(dvar, np.float64)
    with np.errstate(all="ignore"):
        dsd = np.where((sd > EPS)[:, :, None], dvar / (2.0 * np.where(sd > EPS, sd, 1.0))[:, :, None], 0.0)
    grad = part[:, 0, None] * dmu[:, 0] + part[:, 1, None] * dsd[:, 0] + part[:, 2, None] * dmu[:, 1] + part[:, 3, None] * dsd[:, 1]
    return val, grad


def argmax_last(v):
    return len(v) - 1 - int(np.argmax(np.asarray(v)[::-1]))


def box_scale(c1, c2, front, ref):
    """H = (r1 - min a + sqrt(c1)) (r2 - min b + sqrt(c2)): the area of the box the front spans, widened by one prior standard
    deviation per objective -- the scale of a hypervolume improvement.  min a, min b over the reduced front (r1, r2 if empty)."""
    a, b = reduce_front(front, ref)
    amin = a.min() if len(a) else float(ref[0])
    bmin = b.min() if len(b) else float(ref[1])
    return (float(ref[0]) - amin + math.sqrt(c1)) * (float(ref[1]) - bmin + math.sqrt(c2))


def bars(dtype, c1, c2, front, ref):
    """The project's plain bars (1e-8 for f64, 1e-4 for f32) times max(1, H): EHVI is an area, a product of two lengths in y units."""
    return (1e-8 if np.dtype(dtype) == np.float64 else 1e-4) * max(1.0, box_scale(c1, c2, front, ref))
