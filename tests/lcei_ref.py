"""NumPy / scipy float64 restatement of the log-space constrained expected improvement (include/hbegp.h,
hbegp_log_constrained_ei_*), shared by the CPU and GPU tests.  The branches are the kernel's (csrc/kernels.hip: lcei_term).

K = 1 + C independent models: model 0 the minimised objective with the incumbent fmin, models 1 .. C the constraints
g_k <= t_k.  With z_0 = (fmin - mu_0) / sigma_0, z_k = (t_k - mu_k) / sigma_k and h(z) = z Phi(z) + phi(z):

    lei  = log sigma_0 + log h(z_0)   (0 with zero partials for fmin = +inf)
    lF_k = log Phi(z_k),   lpof = lF_1 + .. + lF_C (ascending k),   lcei = lei + lpof

    d lei / d mu_0 = -r / sigma_0,        d lei / d sigma_0 = q / sigma_0,               r = Phi / h, q = phi / h
    d lF_k / d mu_k = -lambda / sigma_k,  d lF_k / d sigma_k = -z_k lambda / sigma_k,    lambda = phi / Phi

z > -1: the direct forms.  z = -a <= -1: the Mills ratio u = sqrt(pi/2) erfcx(a / sqrt 2) = Phi(-a) / phi(a), b = 1 - a u = h / phi;
from a = SERIES_A on, a u and b / x (x = 1 / a^2) from ten terms of their asymptotic series.  sigma = 0 (sigma <= eps):
lei = log((fmin - mu_0)^+) with d / d mu_0 = -1 / (fmin - mu_0) where positive, lF_k = 0 or -inf, every other partial 0."""
import math

import numpy as np
from scipy.special import erfc, erfcx

from ehvi_ref import EPS

SERIES_A = 25.0
BRANCH_POINTS = (-1.0, 0.0, -SERIES_A)  # the z at which lcei_term changes its form
_AU = (1.0, -1.0, 3.0, -15.0, 105.0, -945.0, 10395.0, -135135.0, 2027025.0, -34459425.0)
_BX = (1.0, -3.0, 15.0, -105.0, 945.0, -10395.0, 135135.0, -2027025.0, 34459425.0, -654729075.0)
_HALF_LOG_2PI = 0.91893853320467274
_SQRT_2PI = 2.5066282746310002
_SQRT2 = 1.4142135623730951


def argmax_last(v):
    """The LAST index of the maximum of v; a NaN never wins, -inf wins only where nothing finite exists; -1 without a number."""
    v = np.asarray(v, np.float64)
    ok = np.flatnonzero(~np.isnan(v))
    if not len(ok):
        return -1
    return int(ok[np.flatnonzero(v[ok] == v[ok].max())[-1]])


def _horner(c, x):
    acc = np.full_like(x, c[-1])
    for ck in c[-2::-1]:
        acc = ck + x * acc
    return acc


def scalar_parts(z):
    """(log h, Phi / h, phi / h, log Phi, phi / Phi) at z (any shape), by the kernel's branches."""
    z = np.clip(np.asarray(z, np.float64), -1.7e308, 1.7e308)
    shape = z.shape
    z = z.reshape(-1)
    out = [np.full(z.shape, np.nan) for _ in range(5)]
    with np.errstate(all="ignore"):
        d = z > -1.0
        if d.any():
            zz = z[d]
            az = np.abs(zz)
            cl = 0.5 * erfc(az / _SQRT2)
            pdf = np.exp(-0.5 * az * az) / _SQRT_2PI
            cdf = np.where(zz > 0, 1.0 - cl, cl)
            tail = pdf - az * cl
            h = np.where(zz > 0, zz + tail, tail)
            lam = pdf / cdf
            for o, val in zip(out, (np.log(h), cdf / h, pdf / h, np.where(zz > 0, np.log1p(-cl), np.log(cl)), lam)):
                o[d] = val
        t = ~d & ~np.isnan(z)
        if t.any():
            a = -z[t]
            ser = a >= SERIES_A
            x = np.where(ser, 1.0 / a / a, 1.0)
            au_direct = a * (1.2533141373155003 * erfcx(a / _SQRT2))
            au = np.where(ser, _horner(_AU, x), au_direct)
            bx = np.where(ser, _horner(_BX, x), 1.0 - au_direct)
            base = -0.5 * a * a - _HALF_LOG_2PI
            out[0][t] = base + (np.log(bx) + np.log(x))
            out[1][t] = np.where(ser, a * (au / bx), au / a / bx)
            out[2][t] = np.where(ser, a * (a / bx), 1.0 / bx)
            out[3][t] = base + (np.log(au) - np.log(a))
            out[4][t] = a / au
    return tuple(o.reshape(shape) for o in out)


def parts(mu, var, fmin, limits):
    """(v[m, K], dmu[m, K], dsd[m, K], sd[m, K]): every model's log-term (lei or lF_k) and the term's partials w.r.t. its own mu
    and sigma, which are lcei's.  mu, var [m, K]; limits [C]."""
    mu = np.asarray(mu, np.float64)
    var = np.asarray(var, np.float64)
    m, K = mu.shape
    limits = np.asarray(limits if limits is not None else [], np.float64).reshape(-1)
    assert len(limits) == K - 1
    sd = np.sqrt(var)
    pos = sd > EPS
    s = np.where(pos, sd, 1.0)
    v = np.zeros((m, K))
    dmu = np.zeros((m, K))
    dsd = np.zeros((m, K))
    with np.errstate(all="ignore"):
        if not (math.isinf(fmin) and fmin > 0):
            gap = float(fmin) - mu[:, 0]
            lh, r, q, _, _ = scalar_parts(gap / s[:, 0])
            v[:, 0] = np.where(pos[:, 0], np.log(s[:, 0]) + lh, np.log(np.maximum(gap, 0.0)))
            dmu[:, 0] = np.where(pos[:, 0], -r / s[:, 0], np.where(gap > 0, -1.0 / np.where(gap > 0, gap, 1.0), 0.0))
            dsd[:, 0] = np.where(pos[:, 0], q / s[:, 0], 0.0)
        if K > 1:
            gap = limits[None, :] - mu[:, 1:]
            z = np.clip(gap / s[:, 1:], -1.7e308, 1.7e308)
            _, _, _, lphi, lam = scalar_parts(z)
            zl = np.where((z > -1.0) & (lam == 0.0), 0.0, z * lam)  # (an underflowed phi times a huge z is 0)
            v[:, 1:] = np.where(pos[:, 1:], lphi, np.where(gap > 0, 0.0, -np.inf))
            dmu[:, 1:] = np.where(pos[:, 1:], -lam / s[:, 1:], 0.0)
            dsd[:, 1:] = np.where(pos[:, 1:], -zl / s[:, 1:], 0.0)
    return v, dmu, dsd, sd


def lcei(mu, var, fmin, limits):
    """(lcei[m], lei[m], lpof[m], dlcei_dmu[m, K], dlcei_dsd[m, K]).  A NaN in a row's posteriors gives NaN in that row."""
    mu = np.asarray(mu, np.float64)
    var = np.asarray(var, np.float64)
    v, dmu, dsd, _ = parts(mu, var, fmin, limits)
    m, K = v.shape
    lpof = np.zeros(m)
    for k in range(1, K):
        lpof = lpof + v[:, k]
    lei = v[:, 0].copy()
    bad = np.isnan(mu).any(axis=1) | np.isnan(var).any(axis=1)
    nan = np.where(bad, np.nan, 0.0)
    return lei + lpof + nan, lei + nan, lpof + nan, dmu + nan[:, None], dsd + nan[:, None]


def lcei_grad_x(mu, var, dmean, dvar, fmin, limits):
    """(lcei[m], lei[m], lpof[m], grad[m, d], scale[m]) by the chain rule through dmean, dvar [m, K, d]: dsigma = dvar / (2 sigma),
    0 where sigma is 0.  scale = max over the features of sum_k (|d lcei / d mu_k| |dmean_k| + |d lcei / d sigma_k| |dsigma_k|):
    the rounding scale of the sum the gradient is."""
    val, lei, lpof, pm, ps = lcei(mu, var, fmin, limits)
    sd = np.sqrt(np.asarray(var, np.float64))
    dmean = np.asarray(dmean, np.float64)
    dvar = np.asarray(dvar, np.float64)
    with np.errstate(all="ignore"):
        dsd = np.where((sd > EPS)[:, :, None], dvar / (2.0 * np.where(sd > EPS, sd, 1.0))[:, :, None], 0.0)
        grad = np.zeros(dmean.shape[::2])
        scale = np.zeros(dmean.shape[::2])
        for k in range(dmean.shape[1]):
            grad = grad + (pm[:, k, None] * dmean[:, k] + ps[:, k, None] * dsd[:, k])
            scale = scale + (np.abs(pm[:, k, None] * dmean[:, k]) + np.abs(ps[:, k, None] * dsd[:, k]))
    return val, lei, lpof, grad, (scale.max(axis=1) if scale.shape[1] else np.zeros(len(scale)))


def value_bar(dtype, ref):
    """The project's standing bar: 1e-8 (f64) / 1e-4 (f32) times max(1, |reference value|), per entry of `ref` (a -inf or NaN
    reference has to be met exactly: its bar is 0)."""
    base = 1e-8 if np.dtype(dtype) == np.float64 else 1e-4
    ref = np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(ref), base * np.maximum(1.0, np.abs(ref)), 0.0)


def grad_bar(dtype, ref, scale):
    """Per row: 1e-8 (f64) / 1e-4 (f32) times max(1, |the row's reference lcei|) (1 where that is not finite) times max(1, the
    rounding scale of the row's gradient sum that lcei_grad_x computed), as cei_ref.grad_bar."""
    base = 1e-8 if np.dtype(dtype) == np.float64 else 1e-4
    ref = np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        size = np.where(np.isfinite(ref), np.maximum(1.0, np.abs(ref)), 1.0)
    return base * size * np.maximum(1.0, np.nan_to_num(np.asarray(scale, np.float64), nan=1.0, posinf=1.0))
