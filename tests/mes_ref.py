"""NumPy / scipy float64 restatement of max-value entropy search (include/hbegp.h, hbegp_mes_*), shared by the CPU and GPU
tests.  The branches are the kernel's (csrc/kernels.hip: mes_term).

One minimised model with posterior N(mu, sigma^2) at a candidate and S sampled minimum values y*_s:

    gamma_s = (mu - y*_s) / sigma   (clamped to +-1.7e308),     lambda = phi / Phi
    t(g)  = g lambda(g) / 2 - log Phi(g),      t'(g) = -(lambda / 2) (1 + g^2 + g lambda)
    mes   = (1/S) sum_s t(gamma_s),   d mes / d mu = (1/S) sum t' / sigma,   d mes / d sigma = -(1/S) sum gamma t' / sigma

g > -1: the direct forms.  g = -a <= -1: au = a sqrt(pi/2) erfcx(a / sqrt 2), b = 1 - au, w = a^2 b / au,
t = -w / 2 + log sqrt(2 pi) + (log a - log au), t' = -(a / au) (1 - w) / 2; from a = SERIES_A on au, bx = b / x and (au - bx) / x
(x = 1 / a^2) from ten-term asymptotic series, w = bx / au and 1 - w = x ((au - bx) / x) / au.  sigma = 0 (sigma <= eps): mes = 0
and every partial is 0."""
import numpy as np
from scipy.special import erfc, erfcx

from ehvi_ref import EPS
from lcei_ref import _AU, _BX, _HALF_LOG_2PI, _SQRT2, _SQRT_2PI, SERIES_A, _horner, argmax_last  # noqa: F401 (argmax_last: re-exported)

BRANCH_POINTS = (-1.0, 0.0, -SERIES_A)  # the g at which mes_term changes its form
_DQ = tuple(a - b for a, b in zip(_AU[1:], _BX[1:]))  # (au - bx) / x: the constant terms cancel exactly; 2, -12, 90, ..


def scalar_parts(g):
    """(t, t') at g (any shape), by the kernel's branches."""
    g = np.clip(np.asarray(g, np.float64), -1.7e308, 1.7e308)
    shape = g.shape
    g = g.reshape(-1)
    t = np.full(g.shape, np.nan)
    dt = np.full(g.shape, np.nan)
    with np.errstate(all="ignore"):
        d = g > -1.0
        if d.any():
            gg = g[d]
            az = np.abs(gg)
            cl = 0.5 * erfc(az / _SQRT2)
            pdf = np.exp(-0.5 * az * az) / _SQRT_2PI
            cdf = np.where(gg > 0, 1.0 - cl, cl)
            lam = pdf / cdf
            lphi = np.where(gg > 0, np.log1p(-cl), np.log(cl))
            gl = np.where(pdf > 0, gg * lam, 0.0)
            t[d] = 0.5 * gl - lphi
            dt[d] = np.where(pdf > 0, -0.5 * lam * (1.0 + gg * gg + gl), 0.0)
        n = ~d & ~np.isnan(g)
        if n.any():
            a = -g[n]
            ser = a >= SERIES_A
            x = np.where(ser, 1.0 / a / a, 1.0)
            au_direct = a * (1.2533141373155003 * erfcx(a / _SQRT2))
            au = np.where(ser, _horner(_AU, x), au_direct)
            w_direct = a * a * (1.0 - au_direct) / au_direct
            w = np.where(ser, _horner(_BX, x) / au, w_direct)
            one_minus_w = np.where(ser, x * _horner(_DQ, x) / au, 1.0 - w_direct)
            t[n] = -0.5 * w + _HALF_LOG_2PI + (np.log(a) - np.log(au))
            dt[n] = -(a / au) * one_minus_w / 2.0
    return t.reshape(shape), dt.reshape(shape)


def parts(mu, var, ystar):
    """(mes[m], dmes_dmu[m], dmes_dsd[m]) for mu, var [m] and ystar [S]; the S terms are added in float64 by np.sum (pairwise: the
    device's order differs, which the bars cover).  A NaN in a row's posterior gives NaN in that row."""
    mu = np.asarray(mu, np.float64).reshape(-1)
    var = np.asarray(var, np.float64).reshape(-1)
    ys = np.asarray(ystar, np.float64).reshape(-1)
    sd = np.sqrt(var)
    pos = sd > EPS
    s = np.where(pos, sd, 1.0)
    with np.errstate(all="ignore"):
        g = np.clip((mu[:, None] - ys[None, :]) / s[:, None], -1.7e308, 1.7e308)
        t, dt = scalar_parts(g)
        val = np.where(pos, t.sum(axis=1) / len(ys), 0.0)
        dmu = np.where(pos, dt.sum(axis=1) / len(ys) / s, 0.0)
        dsd = np.where(pos, -(g * dt).sum(axis=1) / len(ys) / s, 0.0)
    nan = np.where(np.isnan(mu) | np.isnan(var), np.nan, 0.0)
    return val + nan, dmu + nan, dsd + nan


def mes(mu, var, ystar):
    """mes[m]."""
    return parts(mu, var, ystar)[0]


def mes_grad_x(mu, var, dmean, dvar, ystar):
    """(mes[m], grad[m, d], scale[m]) by the chain rule through dmean, dvar [m, d]: dsigma = dvar / (2 sigma), 0 where sigma is 0.
    scale = max over the features of |d mes / d mu| |dmean| + |d mes / d sigma| |dsigma|: the rounding scale of the sum the
    gradient is."""
    val, pm, ps = parts(mu, var, ystar)
    sd = np.sqrt(np.asarray(var, np.float64).reshape(-1))
    dmean = np.asarray(dmean, np.float64)
    dvar = np.asarray(dvar, np.float64)
    with np.errstate(all="ignore"):
        dsd = np.where((sd > EPS)[:, None], dvar / (2.0 * np.where(sd > EPS, sd, 1.0))[:, None], 0.0)
        grad = pm[:, None] * dmean + ps[:, None] * dsd
        scale = np.abs(pm[:, None] * dmean) + np.abs(ps[:, None] * dsd)
    return val, grad, (scale.max(axis=1) if scale.shape[1] else np.zeros(len(scale)))


def value_bar(dtype, ref):
    """The project's standing bar: 1e-8 (f64) / 1e-4 (f32) times max(1, |reference value|), per entry of `ref` (a NaN reference
    has to be met exactly: its bar is 0)."""
    base = 1e-8 if np.dtype(dtype) == np.float64 else 1e-4
    ref = np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(ref), base * np.maximum(1.0, np.abs(ref)), 0.0)


def grad_bar(dtype, ref, scale):
    """Per row: 1e-8 (f64) / 1e-4 (f32) times max(1, |the row's reference mes|) (1 where that is not finite) times max(1, the
    rounding scale of the row's gradient sum that mes_grad_x computed)."""
    base = 1e-8 if np.dtype(dtype) == np.float64 else 1e-4
    ref = np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        size = np.where(np.isfinite(ref), np.maximum(1.0, np.abs(ref)), 1.0)
    return base * size * np.maximum(1.0, np.nan_to_num(np.asarray(scale, np.float64), nan=1.0, posinf=1.0))
