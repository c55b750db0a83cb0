"""NumPy float64 restatement of the constrained expected improvement (include/hbegp.h, hbegp_constrained_ei_*), shared by the CPU
and GPU tests.

K = 1 + C independent models: model 0 the minimised objective with the incumbent fmin, models 1 .. C the constraints
g_k <= t_k.  With the posterior N(mu_k, var_k) of model k at a candidate, sigma = sqrt(var), h(z) = z Phi(z) + phi(z):

    ei  = sigma_0 h((fmin - mu_0) / sigma_0)      (1 for fmin = +inf: no feasible incumbent)
    F_k = Phi((t_k - mu_k) / sigma_k)
    cei = ei * pof,   pof = F_1 F_2 .. F_C        (ascending k)

    d ei / d mu_0 = -Phi(z_0),            d ei / d sigma_0 = phi(z_0)
    d F_k / d mu_k = -phi(z_k) / sigma_k, d F_k / d sigma_k = -z_k phi(z_k) / sigma_k
    d cei / d(.)_0 = pof d ei / d(.)_0,   d cei / d(.)_k = ei W_k d F_k / d(.)_k,  W_k = prod_{j != k} F_j

W_k from a prefix and a suffix product: no division by F_k.  sigma = 0 (sigma <= eps): ei = (fmin - mu_0)^+, F_k = [t_k > mu_k],
the partial w.r.t. that sigma is 0 and so are both partials of F_k."""
import math

import numpy as np

from ehvi_ref import EPS, argmax_last, g_parts  # noqa: F401  (argmax_last is part of this module's interface)


def parts(mu, var, fmin, limits):
    """(f[m, K], dmu[m, K], dsd[m, K], sd[m, K]): every model's factor (ei or F_k) and the factor's partials w.r.t. its own mu and
    sigma.  mu, var [m, K]; limits [C]."""
    mu = np.asarray(mu, np.float64)
    var = np.asarray(var, np.float64)
    m, K = mu.shape
    limits = np.asarray(limits if limits is not None else [], np.float64).reshape(-1)
    assert len(limits) == K - 1
    sd = np.sqrt(var)
    pos = sd > EPS
    f = np.ones((m, K))
    dmu = np.zeros((m, K))
    dsd = np.zeros((m, K))
    if not (math.isinf(fmin) and fmin > 0):
        g, cdf, pdf = g_parts(float(fmin), mu[:, 0], sd[:, 0])
        f[:, 0], dmu[:, 0], dsd[:, 0] = g, -cdf, pdf  # pdf is 0 where sigma is 0
    if K > 1:
        _, cdf, pdf = g_parts(limits[None, :], mu[:, 1:], sd[:, 1:])
        s = np.where(pos[:, 1:], sd[:, 1:], 1.0)
        with np.errstate(all="ignore"):
            z = (limits[None, :] - mu[:, 1:]) / s
            f[:, 1:] = cdf
            dmu[:, 1:] = np.where(pos[:, 1:], -pdf / s, 0.0)
            dsd[:, 1:] = np.where(pos[:, 1:], -z * pdf / s, 0.0)
    return f, dmu, dsd, sd


def cei(mu, var, fmin, limits):
    """(cei[m], ei[m], pof[m], dcei_dmu[m, K], dcei_dsd[m, K]).  A NaN in a row's posteriors gives NaN in that row."""
    mu = np.asarray(mu, np.float64)
    var = np.asarray(var, np.float64)
    f, dmu, dsd, _ = parts(mu, var, fmin, limits)
    m, K = f.shape
    pre = np.ones((m, K))  # pre[:, k] = F_1 .. F_{k-1}, suf[:, k] = F_{k+1} .. F_C (built from the end)
    suf = np.ones((m, K))
    for k in range(2, K):
        pre[:, k] = pre[:, k - 1] * f[:, k - 1]
    for k in range(K - 2, 0, -1):
        suf[:, k] = suf[:, k + 1] * f[:, k + 1]
    pof = np.ones(m)
    for k in range(1, K):
        pof = pof * f[:, k]
    ei = f[:, 0].copy()
    w = ei[:, None] * (pre * suf)
    w[:, 0] = pof
    val = ei * pof
    pm, ps = w * dmu, w * dsd
    bad = np.isnan(mu).any(axis=1) | np.isnan(var).any(axis=1)
    nan = np.where(bad, np.nan, 0.0)
    return val + nan, ei + nan, pof + nan, pm + nan[:, None], ps + nan[:, None]


def cei_grad_x(mu, var, dmean, dvar, fmin, limits):
    """(cei[m], ei[m], pof[m], grad[m, d], scale[m]) by the chain rule through dmean, dvar [m, K, d]: dsigma = dvar / (2 sigma), 0
    where sigma is 0.  scale = max over the features of sum_k (|d cei / d mu_k| |dmean_k| + |d cei / d sigma_k| |dsigma_k|): the
    rounding scale of the sum the gradient is."""
    val, ei, pof, pm, ps = cei(mu, var, fmin, limits)
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
    return val, ei, pof, grad, (scale.max(axis=1) if scale.shape[1] else np.zeros(len(scale)))


def value_bar(dtype, mu0, var0, fmin):
    """The project's standing bar: 1e-8 (f64) / 1e-4 (f32) times max(1, max_j(|fmin - mu_0j| + sigma_0j)) -- the size of an
    expected improvement; times 1 for fmin = +inf, where cei is a probability."""
    base = 1e-8 if np.dtype(dtype) == np.float64 else 1e-4
    if math.isinf(fmin):
        return base
    mu0 = np.asarray(mu0, np.float64)
    sd0 = np.sqrt(np.asarray(var0, np.float64))
    return base * max(1.0, float(np.nanmax(np.abs(fmin - mu0) + sd0)))


def grad_bar(dtype, mu0, var0, fmin, scale):
    """value_bar times max(1, the largest rounding scale of the gradient's sum that cei_grad_x computed)."""
    return value_bar(dtype, mu0, var0, fmin) * max(1.0, float(np.nanmax(scale)) if len(scale) else 1.0)
