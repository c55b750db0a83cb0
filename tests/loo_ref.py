"""NumPy fp64 restatement of leave-one-out cross-validation in closed form (hbegp_model_loo_*, hbegp_problem_eval_loo;
Rasmussen & Williams 5.4.2), on the kernel matrices of oracle.gpr_oracle.

In the model's normalised y space, with K = c Matern(X, X) + s2 I, M = K^-1, alpha = M y, m_i = M_ii:

    mu_i = y_i - alpha_i / m_i,   var_i = 1 / m_i (the observation's: it includes s2),
    lpd_i = 1/2 ln m_i - alpha_i^2 / (2 m_i) - 1/2 ln 2 pi,   loo = sum_i lpd_i

m_i is formed twice: as the column sum of squares of L^-1 (what the device does) and as the diagonal of L^-T L^-1.
The gradient in the order [ln s2, ln c, ln ell_k] is formed twice as well: by the book (R&W eq. 5.13, one n^3 product per
parameter) and through the identity the device uses (one n^3 product for all parameters)."""
import math

import numpy as np
from scipy.linalg import solve_triangular

from oracle import gpr_oracle as O


def kernel_and_grads(X, noise, amp, ell, nu):
    """K [n, n] and dK/dtheta_j [n, n, p] in fp64, theta = [ln s2, ln c, ln ell_k] (lml.rs:40-44, product_kernel.rs:40-70)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    K, g = O.product_theta_grad(X, float(amp), np.asarray(ell, dtype=np.float64), nu)
    K = K + float(noise) * np.eye(n)
    dK = np.concatenate([(float(noise) * np.eye(n))[:, :, None], g], axis=2)
    return K, dK


def loo(X, y, noise, amp, ell, nu, want_grad=True, by_the_book=False):
    """dict(mean, var, lpd, loo, m, m_kinv[, grad[, grad_book]]); m from L^-1, m_kinv = diag(L^-T L^-1)."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    if want_grad:
        K, dK = kernel_and_grads(X, noise, amp, ell, nu)
    else:
        K = O.product_kernel(np.asarray(X, dtype=np.float64), np.asarray(X, dtype=np.float64), float(amp),
                             np.asarray(ell, dtype=np.float64), nu) + float(noise) * np.eye(n)
    L = np.linalg.cholesky(K)
    Linv = solve_triangular(L, np.eye(n), lower=True)
    M = Linv.T @ Linv
    alpha = Linv.T @ (Linv @ y)
    m = (Linv * Linv).sum(axis=0)
    out = dict(mean=y - alpha / m, var=1.0 / m, lpd=0.5 * np.log(m) - alpha * alpha / (2.0 * m) - 0.5 * math.log(2.0 * math.pi),
               m=m, m_kinv=np.diag(M).copy(), alpha=alpha)
    out["loo"] = float(out["lpd"].sum())
    if not want_grad:
        return out
    a = alpha / m
    b = 0.5 * (1.0 + alpha * alpha / m) / m
    u = M @ a
    Cm = (M * b[None, :]) @ M
    W = np.outer(u, alpha) + np.outer(alpha, u) - 2.0 * Cm
    out["grad"] = np.array([0.5 * float((W * dK[:, :, j]).sum()) for j in range(dK.shape[2])])
    if by_the_book:  # R&W eq. 5.13 with Z_j = M dK_j
        g = []
        for j in range(dK.shape[2]):
            Z = M @ dK[:, :, j]
            g.append(float(((alpha * (Z @ alpha) - 0.5 * (1.0 + alpha * alpha / m) * np.einsum("ik,ki->i", Z, M)) / m).sum()))
        out["grad_book"] = np.array(g)
    return out


def loo_at_theta(X, y, theta, nu, lo=None, hi=None, **kw):
    """loo at a log-space theta with the engine's clamping (fit.rs:94-96): kernel parameters clamped into [lo, hi], the noise not."""
    v = np.exp(np.asarray(theta, dtype=np.float64))
    if lo is not None:
        v[1:] = np.minimum(np.maximum(v[1:], np.asarray(lo)[1:]), np.asarray(hi)[1:])
    return loo(X, y, v[0], v[1], v[2:], nu, **kw)
