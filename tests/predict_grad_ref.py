"""NumPy restatement of the posterior gradient (include/hbegp.h, hbegp_predict_grad_*), shared by the CPU and GPU tests.

k(x*, x_j) = c phi_nu(r), psi = phi'(r) / r, dk_j/dx*_k = c psi(r) (x*_k - x_jk) / ell_k^2 (0 at r = 0),
dmean = sum_j dk_j alpha_j, dvar = -2 sum_j dk_j v_j with v = K^-1 k*, evaluated as -2 (L^-1 dk) . (L^-1 k*) (the library's
form: both factors are bounded) or through an explicit K^-1 (dvar_ref_kinv)."""
import math

import numpy as np

from oracle import gpr_oracle as O


def psi(r, nu):
    with np.errstate(divide="ignore", invalid="ignore"):
        if math.isinf(nu):
            out = -np.exp(-0.5 * r * r)
        elif nu == 0.5:
            out = -np.exp(-r) / r
        elif nu == 1.5:
            out = -3.0 * np.exp(-math.sqrt(3.0) * r)
        elif nu == 2.5:
            out = -(5.0 / 3.0) * (1.0 + math.sqrt(5.0) * r) * np.exp(-math.sqrt(5.0) * r)
        else:
            raise ValueError(nu)
    return np.where(r == 0.0, 0.0, out)


def _dk(Xs, X, amplitude, length_scale, nu):
    """dk(x*_i, x_j) / dx*_i,k as [m, n, d] in float64."""
    ell = np.asarray(length_scale, dtype=np.float64)
    diff = (np.asarray(Xs, np.float64) / ell)[:, None, :] - (np.asarray(X, np.float64) / ell)[None, :, :]
    r = np.sqrt((diff * diff).sum(axis=2))
    return (amplitude * psi(r, nu))[:, :, None] * diff / ell


def dmean_ref(Xs, X, alpha, amplitude, length_scale, nu):
    return np.einsum("mnd,n->md", _dk(Xs, X, amplitude, length_scale, nu), np.asarray(alpha, dtype=np.float64))


def dvar_ref(Xs, X, amplitude, length_scale, nu, noise, var=None):
    """-2 (L^-1 dk/dx*_k) . (L^-1 k*) with the host's own Cholesky factor of K (the form the library uses)."""
    from scipy.linalg import solve_triangular

    X64, Xs64 = np.asarray(X, np.float64), np.asarray(Xs, np.float64)
    K = O.product_kernel(X64, X64, amplitude, np.asarray(length_scale, np.float64), nu)
    K[np.diag_indices(len(X64))] += noise
    L = np.linalg.cholesky(K)
    ks = O.product_kernel(Xs64, X64, amplitude, np.asarray(length_scale, np.float64), nu)
    q = solve_triangular(L, ks.T, lower=True)  # [n, m]
    dk = _dk(Xs64, X64, amplitude, length_scale, nu)  # [m, n, d]
    m, n, d = dk.shape
    w = solve_triangular(L, dk.transpose(1, 0, 2).reshape(n, m * d), lower=True).reshape(n, m, d)
    dvar = -2.0 * np.einsum("nmd,nm->md", w, q)
    if var is not None:
        dvar[np.asarray(var) == 0] = 0.0
    return dvar


def dvar_ref_kinv(Xs, X, kinv, amplitude, length_scale, nu, var=None):
    """-2 sum_j dk_j v_j with V = Kstar K^-1 from a given K^-1 (the explicit form; loses digits as cond(K) grows)."""
    X64, Xs64 = np.asarray(X, np.float64), np.asarray(Xs, np.float64)
    V = O.product_kernel(Xs64, X64, amplitude, np.asarray(length_scale, np.float64), nu) @ np.asarray(kinv, dtype=np.float64)
    dvar = -2.0 * np.einsum("mnd,mn->md", _dk(Xs64, X64, amplitude, length_scale, nu), V)
    if var is not None:
        dvar[np.asarray(var) == 0] = 0.0
    return dvar


def row_dev(got, ref):
    """max over rows of |got - ref| / max|ref row| (rows whose reference is all zero: absolute)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max(axis=1)
    scale = np.where(scale > 0, scale, 1.0)
    return float((np.abs(got - ref).max(axis=1) / scale).max())
