"""NumPy restatement of the joint posterior (include/hbegp.h, hbegp_predict_cov_* / hbegp_sample_posterior_*), shared by the CPU
and GPU tests.

Sigma = K** + (1e-5 + jitter) I - K*^T K^-1 K*, evaluated as K** + (1e-5 + jitter) I - Q^T Q with Q = L^-1 K*^T (the library's
form) or through an explicit K^-1 (sigma_ref_kinv, the reference's own form for the variance, predict.rs:30-37).  Draws:
mean + L_S z with L_S = cholesky(Sigma)."""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import gpr_oracle as O


def _k(A, B, amplitude, length_scale, nu):
    return O.product_kernel(np.asarray(A, np.float64), np.asarray(B, np.float64), amplitude, np.asarray(length_scale, np.float64), nu)


def kernel_matrix(X, amplitude, length_scale, nu, noise):
    K = _k(X, X, amplitude, length_scale, nu)
    K[np.diag_indices(len(K))] += noise
    return K


def sigma_ref(Xs, X, amplitude, length_scale, nu, noise, jitter=0.0):
    """[m, m] in float64 through the host's Cholesky factor of K."""
    L = np.linalg.cholesky(kernel_matrix(X, amplitude, length_scale, nu, noise))
    Q = solve_triangular(L, _k(Xs, X, amplitude, length_scale, nu).T, lower=True)
    S = _k(Xs, Xs, amplitude, length_scale, nu) - Q.T @ Q
    S[np.diag_indices(len(S))] += O.MIN_NOISE + jitter
    return S


def sigma_ref_kinv(Xs, X, kinv, amplitude, length_scale, nu, jitter=0.0):
    """The same through an explicit K^-1: K** + 1e-5 I - K* K^-1 K*^T."""
    Ks = _k(Xs, X, amplitude, length_scale, nu)
    S = _k(Xs, Xs, amplitude, length_scale, nu) - Ks @ np.asarray(kinv, np.float64) @ Ks.T
    S[np.diag_indices(len(S))] += O.MIN_NOISE + jitter
    return S


def draws_ref(mean, sigma, z):
    """mean + L_S z_s for every row s of z, L_S = cholesky(sigma), in float64."""
    L = np.linalg.cholesky(np.asarray(sigma, np.float64))
    return np.asarray(mean, np.float64)[None, :] + np.asarray(z, np.float64) @ L.T
