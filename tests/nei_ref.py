"""NumPy restatement of noisy expected improvement over a candidate set (include/hbegp.h, hbegp_noisy_ei_*), shared by the CPU and
GPU tests.

From the posterior mean mu and Sigma of the baseline rows (the first mb) followed by the candidates, as predict_cov returns them
at the call's jitter, and the caller's normals z [S, mb]:
    L_b = chol(Sigma_bb),  A = Sigma_cb L_b^-T,  rho_j = max(Sigma_jj - sum_k A_jk^2, 0)
    draw s:  f_s = mu_b + L_b z_s,  fmin_s = min_i f_s,i,  mu_js = mu_j + A_j . z_s
    nei[j] = (1/S) sum_s EI(mu_js, sqrt(rho_j), fmin_s)
with EI of acquisition.rs:141-171 as estimator.expected_improvement states it (ei below is that function over arrays)."""
import math

import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import erfc


def ei(mean, std, fmin):
    """estimator.expected_improvement over broadcast arrays: the std == 0 branch (|std| <= f64::EPSILON) included."""
    mean, std, fmin = np.broadcast_arrays(np.asarray(mean, np.float64), np.asarray(std, np.float64), np.asarray(fmin, np.float64))
    flat = std <= np.finfo(float).eps
    sd = np.where(flat, 1.0, std)
    zz = -(mean - fmin) / sd
    smooth = -(mean - fmin) * (0.5 * erfc(-zz / math.sqrt(2.0))) + sd * np.exp(-0.5 * zz * zz) / math.sqrt(2.0 * math.pi)
    return np.where(flat, np.where(mean < fmin, -(mean - fmin), 0.0), np.maximum(smooth, 0.0))


def parts(sigma, mb):
    """(L_b, A, rho) of the definition, in float64."""
    S = np.asarray(sigma, np.float64)
    Lb = np.linalg.cholesky(S[:mb, :mb])
    A = solve_triangular(Lb, S[mb:, :mb].T, lower=True).T if S.shape[0] > mb else np.zeros((0, mb))
    rho = np.maximum(np.diag(S)[mb:] - np.sum(A * A, axis=1), 0.0)
    return Lb, A, rho


def nei(mu, sigma, mb, z):
    """(nei[mc], rho[mc], fmin_s[S]) of the definition."""
    mu = np.asarray(mu, np.float64)
    z = np.atleast_2d(np.asarray(z, np.float64))
    Lb, A, rho = parts(sigma, mb)
    fmin_s = np.min(mu[None, :mb] + z @ Lb.T, axis=1)
    mu_js = mu[None, mb:] + z @ A.T  # [S, mc]
    vals = ei(mu_js, np.sqrt(rho)[None, :], fmin_s[:, None])
    return vals.sum(axis=0) / z.shape[0], rho, fmin_s


def argmax_last(v):
    return len(v) - 1 - int(np.argmax(np.asarray(v)[::-1]))


def bars(dtype, amplitude):
    """The project's plain bars scaled to y units (kg_ref.bars): nei and fmin_s are means and differences of means."""
    return (1e-8 if dtype == np.float64 else 1e-4) * max(1.0, math.sqrt(amplitude))
