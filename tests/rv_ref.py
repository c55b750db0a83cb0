"""NumPy fp64 reference of the GP with known per-row noise variances (the `_rv` entry points), on the kernel
functions of oracle.gpr_oracle.

In the model's normalised y space, theta = [ln s2, ln c, ln ell_k]:

    K = c Matern(X, X) + diag(s2 + v),   alpha = K^-1 y,   lml = -1/2 y.alpha - sum ln L_ii - n/2 ln 2 pi
    d lml / d theta_j = 1/2 tr((alpha alpha^T - K^-1) dK_j),   dK_0 = s2 I (v is data: it has no derivative)
    predict: mean = K* alpha, var = c + 1e-5 - diag(K* K^-1 K*^T) -- the latent function's, without s2 and v
    leave-one-out: mu_i = y_i - alpha_i / m_i, var_i = 1 / m_i (the noisy observation's: it contains s2 + v_i), m = diag K^-1
    sample paths: residual r_s = y - Phi(X) w_s - sqrt(s2 + v) o eps_s, v_s = K^-1 r_s

`CPU_SHAPES`, `GPU_SHAPES` and `case()` are the inputs the CPU file checks against scikit-learn (cond(K) <= 1e4 there, asserted) and the GPU file
reuses, so that LAPACK is not the limit of any comparison."""
import math

import numpy as np
from scipy.linalg import solve_triangular

from oracle import gpr_oracle as O

S2, AMP, SHIFT = 0.05, 1.3, 0.07
CPU_SHAPES = [(5, 1, 0.5), (60, 3, 2.5), (100, 8, 1.5), (128, 32, math.inf), (200, 9, 2.5)]
COND_MAX = 1e4
NUS = [0.5, 1.5, 2.5, math.inf]
# (n, d) of the GPU file's evaluations, the smallest sizes that reach each stage: the single launch with padding to 128 / plain / full
# with the last feature chunk; the launch path with one ragged tile row / plain / full diagonal tiles; the f32 and the f64 task queue
GPU_SHAPES = [(5, 1), (100, 8), (128, 32), (129, 3), (200, 9), (256, 4), (641, 4), (2048, 8)]
GPU_EXTRA_SHAPES = [(300, 9), (1024, 8), (258, 4)]  # fits, the v = 0 comparisons and the incremental chain


def case(n, d, seed=None):
    """X [n, d] uniform in the unit cube (beyond 64 rows: in the cube that holds them at the density of 64), y a smooth function plus noise of the rows' own variance, v uniform in [0, 0.2] with
    every seventh entry 0, ell uniform in [0.3, 1.3]."""
    rng = np.random.default_rng(1000 * n + d if seed is None else seed)
    X = rng.random((n, d)) * max(1.0, (n / 64.0) ** (1.0 / d))  # beyond 64 rows the cube grows with n: the density, and with it cond(K), stays
    v = rng.uniform(0.0, 0.2, n)
    v[::7] = 0.0
    f = np.sin(3.0 * X[:, 0]) + 0.5 * np.cos(2.0 * X.sum(axis=1))
    y = f + np.sqrt(S2 + v) * rng.standard_normal(n)
    y = (y - y.mean()) / y.std()
    ell = rng.uniform(0.3, 1.3, d)
    theta = np.log(np.concatenate([[S2, AMP], ell]))
    return X, y, v, theta


def kernel_and_grads(X, v, noise, amp, ell, nu):
    """K [n, n] with v on the diagonal and dK/dtheta_j [n, n, p]."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    K, g = O.product_theta_grad(X, float(amp), np.asarray(ell, dtype=np.float64), nu)
    K = K + np.diag(float(noise) + np.asarray(v, dtype=np.float64))
    dK = np.concatenate([(float(noise) * np.eye(n))[:, :, None], g], axis=2)
    return K, dK


def kernel_matrix(X, v, theta, nu):
    p = np.exp(np.asarray(theta, dtype=np.float64))
    X = np.asarray(X, dtype=np.float64)
    return O.product_kernel(X, X, float(p[1]), p[2:], nu) + np.diag(float(p[0]) + np.asarray(v, dtype=np.float64))


def evaluate(X, y, v, theta, nu, want_grad=True):
    """dict(lml, grad, alpha, kinv, ldiag, K, L, Linv, cond) at a log-space theta (no clamping: the tests pass none)."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    p = np.exp(np.asarray(theta, dtype=np.float64))
    K, dK = kernel_and_grads(X, np.zeros(n) if v is None else v, p[0], p[1], p[2:], nu)
    L = np.linalg.cholesky(K)
    Linv = solve_triangular(L, np.eye(n), lower=True)
    kinv = Linv.T @ Linv
    alpha = Linv.T @ (Linv @ y)
    out = dict(K=K, L=L, Linv=Linv, kinv=kinv, alpha=alpha, ldiag=np.diag(L).copy(),
               lml=-0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * n * math.log(2.0 * math.pi))
    if want_grad:
        W = np.outer(alpha, alpha) - kinv
        out["grad"] = np.array([0.5 * float((W * dK[:, :, j]).sum()) for j in range(dK.shape[2])])
    return out


def cond(K):
    w = np.linalg.eigvalsh(K)
    return float(w[-1] / w[0])


def predict(Xs, X, ev, theta, nu):
    """(mean, var) of the latent function at Xs from evaluate()'s dict: var = c + 1e-5 - |L^-1 k*|^2, clamped at 0."""
    p = np.exp(np.asarray(theta, dtype=np.float64))
    Ks = O.product_kernel(np.asarray(Xs, dtype=np.float64), np.asarray(X, dtype=np.float64), float(p[1]), p[2:], nu)
    Q = Ks @ ev["Linv"].T
    return Ks @ ev["alpha"], np.maximum(p[1] + O.MIN_NOISE - (Q * Q).sum(axis=1), 0.0)


def loo(X, y, v, theta, nu, want_grad=True):
    """Closed-form leave-one-out: dict(mean, var, lpd, loo[, grad]); var is that of the left-out noisy observation."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    p = np.exp(np.asarray(theta, dtype=np.float64))
    K, dK = kernel_and_grads(X, v, p[0], p[1], p[2:], nu)
    M = np.linalg.inv(K)
    M = 0.5 * (M + M.T)
    alpha, m = M @ y, np.diag(M).copy()
    out = dict(mean=y - alpha / m, var=1.0 / m, lpd=0.5 * np.log(m) - alpha * alpha / (2.0 * m) - 0.5 * math.log(2.0 * math.pi))
    out["loo"] = float(out["lpd"].sum())
    if want_grad:  # Rasmussen & Williams eq. 5.13 with Z_j = M dK_j
        g = []
        for j in range(dK.shape[2]):
            Z = M @ dK[:, :, j]
            g.append(float(((alpha * (Z @ alpha) - 0.5 * (1.0 + alpha * alpha / m) * np.einsum("ik,ki->i", Z, M)) / m).sum()))
        out["grad"] = np.array(g)
    return out


def loo_by_deletion(X, y, v, theta, nu):
    """(mean, var) of y_i predicted from the other rows, row by row; var includes s2 + v_i."""
    X, y, v = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n = len(y)
    p = np.exp(np.asarray(theta, dtype=np.float64))
    K, _ = kernel_and_grads(X, v, p[0], p[1], p[2:], nu)
    mean, var = np.zeros(n), np.zeros(n)
    for i in range(n):
        keep = np.arange(n) != i
        sol = np.linalg.solve(K[np.ix_(keep, keep)], np.column_stack([y[keep], K[keep, i]]))
        mean[i] = K[i, keep] @ sol[:, 0]
        var[i] = K[i, i] - K[i, keep] @ sol[:, 1]
    return mean, var


def paths_residual(X, y, v, theta, omega0, phase, w, eps):
    """r [S, n] = y - Phi(X) w_s - sqrt(s2 + v) o eps_s (eps None: no noise draw), phi_j(x) = sqrt(2 c / F) cos(om_j . x + b_j)."""
    p = np.exp(np.asarray(theta, dtype=np.float64))
    om = np.asarray(omega0, dtype=np.float64) / p[2:][None, :]
    F = om.shape[0]
    Phi = math.sqrt(2.0 * p[1] / F) * np.cos(np.asarray(X, dtype=np.float64) @ om.T + np.asarray(phase, dtype=np.float64)[None, :])
    r = np.asarray(y, dtype=np.float64)[None, :] - np.atleast_2d(np.asarray(w, dtype=np.float64)) @ Phi.T
    if eps is not None:
        vv = np.zeros(len(y)) if v is None else np.asarray(v, dtype=np.float64)
        r = r - np.sqrt(p[0] + vv)[None, :] * np.atleast_2d(np.asarray(eps, dtype=np.float64))
    return r


# ---- the estimator's scenario: means of replicates with the variance of each mean ---------------------------------------------------
EST_SEED = 4  # tests/test_rv_cpu.py: the reference, fitted by scipy, covers 30 of 30 rows for this seed


def estimator_data(seed=EST_SEED):
    """30 configurations x 4 replicates of a noisy quadratic whose noise grows along the first feature, the rows shuffled:
    (x [120, 2], y [120], the noiseless function)."""
    rng = np.random.default_rng(seed)
    xc = rng.random((30, 2))
    f = lambda x: 2.0 + 6.0 * ((x - 0.4) ** 2).sum(axis=1)  # noqa: E731
    x = np.repeat(xc, 4, axis=0)
    sd = 0.15 + 0.6 * x[:, 0]
    y = f(x) + sd * rng.standard_normal(len(x))
    perm = rng.permutation(len(x))
    return x[perm], y[perm], f


def rows_within_two_sigma(mean, var, v, truth):
    """How many training rows have the noiseless function within two posterior-plus-v standard deviations of the posterior mean."""
    return int((np.abs(np.asarray(mean) - truth) <= 2.0 * np.sqrt(np.asarray(var) + v)).sum())
