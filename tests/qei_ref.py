"""NumPy restatement of the Monte Carlo batch expected improvement (include/hbegp.h, hbegp_qei_*), shared by the CPU and GPU tests.

Per batch of q points: mu = the posterior mean, Sigma = K** + (1e-5 + jitter) I - Q^T Q (tests/posterior_cov_ref.py), L = chol(Sigma),
f_s = mu + L z_s, j_s = argmin (ties to the lowest index), I_s = max(0, fmin - f_s,j_s), qEI = mean_s I_s.  The gradient is the
hand-written reverse pass of the header: mubar, Lbar, Sigmabar = sym(L^-T Phi(L^T Lbar) L^-1), then
dqEI/dx_a,k = mubar_a dmu_a/dx_a,k + 2 sum_c Sigmabar_ac (dk(x_a, x_c)/dx_a,k - w_a,k . q_c) with the bounded w = L_K^-1 dk*/dx and
q = L_K^-1 k*.  qei_torch is the same forward pass in torch (float64, CPU), for autograd."""
import math

import numpy as np
from scipy.linalg import solve_triangular

import posterior_cov_ref as PC
import predict_grad_ref as PG
from oracle import gpr_oracle as O


class Posterior:
    """The model pieces the restatement needs, from the oracle: alpha and L_K of K = k(X, X) + noise I."""

    def __init__(self, X, y, amplitude, length_scale, nu, noise, alpha=None):
        self.X = np.asarray(X, np.float64)
        self.amp, self.ell, self.nu, self.noise = float(amplitude), np.asarray(length_scale, np.float64), nu, float(noise)
        self.LK = np.linalg.cholesky(PC.kernel_matrix(self.X, self.amp, self.ell, nu, self.noise))
        if alpha is None:
            alpha = np.linalg.solve(self.LK.T, np.linalg.solve(self.LK, np.asarray(y, np.float64)))
        self.alpha = np.asarray(alpha, np.float64)

    def mean_cov(self, xb, jitter=0.0):
        """(mu[q], Sigma[q, q]) at the q points xb."""
        xb = np.asarray(xb, np.float64)
        ks = PC._k(xb, self.X, self.amp, self.ell, self.nu)
        Q = solve_triangular(self.LK, ks.T, lower=True)
        S = PC._k(xb, xb, self.amp, self.ell, self.nu) - Q.T @ Q
        S[np.diag_indices(len(S))] += O.MIN_NOISE + jitter
        return ks @ self.alpha, S

    def batch(self, xb, jitter=0.0):
        """(mu[q], Sigma[q, q], dmu[q, d], Q[n, q], W[n, q, d], dKss[q, q, d]) at the q points xb."""
        xb = np.asarray(xb, np.float64)
        ks = PC._k(xb, self.X, self.amp, self.ell, self.nu)
        mu = ks @ self.alpha
        Q = solve_triangular(self.LK, ks.T, lower=True)
        S = PC._k(xb, xb, self.amp, self.ell, self.nu) - Q.T @ Q
        S[np.diag_indices(len(S))] += O.MIN_NOISE + jitter
        dk = PG._dk(xb, self.X, self.amp, self.ell, self.nu)  # [q, n, d]
        q, n, d = dk.shape
        W = solve_triangular(self.LK, dk.transpose(1, 0, 2).reshape(n, q * d), lower=True).reshape(n, q, d)
        dmu = np.einsum("qnd,n->qd", dk, self.alpha)
        return mu, S, dmu, Q, W, PG._dk(xb, xb, self.amp, self.ell, self.nu)


def draws(mu, L, z, fmin):
    """(I[S], j[S]) of the draws f_s = mu + L z_s."""
    f = np.asarray(mu)[None, :] + np.asarray(z, np.float64) @ L.T
    j = np.argmin(f, axis=1)  # ties to the lowest index
    imp = fmin - f[np.arange(len(f)), j]
    return np.maximum(imp, 0.0), j


def qei_from(mu, Sigma, z, fmin):
    """qEI from a mean and a covariance (e.g. hbegp_predict_cov's)."""
    I, _ = draws(mu, np.linalg.cholesky(Sigma), z, fmin)
    return float(I.sum() / len(I))


def sigma_bar(L, Lbar):
    """Murray (2016): X = L^-T Phi(L^T Lbar) L^-1, Sigmabar = (X + X^T) / 2."""
    M = np.tril(L.T @ Lbar)
    M[np.diag_indices(len(M))] *= 0.5
    P = solve_triangular(L.T, M, lower=False)      # L^-T Phi
    X = solve_triangular(L.T, P.T, lower=False).T  # P L^-1 = (L^-T P^T)^T
    return 0.5 * (X + X.T)


def qei_batch(post, xb, z, fmin, jitter=0.0):
    """(qei, grad[q, d]) of one batch by the restatement; raises LinAlgError where Sigma does not factor."""
    mu, S, dmu, Q, W, dKss = post.batch(xb, jitter)
    L = np.linalg.cholesky(S)
    z = np.asarray(z, np.float64)
    I, j = draws(mu, L, z, fmin)
    ns, q = z.shape
    qei = float(I.sum() / ns)
    act = I > 0
    mubar = -np.bincount(j[act], minlength=q) / ns
    Lbar = np.zeros((q, q))
    np.add.at(Lbar, j[act], z[act])
    Lbar = -np.tril(Lbar) / ns
    Sb = sigma_bar(L, Lbar)
    wq = np.einsum("nad,nc->acd", W, Q)  # w_a,k . q_c
    grad = mubar[:, None] * dmu + 2.0 * np.einsum("ac,acd->ad", Sb, dKss - wq)
    return qei, grad


def qei_many(post, Xb, z, fmin, jitter=0.0):
    """qei[B], grad[B, q, d] of every batch of Xb [B, q, d]."""
    out = [qei_batch(post, xb, z, fmin, jitter) for xb in np.asarray(Xb, np.float64)]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out])


def draw_values(post, xb, z, jitter=0.0):
    """f[S, q] = mu + L z_s of one batch."""
    mu, S = post.mean_cov(xb, jitter)
    return mu[None, :] + np.asarray(z, np.float64) @ np.linalg.cholesky(S).T


def top_two_gap(post, xb, z, fmin, jitter=0.0):
    """The smallest gap between the two lowest entries of a draw over the improving draws, and the smallest |fmin - f_min| over
    all draws: how far the batch is from a kink of the sample average (where a float32 evaluation may pick another branch)."""
    f = draw_values(post, xb, z, jitter)
    fs = np.sort(f, axis=1)
    imp = fmin - fs[:, 0]
    gap = (fs[:, 1] - fs[:, 0])[imp > 0] if f.shape[1] > 1 else np.array([np.inf])
    return float(gap.min()) if gap.size else math.inf, float(np.abs(imp).min())


# ---- the same forward pass in torch (float64, CPU), for autograd ----------------------------------------------------------
def _phi_torch(torch, r, nu):
    if math.isinf(nu):
        return torch.exp(-0.5 * r * r)
    if nu == 0.5:
        return torch.exp(-r)
    if nu == 1.5:
        k = math.sqrt(3.0) * r
        return (1.0 + k) * torch.exp(-k)
    if nu == 2.5:
        k = math.sqrt(5.0) * r
        return (1.0 + k + k * k / 3.0) * torch.exp(-k)
    raise ValueError(nu)


def qei_torch(post, xb, z, fmin, jitter=0.0):
    """(qei, grad[q, d]) by torch.autograd through the whole forward pass from the points (distinct points, none at a training
    point: the diagonal of K** is the constant c, as every r = 0 term is)."""
    import torch

    x = torch.tensor(np.asarray(xb, np.float64), dtype=torch.float64, requires_grad=True)
    ell = torch.tensor(post.ell, dtype=torch.float64)
    Xt = torch.tensor(post.X, dtype=torch.float64)
    s, St = x / ell, Xt / ell
    rs = torch.sqrt(((s[:, None, :] - St[None, :, :]) ** 2).sum(-1))
    ks = post.amp * _phi_torch(torch, rs, post.nu)
    mu = ks @ torch.tensor(post.alpha, dtype=torch.float64)
    Q = torch.linalg.solve_triangular(torch.tensor(post.LK, dtype=torch.float64), ks.T, upper=False)
    q = x.shape[0]
    eye = torch.eye(q, dtype=torch.float64)
    d2 = ((s[:, None, :] - s[None, :, :]) ** 2).sum(-1)
    r = torch.sqrt(d2 + eye)  # the diagonal is replaced below; + eye keeps sqrt away from 0 there
    Kss = torch.where(eye > 0, torch.full_like(d2, post.amp), post.amp * _phi_torch(torch, r, post.nu))
    Sigma = Kss + (O.MIN_NOISE + jitter) * eye - Q.T @ Q
    L = torch.linalg.cholesky(Sigma)
    zt = torch.tensor(np.asarray(z, np.float64), dtype=torch.float64)
    f = mu[None, :] + zt @ L.T
    fmn = f.min(dim=1).values
    val = torch.clamp(fmin - fmn, min=0.0).mean()
    val.backward()
    return float(val.detach()), x.grad.numpy().copy()
