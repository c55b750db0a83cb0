"""NumPy fp64 restatement of the posterior sample paths (hbegp_paths_*).

Pathwise conditioning (Matheron's rule) on a random-Fourier-feature prior draw, in the model's normalised y space:

    f_s(x) = phi(x) . w_s + k(x, X) . v_s,    v_s = K^-1 (y - Phi(X) w_s - sqrt(noise) eps_s),   K = k(X, X) + noise I
    phi_j(x) = sqrt(2 c / F) cos(om_j . x + b_j),   om_jk = omega0_jk / ell_k

v by Cholesky solves; the gradient with psi(r) = phi_nu'(r) / r and 0 at r = 0 (as predict_grad_ref has it); and the covariance
of the paths given (omega, b) in closed form."""
import math

import numpy as np


def scaled_dist(A, B, ell):
    return np.sqrt((((A[:, None, :] - B[None, :, :]) / ell) ** 2).sum(-1))


def matern(r, nu):
    if math.isinf(nu):
        return np.exp(-0.5 * r * r)
    if nu == 0.5:
        return np.exp(-r)
    if nu == 1.5:
        k = math.sqrt(3.0) * r
        return (1.0 + k) * np.exp(-k)
    if nu == 2.5:
        k = math.sqrt(5.0) * r
        return (1.0 + k + k * k / 3.0) * np.exp(-k)
    raise ValueError(nu)


def matern_psi(r, nu):
    """phi'(r) / r; the caller zeroes r = 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if math.isinf(nu):
            return -np.exp(-0.5 * r * r)
        if nu == 0.5:
            return -np.exp(-r) / r
        if nu == 1.5:
            return -3.0 * np.exp(-math.sqrt(3.0) * r)
        if nu == 2.5:
            k = math.sqrt(5.0) * r
            return -(5.0 / 3.0) * (1.0 + k) * np.exp(-k)
    raise ValueError(nu)


class Paths:
    """S paths of the model (X, y, amp, ell, nu, noise) from the draws (omega0 [F, d], phase [F], w [S, F], eps [S, n] or None)."""

    def __init__(self, X, y, amp, ell, nu, noise, omega0, phase, w, eps=None, solve=None):
        f8 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
        self.X, self.y, self.amp, self.ell, self.nu, self.noise = f8(X), f8(y), float(amp), f8(ell), nu, float(noise)
        self.om = f8(omega0) / self.ell[None, :]
        self.b, self.w = f8(phase), np.atleast_2d(f8(w))
        self.F = self.om.shape[0]
        self.A = math.sqrt(2.0 * self.amp / self.F)
        n = len(self.y)
        self.K = self.amp * matern(scaled_dist(self.X, self.X, self.ell), nu) + self.noise * np.eye(n)
        self.resid = self.y[None, :] - self.w @ self.features(self.X).T
        if eps is not None:
            self.resid = self.resid - math.sqrt(self.noise) * np.atleast_2d(f8(eps))
        if solve is None:
            L = np.linalg.cholesky(self.K)
            self.v = np.linalg.solve(L.T, np.linalg.solve(L, self.resid.T))  # [n, S]
        else:
            self.v = np.stack([solve(r) for r in self.resid], axis=1)

    def features(self, x):
        return self.A * np.cos(f8_(x) @ self.om.T + self.b[None, :])

    def kstar(self, x):
        return self.amp * matern(scaled_dist(f8_(x), self.X, self.ell), self.nu)

    def evaluate(self, x, want_grad=True):
        """x [m, d] (shared) or [S, m, d] (per path) -> f [S, m], df [S, m, d]."""
        x = f8_(x)
        if x.ndim == 3:
            out = [Paths._eval_one(self, x[s], slice(s, s + 1), want_grad) for s in range(x.shape[0])]
            return np.concatenate([o[0] for o in out]), (np.concatenate([o[1] for o in out]) if want_grad else None)
        return self._eval_one(x, slice(None), want_grad)

    def _eval_one(self, x, sl, want_grad):
        w, v = self.w[sl], self.v[:, sl]
        th = x @ self.om.T + self.b[None, :]
        f = self.A * (w @ np.cos(th).T) + (self.kstar(x) @ v).T
        if not want_grad:
            return f, None
        # features: -A sum_j w_sj sin(th_ij) om_jk
        df = -self.A * np.einsum("sj,ij,jk->sik", w, np.sin(th), self.om)
        r = scaled_dist(x, self.X, self.ell)
        psi = np.where(r > 0, matern_psi(r, self.nu), 0.0)
        diff = (x[:, None, :] - self.X[None, :, :]) / self.ell**2  # [m, n, d]
        df += self.amp * np.einsum("in,ns,ink->sik", psi, v, diff)
        return f, df

    def evaluate_by_matmul(self, x):
        """`evaluate` at shared points x [m, d] with every contraction a matrix product, one per gradient component: the same
        sums, but O(S F m d) where the einsum above walks S F m d^2 at best (S = 1000, F = 16384: minutes against a second)."""
        x = f8_(x)
        th = x @ self.om.T + self.b[None, :]
        cs, sn = np.cos(th), np.sin(th)
        f = self.A * (self.w @ cs.T) + (self.kstar(x) @ self.v).T
        r = scaled_dist(x, self.X, self.ell)
        psi = np.where(r > 0, matern_psi(r, self.nu), 0.0)
        df = np.empty(f.shape + (x.shape[1],))
        for k in range(x.shape[1]):
            slope = psi * ((x[:, None, k] - self.X[None, :, k]) / self.ell[k] ** 2)  # [m, n]
            df[:, :, k] = -self.A * (self.w @ (sn * self.om[None, :, k]).T) + self.amp * (slope @ self.v).T
        return f, df

    def mean(self, x):
        return self.kstar(x) @ np.linalg.solve(self.K, self.y)

    def covariance(self, x):
        """Covariance of f(x) over (w, eps) given (omega, b): Phi* Phi*^T - A Phi_X Phi*^T - Phi* Phi_X^T A^T + A (Phi_X Phi_X^T +
        noise I) A^T with A = K* K^-1 (noise I only with a noise draw)."""
        Ps, PX = self.features(x), self.features(self.X)
        Am = np.linalg.solve(self.K, self.kstar(x).T).T
        return Ps @ Ps.T - Am @ (PX @ Ps.T) - (Ps @ PX.T) @ Am.T + Am @ (PX @ PX.T + self.noise * np.eye(len(self.y))) @ Am.T

    def exact_covariance(self, x):
        Ks = self.kstar(x)
        return self.amp * matern(scaled_dist(f8_(x), f8_(x), self.ell), self.nu) - Ks @ np.linalg.solve(self.K, Ks.T)


def f8_(a):
    return np.asarray(a, dtype=np.float64)


def gather(f, df, idx):
    """Per-path values from values at a shared pool of points: path s at its points pool[idx[s, i]] -> (f [S, m], df [S, m, d])
    from f [S, P], df [S, P, d] at the pool.  A path's value at a point depends on nothing else, so this is `evaluate` at
    pool[idx] without S times the pool's cosines."""
    rows = np.arange(f.shape[0])[:, None]
    return f[rows, idx], df[rows, idx]
