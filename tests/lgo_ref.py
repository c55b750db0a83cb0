"""NumPy fp64 restatement of leave-group-out cross-validation in closed form (hbegp_model_lgo_*, hbegp_problem_eval_lgo;
DESIGN.md section 33), on the kernel matrices of oracle.gpr_oracle, like tests/loo_ref.py.

In the model's normalised y space, with K = c Matern(X, X) + diag(s2 + v), M = K^-1, alpha = M y and a group's row set I (s rows):

    Sigma_g = (M_II)^-1,   r_g = Sigma_g alpha_I,   mu_g = y_I - r_g,   var = diag Sigma_g (the observations': it includes s2),
    lpd_g = -1/2 alpha_I^T r_g + 1/2 ln|M_II| - s/2 ln 2 pi,   lgo = sum_g lpd_g

M_II is formed as the device forms it, the Gram matrix of the group's columns of L^-1.  The gradient in the order
[ln s2, ln c, ln ell_k] is formed twice: by the book, group by group with Z_j = M dK_j, and through the identity the device uses,
one n^3 product C = Y Y^T for all parameters with Y[:, I] = M[:, I] chol(1/2 (r_g r_g^T + Sigma_g))."""
import math

import numpy as np
from scipy.linalg import solve_triangular

import loo_ref as LR
from oracle import gpr_oracle as O


def dense_groups(groups, n):
    """The labels -> member lists in order of first appearance, rows ascending inside a group (None: singletons)."""
    if groups is None:
        return [np.array([i]) for i in range(n)]
    groups = np.asarray(groups).reshape(-1)
    assert groups.shape == (n,)
    order, members = {}, []
    for i, g in enumerate(groups.tolist()):
        if g not in order:
            order[g] = len(members)
            members.append([])
        members[order[g]].append(i)
    return [np.array(m) for m in members]


def lgo(X, y, noise, amp, ell, nu, groups, want_grad=True, by_the_book=False, rv=None):
    """dict(mean [n], var [n], lpd [G], lgo, members[, grad[, grad_book]])."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    X = np.asarray(X, dtype=np.float64)
    if want_grad:
        K, dK = LR.kernel_and_grads(X, noise, amp, ell, nu)
    else:
        K = O.product_kernel(X, X, float(amp), np.asarray(ell, dtype=np.float64), nu) + float(noise) * np.eye(n)
    if rv is not None:
        K = K + np.diag(np.asarray(rv, dtype=np.float64))
    L = np.linalg.cholesky(K)
    Linv = solve_triangular(L, np.eye(n), lower=True)
    M = Linv.T @ Linv
    alpha = Linv.T @ (Linv @ y)
    members = dense_groups(groups, n)
    mean, var, a = np.zeros(n), np.zeros(n), np.zeros(n)
    lpd = np.zeros(len(members))
    Y = np.zeros((n, n))
    sig, res = [], []
    for g, I in enumerate(members):
        Li = Linv[:, I]
        MII = Li.T @ Li
        Lm = np.linalg.cholesky(MII)
        Sigma = np.linalg.inv(MII)
        Sigma = 0.5 * (Sigma + Sigma.T)
        r = Sigma @ alpha[I]
        mean[I], var[I], a[I] = y[I] - r, np.diag(Sigma), r
        lpd[g] = -0.5 * float(alpha[I] @ r) + float(np.log(np.diag(Lm)).sum()) - 0.5 * len(I) * math.log(2.0 * math.pi)
        sig.append(Sigma)
        res.append(r)
        if want_grad:
            Y[:, I] = M[:, I] @ np.linalg.cholesky(0.5 * (np.outer(r, r) + Sigma))
    out = dict(mean=mean, var=var, lpd=lpd, lgo=float(lpd.sum()), members=members, alpha=alpha)
    if not want_grad:
        return out
    u = M @ a
    W = np.outer(u, alpha) + np.outer(alpha, u) - 2.0 * (Y @ Y.T)
    out["grad"] = np.array([0.5 * float((W * dK[:, :, j]).sum()) for j in range(dK.shape[2])])
    if by_the_book:
        # d lpd_g = -alpha_I^T d r - 1/2 r^T d(M_II) r ... written out from dM = -M dK M, d alpha = -M dK alpha:
        #   d(M_II) = -(Z M)_II,  d alpha_I = -(Z alpha)_I,  d Sigma = Sigma (Z M)_II Sigma,  d ln|M_II| = -tr(Sigma (Z M)_II)
        g = []
        for j in range(dK.shape[2]):
            Z = M @ dK[:, :, j]
            ZM, Za = Z @ M, Z @ alpha
            tot = 0.0
            for I, Sigma, r in zip(members, sig, res):
                P = ZM[np.ix_(I, I)]
                # d(alpha_I^T Sigma alpha_I) = 2 r^T d alpha_I + alpha_I^T dSigma alpha_I = -2 r^T (Z alpha)_I + r^T P r
                tot += -0.5 * (-2.0 * float(r @ Za[I]) + float(r @ P @ r)) - 0.5 * float(np.trace(Sigma @ P))
            g.append(tot)
        out["grad_book"] = np.array(g)
    return out


def lgo_at_theta(X, y, theta, nu, groups, lo=None, hi=None, **kw):
    """lgo at a log-space theta with the engine's clamping (fit.rs:94-96): kernel parameters clamped into [lo, hi], the noise not."""
    v = np.exp(np.asarray(theta, dtype=np.float64))
    if lo is not None:
        v[1:] = np.minimum(np.maximum(v[1:], np.asarray(lo)[1:]), np.asarray(hi)[1:])
    return lgo(X, y, v[0], v[1], v[2:], nu, groups, **kw)


def group_mix(n, seed=0):
    """Groups of 1, 1, 2, 5, 17, 33 and 64 rows plus singletons for the rest, the rows scattered by a permutation; labels are
    arbitrary ints (negative ones too)."""
    perm = np.random.default_rng(seed).permutation(n)
    labels = np.empty(n, dtype=np.int32)
    pos, lab = 0, -3
    for s in (1, 1, 2, 5, 17, 33, 64):
        labels[perm[pos:pos + s]] = lab
        pos, lab = pos + s, lab + 7
    for i in perm[pos:]:
        labels[i] = lab
        lab += 1
    return labels
