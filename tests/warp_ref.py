"""NumPy restatement of input warping (include/hbegp.h: hbegp_warp_*, hbegp_problem_eval_xgrad, hbegp_problem_eval_warped; DESIGN.md
section 34), shared by the CPU and GPU tests.

Warp of feature k: u = 1 - (1 - x^a)^b on [0, 1] (Kumaraswamy CDF), formed as -expm1(b log1p(-x^a)).
G_ik = d lml / d x_ik = sum_j W_ij c psi(r_ij) (x_ik - x_jk) / ell_k^2 with W = alpha alpha^T - K^-1 and psi = phi'(r) / r
(predict_grad_ref.psi; 0 at r = 0: the diagonal and duplicate rows).  Neither the noise nor known row variances enter the map
x -> K other than through W.  The warped objective lml(w(X; a, b), theta) has the gradient [theta's p entries at the warped rows,
sum_i G_ik du_ik/dln a_k, sum_i G_ik du_ik/dln b_k]."""
import math

import numpy as np

from oracle import gpr_oracle as O
from predict_grad_ref import psi


def warp(X, ab):
    """(U, dU/dln a, dU/dln b, dU/dx) of rows X [m, d] in fp64; ab = [a_1..a_d, b_1..b_d].  The ends take their limits."""
    X = np.asarray(X, np.float64)
    d = X.shape[-1]
    a, b = np.asarray(ab, np.float64)[:d], np.asarray(ab, np.float64)[d:]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lx = np.log(X)
        t = a * lx
        L = np.where(t < -math.log(2.0), np.log1p(-np.exp(t)), np.log(-np.expm1(t)))  # ln(1 - x^a)
        v = b * L
        U = -np.expm1(v)
        da = b * t * np.exp((b - 1.0) * L + t)
        db = -v * np.exp(v)
        dx = a * b * np.exp((a - 1.0) * lx + (b - 1.0) * L)
    lo, hi = X <= 0.0, X >= 1.0
    U = np.where(lo, 0.0, np.where(hi, 1.0, U))
    da = np.where(lo | hi, 0.0, da)
    db = np.where(lo | hi, 0.0, db)
    ends = lambda ex, other: np.where(ex < 1.0, np.inf, np.where(ex == 1.0, other, 0.0))  # noqa: E731
    dx = np.where(lo, np.broadcast_to(ends(a, b), X.shape), np.where(hi, np.broadcast_to(ends(b, a), X.shape), dx))
    return U, da, db, dx


def unwarp(U, ab):
    """x = (1 - (1 - u)^(1/b))^(1/a)."""
    U = np.asarray(U, np.float64)
    d = U.shape[-1]
    a, b = np.asarray(ab, np.float64)[:d], np.asarray(ab, np.float64)[d:]
    with np.errstate(divide="ignore"):
        q = np.log1p(-U) / b
        M = np.where(q < -math.log(2.0), np.log1p(-np.exp(q)), np.log(-np.expm1(q)))
        x = np.exp(M / a)
    return np.where(U <= 0.0, 0.0, np.where(U >= 1.0, 1.0, x))


def params_of(theta, lo=None, hi=None):
    """(noise, c, ell) the evaluation runs with: exp(theta), the kernel parameters clamped into [lo, hi] (fit.rs:94-96)."""
    v = np.exp(np.asarray(theta, np.float64))
    if lo is not None:
        v[1:] = np.minimum(np.maximum(v[1:], np.asarray(lo, np.float64)[1:]), np.asarray(hi, np.float64)[1:])
    return float(v[0]), float(v[1]), v[2:]


def evaluate(X, y, noise, c, ell, nu, rv=None):
    """lml, its theta gradient [p], G [n, d], K, alpha, K^-1 in fp64 (numpy's LAPACK)."""
    X, y, ell = np.asarray(X, np.float64), np.asarray(y, np.float64), np.asarray(ell, np.float64)
    n, d = X.shape
    kernel, dk = O.product_theta_grad(X, c, ell, nu)
    K = kernel.copy()
    K[np.diag_indices(n)] += noise + (0.0 if rv is None else np.asarray(rv, np.float64))
    L = np.linalg.cholesky(K)
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = np.linalg.solve(K, y)
    lml = -0.5 * float(y @ alpha) - float(np.log(np.diag(L)).sum()) - 0.5 * n * math.log(2.0 * math.pi)
    W = np.outer(alpha, alpha) - Kinv
    grad = np.array([0.5 * noise * float(np.trace(W))] + [0.5 * float((W * dk[:, :, j]).sum()) for j in range(d + 1)])
    diff = (X[:, None, :] - X[None, :, :]) / ell  # [n, n, d]
    r = np.sqrt((diff * diff).sum(axis=2))
    G = np.einsum("ij,ijk->ik", W * (c * psi(r, nu)), diff / ell)
    return dict(lml=lml, grad=grad, G=G, K=K, alpha=alpha, k_inv=Kinv)


def warped_objective(X, y, theta, ab, nu, lo=None, hi=None, rv=None):
    """lml(w(X; a, b), theta) and its gradient [p + 2 d]."""
    noise, c, ell = params_of(theta, lo, hi)
    U, da, db, _ = warp(X, ab)
    ev = evaluate(U, y, noise, c, ell, nu, rv)
    grad = np.concatenate([ev["grad"], (ev["G"] * da).sum(axis=0), (ev["G"] * db).sum(axis=0)])
    return ev["lml"], grad, ev


# ---- central differences of the lml in extended precision (the check of the yardstick itself) --------------------------------

def _kernel_ld(X, c, ell, nu):
    LD = np.longdouble
    Z = X / ell
    diff = Z[:, None, :] - Z[None, :, :]
    r = np.sqrt((diff * diff).sum(axis=2))
    if math.isinf(nu):
        return c * np.exp(-LD(0.5) * r * r)
    if nu == 0.5:
        return c * np.exp(-r)
    if nu == 1.5:
        k = np.sqrt(LD(3)) * r
        return c * (1 + k) * np.exp(-k)
    k = np.sqrt(LD(5)) * r
    return c * (1 + k + k * k / 3) * np.exp(-k)


def lml_ld(X, y, noise, c, ell, nu, rv=None):
    """The lml in np.longdouble throughout (an outer-product Cholesky; small n only)."""
    LD = np.longdouble
    X, y, ell = np.asarray(X, LD), np.asarray(y, LD), np.asarray(ell, LD)
    n = len(y)
    A = _kernel_ld(X, LD(c), ell, nu)
    A[np.diag_indices(n)] += LD(noise) + (LD(0) if rv is None else np.asarray(rv, LD))
    w = y.copy()
    logdet = LD(0)
    for k in range(n):  # right-looking Cholesky with the forward substitution carried along
        piv = np.sqrt(A[k, k])
        logdet += np.log(piv)
        col = A[k + 1:, k] / piv
        w[k] /= piv
        w[k + 1:] -= col * w[k]
        A[k + 1:, k + 1:] -= np.outer(col, col)
    return -LD(0.5) * (w @ w) - logdet - LD(0.5) * n * np.log(2 * LD(np.pi))


def warp_ld(X, ab):
    LD = np.longdouble
    X = np.asarray(X, LD)
    d = X.shape[-1]
    a, b = np.asarray(ab, LD)[:d], np.asarray(ab, LD)[d:]
    return -np.expm1(b * np.log1p(-X ** a))


# ---- the reference fits: scipy's L-BFGS-B on the restated objectives ------------------------------------------------------------

def reference_fits(X, y, theta0, lo, hi, nu, ab_lo=0.2, ab_hi=5.0):
    """The plain optimum from theta0 inside [lo, hi], then the warped optimum from (that optimum, the identity warp) with a and b
    inside [ab_lo, ab_hi].  Returns dict(theta_plain, lml_plain, v_warped [p + 2 d], lml_warped, gain)."""
    from scipy.optimize import minimize

    X, y = np.asarray(X, np.float64), np.asarray(y, np.float64)
    d = X.shape[1]
    p = d + 2
    box = list(zip(np.log(lo), np.log(hi)))

    def plain(th):
        ev = evaluate(X, y, *params_of(th, lo, hi), nu)
        return -ev["lml"], -ev["grad"]

    r0 = minimize(plain, np.asarray(theta0, np.float64), jac=True, method="L-BFGS-B", bounds=box)

    def warped(v):
        lml, grad, _ = warped_objective(X, y, v[:p], np.exp(v[p:]), nu, lo, hi)
        return -lml, -grad

    wbox = box + [(math.log(ab_lo), math.log(ab_hi))] * (2 * d)
    r1 = minimize(warped, np.concatenate([r0.x, np.zeros(2 * d)]), jac=True, method="L-BFGS-B", bounds=wbox)
    return dict(theta_plain=r0.x, lml_plain=-float(r0.fun), v_warped=r1.x, lml_warped=-float(r1.fun), gain=float(r0.fun - r1.fun))
