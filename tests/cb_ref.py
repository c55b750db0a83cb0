"""The confidence bound of hbegp_confidence_bound_* restated in NumPy, for the tests (test_cb_cpu.py, test_gpu_cb.py):

    cb = mu + kappa sigma,   grad[i] = dmean[i] + kappa dvar[i] / (2 sigma),   sigma = sqrt(var)

all of it in float64 on the posteriors given (mean, var [m]; dmean, dvar [m, d]).  "sigma = 0" is the library's
!(sigma > 2.220446049250313e-16): cb = mu and grad = dmean, the sigma term dropped and never divided; kappa = 0 drops it too.  A NaN
mean or variance gives NaN in cb and in the whole gradient row."""
import numpy as np

EPS = 2.220446049250313e-16


def cb_grad(mean, var, dmean, dvar, kappa):
    """(cb[m], grad[m, d], scale[m]): the bound, its gradient and, per row, |dmean| + |kappa| |dvar| / (2 sigma) at its largest
    feature -- the size of the terms the gradient is the sum of, which grad_bar scales with."""
    mu = np.asarray(mean, np.float64).reshape(-1)
    v = np.asarray(var, np.float64).reshape(-1)
    dm = np.asarray(dmean, np.float64).reshape(len(mu), -1)
    dv = np.asarray(dvar, np.float64).reshape(len(mu), -1)
    kappa = float(kappa)
    with np.errstate(all="ignore"):
        sd = np.sqrt(v)
        live = (sd > EPS) & (kappa != 0.0)
        safe = np.where(live, sd, 1.0)
        cb = np.where(live, mu + kappa * safe, mu)
        term = np.where(live[:, None], dv / (2.0 * safe)[:, None], 0.0)
        grad = np.where(live[:, None], dm + kappa * term, dm)
        scale = (np.abs(dm) + abs(kappa) * np.abs(term)).max(axis=1) if dm.shape[1] else np.zeros(len(mu))
    bad = np.isnan(mu) | np.isnan(v)
    cb = np.where(bad, np.nan, cb)
    grad = np.where(bad[:, None], np.nan, grad)
    return cb, grad, scale


def argmin_first(v):
    """The first index of the minimum of v; a NaN never wins; -1 where no entry is a number (or there is none)."""
    a = np.asarray(v, np.float64).reshape(-1)
    best = -1
    for i, e in enumerate(a):
        if e == e and (best < 0 or e < a[best]):
            best = i
    return best


def _base(dtype):
    return 1e-8 if np.dtype(dtype) == np.float64 else 1e-4  # parity_rules.TOL64 / TOL32


def value_bar(dtype, ref):
    """The project's standing bar: 1e-8 (f64) / 1e-4 (f32) times max(1, |reference value|), per entry of `ref` (a NaN reference
    has to be met exactly: its bar is 0)."""
    ref = np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(ref), _base(dtype) * np.maximum(1.0, np.abs(ref)), 0.0)


def grad_bar(dtype, ref, scale):
    """Per row: the value's bar times max(1, |dmean| + |kappa| |dvar| / (2 sigma)) (cb_grad's scale; 1 where it is not finite)."""
    ref = np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        size = np.where(np.isfinite(ref), np.maximum(1.0, np.abs(ref)), 1.0)
    return _base(dtype) * size * np.maximum(1.0, np.nan_to_num(np.asarray(scale, np.float64), nan=1.0, posinf=1.0))
