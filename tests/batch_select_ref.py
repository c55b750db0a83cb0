"""NumPy restatement of the greedy batch selection (include/hbegp.h, hbegp_select_batch_*), shared by the CPU and GPU tests.

From the posterior mean mu and Sigma (predict_cov's matrix at jitter 0), the model's noise s2, fmin and an optional constant lie:
per step the EI of every row not yet picked (estimator.expected_improvement, vectorised), the last index of its maximum, the
fantasy f = mu_j or the lie, fmin = min(fmin, f), and the conditioning on a noisy observation f at row j:
r = Sigma[:, j] - C[:t]^T C[:t, j], r_j = v_j - 1e-5, c = r / sqrt(max(r_j, 0) + s2), v -= c^2, mu += c (f - mu_j) / sqrt(...)."""
import math

import numpy as np
from scipy.special import erfc

MIN_NOISE = 1e-5
EPS = np.finfo(float).eps


def expected_improvement(mu, var, fmin):
    """estimator.expected_improvement at (mu, sqrt(max(var, 0))) for every entry, in float64."""
    mu = np.asarray(mu, np.float64)
    sd = np.sqrt(np.maximum(np.asarray(var, np.float64), 0.0))
    flat = sd <= EPS  # ulps_eq!(std, 0.0)
    sds = np.where(flat, 1.0, sd)
    z = -(mu - fmin) / sds
    ei = -(mu - fmin) * (0.5 * erfc(-z / math.sqrt(2.0))) + sds * (np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))
    return np.where(flat, np.where(mu < fmin, -(mu - fmin), 0.0), np.maximum(ei, 0.0))


def _argmax_last(e):
    return len(e) - 1 - int(np.argmax(e[::-1]))


def select(mu, sigma, s2, fmin, k, lie=None, picks=None):
    """k greedy picks.  picks: replay these indices (the device's) instead of the argmax.  Returns a dict with idx, ei (the EI
    of each pick), best (each step's maximal EI), fantasy (f_t), mean / var (the final state, var clamped at 0) and history:
    the (mean, raw variance) after every step."""
    mu = np.array(mu, np.float64)
    S = np.asarray(sigma, np.float64)
    m = len(mu)
    v = np.diag(S).copy()
    C = np.zeros((k, m))
    picked = np.zeros(m, bool)
    fm = float(fmin)
    out = dict(idx=[], ei=[], best=[], fantasy=[], history=[])
    for t in range(k):
        e = expected_improvement(mu, v, fm)
        e[picked] = -np.inf
        j = _argmax_last(e) if picks is None else int(picks[t])
        assert not picked[j]
        out["idx"].append(j)
        out["ei"].append(float(e[j]))
        out["best"].append(float(e.max()))
        muj = mu[j]
        f = muj if lie is None else float(lie)
        out["fantasy"].append(float(f))
        r = S[:, j] - C[:t].T @ C[:t, j]
        r[j] = v[j] - MIN_NOISE  # the latent variance: the observation's own noise is s2
        sd = math.sqrt(max(r[j], 0.0) + s2)
        c = r / sd
        C[t] = c
        v = v - c * c
        mu = mu + c * (f - muj) / sd
        picked[j] = True
        fm = min(fm, f)
        out["history"].append((mu.copy(), v.copy()))
    out["idx"] = np.array(out["idx"], np.int64)
    out["ei"] = np.array(out["ei"])
    out["best"] = np.array(out["best"])
    out["mean"] = mu
    out["var"] = np.maximum(v, 0.0)
    return out


def bars(dtype):
    # (pick: EI of the device's pick against the step's maximum, relative to max(1, EI); values: relative to c or max(1, |.|))
    return (1e-12, 1e-8) if dtype == np.float64 else (1e-5, 1e-4)


def replay(fk, Xs, k, fmin, lie, dtype):
    """The device's k picks (fk.select_batch) replayed through select on the engine's own mean and Sigma (predict_cov at
    jitter 0), against bars(dtype).  Returns (idx, ei, mean, var, (pick gap, ei, mean, var deviations))."""
    pick_bar, bar = bars(dtype)
    c = fk.amplitude
    idx, ei, mean, var = fk.select_batch(Xs, k, fmin, lie=lie)
    assert idx.dtype == np.int64 and idx.shape == (k,) and ei.shape == (k,)
    assert mean.dtype == dtype and var.dtype == dtype and mean.shape == (len(Xs),)
    assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < len(Xs)
    mean0, cov = fk.predict_cov(Xs)
    r = select(mean0, cov, fk.noise, fmin, k, lie=lie, picks=idx)
    gap = float(np.max((r["best"] - r["ei"]) / np.maximum(1.0, r["best"])))
    dei = float(np.abs(ei - r["ei"]).max()) / max(1.0, float(np.abs(r["ei"]).max()))
    dmean = float(np.abs(mean.astype(np.float64) - r["mean"]).max()) / max(1.0, float(np.abs(r["mean"]).max()))
    dvar = float(np.abs(var.astype(np.float64) - r["var"]).max()) / c
    assert gap <= pick_bar, gap
    assert dei <= bar and dmean <= bar and dvar <= bar, (dei, dmean, dvar)
    return idx, ei, mean, var, (gap, dei, dmean, dvar)
