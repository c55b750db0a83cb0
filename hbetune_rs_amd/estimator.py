"""Host-side mirror of the reference's GP adapter: `EstimatorGPR` / `SurrogateModelGPR` (src/core/gpr.rs:54-63, 215-450)
over the C ABI, with the O(n) scalar pieces the adapter keeps on the host: y-normalisation (src/core/ynormalize.rs),
the amplitude heuristic (gpr.rs:429-450), expected improvement (src/core/acquisition.rs:141-171) and summary statistics
(gpr.rs:114-177).  Same names, argument meaning and error behaviour as the traits in src/core/surrogate_model.rs:6-65,
so that tests read like tests/gpr_tests.rs.  All O(n^2 d)/O(n^3) work happens in libhbegp.so on the GPU.
"""
import math

import numpy as np

from . import gpr
from .synth import splitmix64_uniform_fast

FUDGE_MIN = 0.05  # ynormalize.rs:5


class BoundsError(ValueError):
    """bounded_value.rs:73-77 / gpr.rs:453-473"""

    def __init__(self, what, value, lo, hi):
        super().__init__(f"{what} {value} violated bounds [{lo}, {hi}] during model fitting")
        self.value, self.min, self.max = value, lo, hi


def _bounded(what, value, lo, hi):  # BoundedValue::new bounded_value.rs:14-20
    if not (lo <= value <= hi):
        raise BoundsError(what, value, lo, hi)
    return value


class YNormalize:
    """ynormalize.rs:7-288: linear or logarithmic projection of y into the normalised range and back."""

    def __init__(self, amplitude, expected, projection):
        self.amplitude, self.expected, self.projection = amplitude, expected, projection

    @staticmethod
    def new_project_into_normalized(y, projection="linear", known_optimum=None):  # :162-195
        y = np.asarray(y)
        dt = y.dtype.type
        minimum = dt(0) if projection == "linear" else dt(1)
        expected = y.min() - minimum  # guess_min :291-303
        if known_optimum is not None and dt(known_optimum) < expected:
            expected = dt(known_optimum)
        if projection == "linear":
            yn = y - expected
            amp = yn.mean()
            amp = amp if amp > 0 else dt(1)  # guess_amplitude :307-322
            return yn / amp + dt(FUDGE_MIN), YNormalize(amp, expected, projection)
        if projection == "logarithmic":
            yn = np.log(y - expected)
            amp = yn.mean()
            amp = amp if amp > 0 else dt(1)
            return yn / amp, YNormalize(amp, expected, projection)
        raise ValueError(projection)

    def project_into_normalized(self, y):  # :197-209
        y = np.asarray(y)
        if self.projection == "linear":
            return (y - self.expected) / self.amplitude + y.dtype.type(FUDGE_MIN)
        return np.log(y - self.expected) / self.amplitude

    def project_variance_into_normalized(self, y, y_variance):
        """The variance of a measured y (of a mean of replicates: the variance of that mean) in the normalised space, for
        FittedKernel's row_variance.  Linear: y_variance / amplitude^2, exact.  Logarithmic: first order (the delta method),
        y_variance times the squared derivative of the projection, 1 / ((y - expected) amplitude)^2.  Not in the reference."""
        y = np.asarray(y)
        var = np.asarray(y_variance, dtype=np.float64)
        if self.projection == "linear":
            return var / float(self.amplitude) ** 2
        return var / ((y.astype(np.float64) - float(self.expected)) * float(self.amplitude)) ** 2

    def project_location_from_normalized(self, y):  # :214-224
        y = np.asarray(y)
        if self.projection == "linear":
            return (y - y.dtype.type(FUDGE_MIN)) * self.amplitude + self.expected
        return np.exp(y * self.amplitude) + self.expected

    def project_mean_from_normalized(self, mean, variance):  # :226-245
        mean, variance = np.asarray(mean), np.asarray(variance)
        if self.projection == "linear":
            return (mean - mean.dtype.type(FUDGE_MIN)) * self.amplitude + self.expected
        return np.exp(mean * self.amplitude + variance * self.amplitude ** 2 / 2) + self.expected

    def project_std_from_normalized(self, mean, variance):  # :247-265
        mean, variance = np.asarray(mean), np.asarray(variance)
        if self.projection == "linear":
            return np.sqrt(variance) * self.amplitude
        mu, s2 = mean * self.amplitude, variance * self.amplitude ** 2
        return np.sqrt(np.exp(mu * 2 + s2) * (np.exp(s2) - 1))  # logwarp::project_variance_from :112-119

    def project_cv_from_normalized(self, mean, variance):  # :267-286
        mean, variance = np.asarray(mean), np.asarray(variance)
        if self.projection == "linear":
            return np.sqrt(variance) * self.amplitude / ((mean - mean.dtype.type(FUDGE_MIN)) * self.amplitude + self.expected)
        return np.sqrt(np.exp(variance * self.amplitude ** 2) - 1)


def aggregate_replicates(x, y):
    """Repeated measurements of the same configuration -> one row each: (x_unique [u, d] in order of first appearance, mean [u],
    variance of that mean [u] float64, count [u]).  A row seen k >= 2 times: its unbiased sample variance / k.  A row seen once
    has no variance of its own: it gets the pooled variance of the replicated rows (their within-row sums of squares over their
    degrees of freedom; 0 where no row is replicated).  The result feeds EstimatorGPR.estimate(..., y_variance=): n and the n^3
    work then follow the number of configurations, not of measurements."""
    x = np.asarray(x)
    y = np.asarray(y)
    assert x.ndim == 2 and y.shape == (x.shape[0],)
    _, first, inverse, counts = np.unique(x, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inverse = np.asarray(inverse).reshape(-1)
    order = np.argsort(first, kind="stable")  # np.unique sorts the rows: back to the order of first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    group = rank[inverse]
    u = len(order)
    counts = counts[order]
    y64 = y.astype(np.float64)
    mean = np.bincount(group, weights=y64, minlength=u) / counts
    ss = np.bincount(group, weights=(y64 - mean[group]) ** 2, minlength=u)
    dof = counts - 1
    pooled = ss[dof > 0].sum() / dof[dof > 0].sum() if (dof > 0).any() else 0.0
    var = np.where(dof > 0, ss / np.maximum(dof, 1) / counts, pooled)
    return x[first[order]], mean.astype(y.dtype), var, counts


def replicate_groups(x, max_size=64):
    """Group labels for leave-group-out cross-validation (EstimatorGPR.estimate(..., groups=), SurrogateModelGPR.lgo_a): rows with
    equal x share a label, int32 [n], dense 0 .. L - 1 in order of first appearance.  A set of more than max_size equal rows
    (the engine holds out at most 64 rows together) is split, in row order, into consecutive labels of max_size rows each."""
    x = np.asarray(x)
    assert x.ndim == 2 and max_size >= 1
    _, inverse = np.unique(x, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    labels = np.empty(x.shape[0], dtype=np.int32)
    current, held, nxt = {}, {}, 0
    for i, u in enumerate(inverse.tolist()):
        if u not in current or held[u] == max_size:
            current[u], held[u] = nxt, 0
            nxt += 1
        labels[i] = current[u]
        held[u] += 1
    return labels


def _norm_cdf(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def _norm_pdf(z):
    return math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _norm_inverse_cdf(p, mu, sigma):
    from scipy.special import ndtri

    return mu + sigma * float(ndtri(p))


def expected_improvement_with_gradient(mean, var, dmean, dvar, fmin):
    """EI of `expected_improvement` at (mean, sqrt(var)) and its gradient from those of the mean and the variance:
    dEI = -Phi(z) dmean + phi(z) dstd with dstd = dvar / (2 std); where std is 0 (the ulps_eq branch) -dmean if mean < fmin,
    else 0.  The same arithmetic as hbegp_maximize_ei_* (hbegp.cpp, ei_with_gradient)."""
    std = math.sqrt(var)
    dmean = np.asarray(dmean, dtype=np.float64)
    if std <= 0.0 or abs(std) <= np.finfo(float).eps:
        return expected_improvement(mean, std, fmin), (-dmean if mean < fmin else np.zeros_like(dmean))
    z = -(mean - fmin) / std
    cdf, pdf = _norm_cdf(z), _norm_pdf(z)
    return expected_improvement(mean, std, fmin), -cdf * dmean + pdf * (np.asarray(dvar, dtype=np.float64) / (2.0 * std))


def expected_improvement(mean, std, fmin):
    """acquisition.rs:141-171"""
    assert math.isfinite(mean) and math.isfinite(std) and math.isfinite(fmin)
    if std <= 0.0 or abs(std) <= np.finfo(float).eps:  # ulps_eq!(std, 0.0): |std| <= f64::EPSILON (acquisition.rs:148)
        return -(mean - fmin) if mean < fmin else 0.0
    z = -(mean - fmin) / std
    ei = -(mean - fmin) * _norm_cdf(z) + std * _norm_pdf(z)
    assert math.isfinite(ei) and ei >= -1e-300
    return max(ei, 0.0)


class SummaryStatistics:
    """surrogate_model.rs:67-135"""

    def __init__(self, mean, std, cv, quartiles):
        self._mean, self._std, self._cv = mean, std, cv
        self.q1, self.q2, self.q3 = quartiles

    def mean(self):
        return self._mean

    def std(self):
        return self._std

    def cv(self):
        return self._cv

    def median(self):
        return self.q2

    def iqr(self):
        return self.q3 - self.q1


def estimate_amplitude(y, bounds=None):
    """gpr.rs:429-450 -> (start, lo, hi)"""
    y = np.asarray(y, dtype=np.float64)
    if bounds is None:
        hi = float((y ** 2).sum())
        ys = np.sort(y)
        q = float(ys[int(math.floor((len(ys) - 1) * 0.1))])  # Quantile1dExt::quantile_mut(0.1, Lower)
        lo = q * q * len(y)
        assert lo >= 0.0
        lo = lo if lo > 2e-5 else 2e-5
        lo, hi = lo / 2.0, hi * 2.0
    else:
        lo, hi = bounds
    start = math.exp((math.log(lo) + math.log(hi)) / 2.0)
    return _bounded("amplitude", start, lo, hi), lo, hi


class RNG:
    """Stand-in for the caller's RNG (random.rs:9-52): only `uniform` is needed by the fit (gradmin.rs:22-24)."""

    def __init__(self, seed):
        self.seed, self.count = int(seed), 0

    @staticmethod
    def new_with_seed(seed):
        return RNG(seed)

    def fork_random_state(self):
        self.count += 1
        return RNG(self.seed * 1000003 + self.count)

    def uniform(self, lo, hi, size):
        u = splitmix64_uniform_fast(self.seed + 7919 * self.count, size)
        self.count += 1
        return lo + (hi - lo) * u

    def standard_normal(self, size):
        """Deterministic standard normals (Box-Muller over the same SplitMix64 stream as `uniform`), shape `size`.  The first
        uniform of every pair enters as 1 - u, in (0, 1]: the logarithm never sees 0, so no draw is infinite."""
        shape = (size,) if np.isscalar(size) else tuple(size)
        count = int(np.prod(shape, dtype=np.int64))
        pairs = (count + 1) // 2
        u = splitmix64_uniform_fast(self.seed + 7919 * self.count, 2 * pairs)
        self.count += 1
        r = np.sqrt(-2.0 * np.log(1.0 - u[0::2]))
        t = 2.0 * math.pi * u[1::2]
        z = np.empty(2 * pairs)
        z[0::2] = r * np.cos(t)
        z[1::2] = r * np.sin(t)
        return z[:count].reshape(shape)


class SurrogateModelGPR:
    """gpr.rs:54-63 + impl SurrogateModel (gpr.rs:71-213)."""

    def __init__(self, fitted, noise_bounds, amplitude_bounds, length_scale_bounds, y_norm, dtype):
        self.fitted = fitted  # gpr.FittedKernel: kernel parameters, alpha, k_inv on the device
        self.noise_bounds, self.amplitude_bounds, self.length_scale_bounds = noise_bounds, amplitude_bounds, length_scale_bounds
        self.y_norm = y_norm
        self.dtype = np.dtype(dtype)
        self.lml = fitted.lml

    def length_scales(self):  # gpr.rs:72-79
        return list(self.fitted.length_scale)

    def kernel(self):
        return dict(amplitude=self.fitted.amplitude, length_scale=self.fitted.length_scale, noise=self.fitted.noise)

    def predict_mean_a(self, x):  # gpr.rs:81-92
        y, _, _ = self.fitted.predict(np.asarray(x, dtype=self.dtype), want_variance=False)
        return self.y_norm.project_location_from_normalized(y)

    def predict_mean(self, x):  # surrogate_model.rs:42-45
        return self.predict_mean_a(np.asarray(x, dtype=self.dtype)[None, :])[0]

    def _predict_norm(self, x2d):
        m, v, n_warn = self.fitted.predict(np.asarray(x2d, dtype=self.dtype), want_variance=True)
        if n_warn:
            import sys

            print("Variances below 0 were predicted and will be corrected", file=sys.stderr)  # predict.rs:39-48
        return m, v

    def predict_confidence_bound(self, x, cb):  # gpr.rs:94-112
        m, v = self._predict_norm(np.asarray(x, dtype=self.dtype)[None, :])
        return self.y_norm.project_location_from_normalized(m + np.sqrt(v) * self.dtype.type(cb))[0]

    def predict_statistics(self, x):  # gpr.rs:114-177
        m, v = self._predict_norm(np.asarray(x, dtype=self.dtype)[None, :])
        std_n, mean_n = float(np.sqrt(v[0])), float(m[0])
        mean = self.y_norm.project_mean_from_normalized(m, v)[0]
        std = self.y_norm.project_std_from_normalized(m, v)[0]
        cv = self.y_norm.project_cv_from_normalized(m, v)[0]
        if abs(std_n) <= np.finfo(float).eps:  # abs_diff_eq!(std, 0.0): |std| <= f64::EPSILON (gpr.rs:133)
            qn = np.array([mean_n] * 3, dtype=self.dtype)
        else:
            qn = np.array([_norm_inverse_cdf(p, mean_n, std_n) for p in (0.25, 0.5, 0.75)], dtype=self.dtype)
        q = self.y_norm.project_location_from_normalized(qn)
        return SummaryStatistics(mean, std, cv, (q[0], q[1], q[2]))

    def predict_statistics_a(self, x):
        """predict_statistics at every row of x [m, d]: ONE predict for all rows, the quartiles as mu + z_p sigma on the host.
        Returns a list of m SummaryStatistics, row by row the numbers the scalar method gives."""
        from scipy.special import ndtri

        m, v = self._predict_norm(np.asarray(x, dtype=self.dtype).reshape(-1, self.fitted.d))
        mean = self.y_norm.project_mean_from_normalized(m, v)
        std = self.y_norm.project_std_from_normalized(m, v)
        cv = self.y_norm.project_cv_from_normalized(m, v)
        mean_n, std_n = m.astype(np.float64), np.sqrt(v).astype(np.float64)
        z = np.array([float(ndtri(p)) for p in (0.25, 0.5, 0.75)])
        qn = mean_n[:, None] + std_n[:, None] * z[None, :]
        qn = np.where((np.abs(std_n) <= np.finfo(float).eps)[:, None], mean_n[:, None], qn).astype(self.dtype)
        q = self.y_norm.project_location_from_normalized(qn)
        return [SummaryStatistics(mean[i], std[i], cv[i], (q[i, 0], q[i, 1], q[i, 2])) for i in range(len(m))]

    def predict_mean_ei_a(self, x, fmin):  # gpr.rs:179-212
        m, v = self._predict_norm(x)
        fmin_n = float(self.y_norm.project_into_normalized(np.array([fmin], dtype=self.dtype))[0])
        ei = np.array([expected_improvement(float(mi), float(math.sqrt(vi)), fmin_n) for mi, vi in zip(m, v)], dtype=self.dtype)
        return self.y_norm.project_location_from_normalized(m), ei

    # Gradients w.r.t. the features (opt-in; nothing the estimator suggests by default uses them).
    def predict_mean_grad_a(self, x):
        """projected mean and its gradient [m, d] (chain rule through project_location_from_normalized)."""
        m, _, dm, _, _ = self.fitted.predict_with_gradient(np.asarray(x, dtype=self.dtype), want_variance=False)
        amp = self.y_norm.amplitude
        if self.y_norm.projection == "linear":
            scale = np.full(m.shape, amp, dtype=self.dtype)
        else:
            scale = amp * np.exp(m * amp)
        return self.y_norm.project_location_from_normalized(m), dm * scale[:, None]

    def _fmin_normalized(self, fmin):
        return float(self.y_norm.project_into_normalized(np.array([fmin], dtype=self.dtype))[0])

    def predict_mean_ei_grad_a(self, x, fmin):
        """predict_mean_ei_a plus dEI/dx [m, d] (EI in normalised space, as predict_mean_ei_a computes it)."""
        m, v, dm, dv, n_warn = self.fitted.predict_with_gradient(np.asarray(x, dtype=self.dtype), want_variance=True)
        if n_warn:
            import sys

            print("Variances below 0 were predicted and will be corrected", file=sys.stderr)  # predict.rs:39-48
        fmin_n = self._fmin_normalized(fmin)
        pairs = [expected_improvement_with_gradient(float(mi), float(vi), dmi, dvi, fmin_n) for mi, vi, dmi, dvi in zip(m, v, dm, dv)]
        ei = np.array([p[0] for p in pairs], dtype=self.dtype)
        dei = np.array([p[1] for p in pairs], dtype=self.dtype).reshape(len(m), -1)
        return self.y_norm.project_location_from_normalized(m), ei, dei

    def maximize_ei(self, starts, bounds, fmin, maxeval=150):
        """Bounded L-BFGS ascent of EI from every row of `starts` (the box: `bounds` = [(lo, hi)] per feature), all runs in
        lockstep on the device model.  fmin is projected into normalised space as predict_mean_ei_a does it.
        Returns (x[S, d], ei[S], nevals[S])."""
        lo = np.array([b[0] for b in bounds], dtype=np.float64)
        hi = np.array([b[1] for b in bounds], dtype=np.float64)
        return self.fitted.maximize_ei(np.asarray(starts, dtype=self.dtype), lo, hi, self._fmin_normalized(fmin), maxeval=maxeval)

    def maximize_log_ei(self, starts, bounds, fmin, maxeval=150):
        """maximize_ei on log EI (FittedKernel.maximize_log_ei): the runs move where EI itself underflows to 0.  Opt-in.
        Returns (x[S, d], log ei[S], nevals[S])."""
        lo = np.array([b[0] for b in bounds], dtype=np.float64)
        hi = np.array([b[1] for b in bounds], dtype=np.float64)
        return self.fitted.maximize_log_ei(np.asarray(starts, dtype=self.dtype), lo, hi, self._fmin_normalized(fmin), maxeval=maxeval)

    # Joint posterior draws (opt-in; nothing the estimator suggests by default uses them).
    def sample_a(self, x, n_samples, rng, jitter=0.0):
        """n_samples joint draws of the surrogate at the rows of x [m, d], projected like predict_mean_a: [n_samples, m].
        The normals come from rng.standard_normal; the projection is elementwise and monotone, so it is exact for draws."""
        x = np.asarray(x, dtype=self.dtype)
        z = rng.standard_normal((int(n_samples), x.shape[0])).astype(self.dtype)
        samples, _ = self.fitted.sample_posterior(x, z, jitter=jitter)
        return self.y_norm.project_location_from_normalized(samples)

    # Greedy batch selection by EI (opt-in; nothing the estimator suggests by default uses it).
    def select_batch_a(self, x, k, fmin, lie=None):
        """k rows of x [m, d] picked greedily by EI with fantasised observations (FittedKernel.select_batch).  fmin and the
        constant lie are in y units and projected like predict_mean_ei_a projects fmin.  Returns (idx[k], the projected means of
        the picks under the model before any fantasy, ei[k] in the normalised space)."""
        x = np.asarray(x, dtype=self.dtype)
        lie_n = None if lie is None else self._fmin_normalized(lie)
        idx, ei, _, _ = self.fitted.select_batch(x, k, self._fmin_normalized(fmin), lie=lie_n)
        means, _, _ = self.fitted.predict(x[idx], want_variance=False) if len(idx) else (np.zeros(0, self.dtype), None, 0)
        return idx, self.y_norm.project_location_from_normalized(means), ei

    # Knowledge gradient over a candidate set (opt-in; nothing the estimator suggests by default uses it).
    def knowledge_gradient_a(self, x, n_candidates=None):
        """Knowledge gradient of one more noisy observation at each of the first n_candidates rows of x [m, d] (all by default),
        the minimum of the posterior mean taken over all m rows (FittedKernel.knowledge_gradient).  It needs no fmin.  KG is
        returned in the NORMALISED y space, as predict_mean_ei_a returns EI: no projection is applied (the y projection is
        monotone increasing, so the ranking of rows by mean is the projected one's, but a difference of means is not a
        difference in y units under the logarithmic projection).  Returns (kg[n_candidates] float64, best): best the last index of
        the maximum of kg, -1 without candidates."""
        kg, best, _ = self.fitted.knowledge_gradient(np.asarray(x, dtype=self.dtype), n_candidates=n_candidates)
        return kg, best

    def best_by_mean_a(self, x):
        """The row of x [m, d] with the lowest posterior mean (ties to the lowest index) and that mean projected like
        predict_mean_a: what a tuner of a noisy objective should report instead of its best observation."""
        _, _, imin, mean, _ = self.fitted.knowledge_gradient(np.asarray(x, dtype=self.dtype), n_candidates=0, want_posterior=True)
        return imin, self.y_norm.project_location_from_normalized(mean[imin:imin + 1])[0]

    # Noisy expected improvement over a candidate set (opt-in; nothing the estimator suggests by default uses it).
    def noisy_ei_a(self, x, n_samples, rng, baseline=None, jitter=0.0, max_baseline=None):
        """Noisy EI of the rows of x [mc, d] (FittedKernel.noisy_ei): EI averaged over n_samples joint posterior draws of the latent
        function at the baseline, each with its own incumbent, so no fmin is needed.  The baseline defaults to the model's training
        rows; with max_baseline only its rows of lowest posterior mean are kept (deterministic: no random numbers).  z
        [n_samples, mb] comes from rng.standard_normal.  NEI is returned in the NORMALISED y space, as knowledge_gradient_a returns
        KG.  Returns (nei[mc] float64, best): best the last index of the maximum of nei, -1 without candidates."""
        b = _nei_baseline(self.fitted, baseline, max_baseline, self.dtype)
        z = rng.standard_normal((int(n_samples), b.shape[0])).astype(self.dtype)
        return self.fitted.noisy_ei(b, np.asarray(x, dtype=self.dtype), z, jitter=jitter)

    # Batch expected improvement by Monte Carlo (opt-in; nothing the estimator suggests by default uses it).
    def qei_a(self, x, fmin, n_samples, rng, jitter=0.0, want_grad=True):
        """q-EI of batches x [B, q, d] (or [q, d]) in the normalised space (FittedKernel.qei), fmin projected as predict_mean_ei_a
        projects it, z [n_samples, q] from rng.standard_normal.  Returns (qei[B], grad[B, q, d] or None, info[B])."""
        x = np.asarray(x, dtype=self.dtype)
        q = x.shape[-2]
        z = rng.standard_normal((int(n_samples), q)).astype(self.dtype)
        return self.fitted.qei(x, z, self._fmin_normalized(fmin), jitter=jitter, want_grad=want_grad)

    def maximize_qei(self, starts, bounds, fmin, n_samples, rng, jitter=0.0, maxeval=150):
        """Bounded L-BFGS ascents of q-EI from every batch of `starts` [R, q, d] (the box: `bounds` = [(lo, hi)] per feature), all
        runs in lockstep with one z [n_samples, q] from rng.standard_normal.  Returns (x[R, q, d], qei[R], nevals[R])."""
        starts = np.asarray(starts, dtype=self.dtype)
        lo = np.array([b[0] for b in bounds], dtype=np.float64)
        hi = np.array([b[1] for b in bounds], dtype=np.float64)
        z = rng.standard_normal((int(n_samples), starts.shape[-2])).astype(self.dtype)
        return self.fitted.maximize_qei(starts, lo, hi, z, self._fmin_normalized(fmin), jitter=jitter, maxeval=maxeval)

    # Posterior sample paths (opt-in; nothing the estimator suggests by default uses them).
    def sample_paths_a(self, n_paths, n_features, rng, noise_draw=True):
        """n_paths posterior draws of the surrogate that are functions (FittedKernel.sample_paths), in the normalised y space:
        random Fourier frequencies from gpr.draw_spectral, weights and, with noise_draw, the noise draw from rng.standard_normal.
        Project values with y_norm.project_location_from_normalized as sample_a does; the projection is monotone increasing, so
        a path's minimiser is the projected path's."""
        fk = self.fitted
        omega0, phase = gpr.draw_spectral(fk.nu, int(n_features), fk.d, rng)
        w = rng.standard_normal((int(n_paths), int(n_features)))
        eps = rng.standard_normal((int(n_paths), fk.n)) if noise_draw else None
        return fk.sample_paths(omega0, phase, w, eps)

    # Max-value entropy search (opt-in; nothing the estimator suggests by default uses it).
    def sample_min_values(self, n_samples, rng, bounds, n_features=1024, n_restarts=8, maxeval=150, grid=None, starts=None):
        """n_samples draws y* of the VALUE of the surrogate's global minimum over the box `bounds` = [(lo, hi)] per feature, in the
        NORMALISED y space (what mes_a and maximize_mes take): float64 [n_samples].  Default: n_samples posterior sample paths
        (sample_paths_a with n_features random features) and each path's lowest value over n_restarts bounded L-BFGS descents
        (PosteriorPaths.minimize's f_best) from `starts` [n_samples, n_restarts, d] or [n_restarts, d] (default: uniform in the
        box from rng, drawn before the paths).  With `grid` [m, d]: the row minima of n_samples joint posterior draws at the grid
        (FittedKernel.sample_posterior with z from rng.standard_normal); bounds is then not used."""
        S = int(n_samples)
        if grid is not None:
            g = np.asarray(grid, dtype=self.dtype)
            z = rng.standard_normal((S, g.shape[0])).astype(self.dtype)
            samples, _ = self.fitted.sample_posterior(g, z)
            return np.asarray(samples, dtype=np.float64).min(axis=1)
        lo = np.array([b[0] for b in bounds], dtype=np.float64)
        hi = np.array([b[1] for b in bounds], dtype=np.float64)
        if starts is None:
            u = np.asarray(rng.uniform(0.0, 1.0, S * int(n_restarts) * lo.shape[0]), dtype=np.float64)
            starts = lo + (hi - lo) * u.reshape(S, int(n_restarts), lo.shape[0])
        st = _starts_in_box(starts, lo, hi, self.dtype)
        paths = self.sample_paths_a(S, n_features, rng)
        try:
            _, f_best, _ = paths.minimize(st, lo, hi, maxeval=maxeval)
        finally:
            paths.release()
        return np.asarray(f_best, dtype=np.float64)

    def mes_a(self, x, ystar):
        """Max-value entropy search at the rows of x [m, d] (FittedKernel.mes) given sampled minimum values ystar in the normalised
        y space (sample_min_values).  MES is an entropy difference in nats: no projection applies.  Returns (mes[m] float64,
        best): best the last index of the maximum, -1 without rows."""
        return self.fitted.mes(np.asarray(x, dtype=self.dtype), ystar)

    def maximize_mes(self, starts, bounds, ystar, maxeval=150):
        """Bounded L-BFGS ascent of MES from every row of `starts` (the box: `bounds` = [(lo, hi)] per feature), all runs in
        lockstep on the device model (FittedKernel.maximize_mes).  Returns (x[R, d], mes[R], nevals[R])."""
        lo = np.array([b[0] for b in bounds], dtype=np.float64)
        hi = np.array([b[1] for b in bounds], dtype=np.float64)
        return self.fitted.maximize_mes(np.asarray(starts, dtype=self.dtype), lo, hi, ystar, maxeval=maxeval)

    def minimize_confidence_bound(self, starts, bounds, cb, maxeval=150):
        """Bounded L-BFGS descent of the confidence bound mean + cb * std from every row of `starts` (the box: `bounds` = [(lo, hi)]
        per feature), all runs in lockstep on the device model (FittedKernel.minimize_confidence_bound): the device alternative to
        the BOBYQA loop of the reference's suggest_optimum (minimize.rs:598-610).  The runs work on the NORMALISED bound:
        project_location_from_normalized is strictly increasing for the linear and for the logarithmic projection, so the point
        that minimises the normalised bound minimises predict_confidence_bound too.  Returns (x[S, d], bound[S], nevals[S]), the
        bound PROJECTED like predict_confidence_bound's (float64)."""
        lo = np.array([b[0] for b in bounds], dtype=np.float64)
        hi = np.array([b[1] for b in bounds], dtype=np.float64)
        x, val, nevals = self.fitted.minimize_confidence_bound(np.asarray(starts, dtype=self.dtype), lo, hi, float(cb), maxeval=maxeval)
        return x, self.y_norm.project_location_from_normalized(val), nevals

    # Sensitivity of the surrogate to its features (opt-in; nothing the estimator suggests by default uses it).
    def _uniform_rows(self, n_samples, rng, bounds):
        """[n_samples, d] uniform rows from rng.uniform in the unit box, or in `bounds` = [(lo, hi)] per feature."""
        d = self.fitted.d
        u = np.asarray(rng.uniform(0.0, 1.0, int(n_samples) * d), dtype=np.float64).reshape(int(n_samples), d)
        if bounds is not None:
            lo = np.array([b[0] for b in bounds], dtype=np.float64)
            hi = np.array([b[1] for b in bounds], dtype=np.float64)
            assert lo.shape == (d,) and hi.shape == (d,)
            u = lo + (hi - lo) * u
        return u.astype(self.dtype)

    def sobol_indices_a(self, n_samples, rng, bounds=None):
        """First-order and total Sobol indices of the surrogate's mean per feature (FittedKernel.sobol_indices): which parameters
        mattered, and whether through a main effect (first) or through interactions too (total - first).  The two pick-freeze
        sample matrices [n_samples, d] are drawn uniformly in the unit box, or in `bounds` = [(lo, hi)] per feature, from
        rng.uniform (A first, then B).  Under the linear y projection the indices are those of y itself, because a variance ratio
        is invariant under affine maps; under the logarithmic projection they are those of the normalised response (of
        log(y - expected)), not of y.  Returns (first[d], total[d]) float64."""
        A = self._uniform_rows(n_samples, rng, bounds)
        B = self._uniform_rows(n_samples, rng, bounds)
        first, total, _, _ = self.fitted.sobol_indices(A, B)
        return first, total

    def main_effects_a(self, n_samples, grid_size, rng, bounds=None):
        """Main-effect (partial dependence) curves of the surrogate's mean (FittedKernel.main_effects): per feature the mean
        prediction over n_samples uniform rows (unit box or `bounds`, from rng.uniform) with that feature set to each of
        grid_size midpoints of its range.  The averages are taken in the normalised space and projected like predict_mean_a:
        under the linear projection that is the average in y units, under the logarithmic one the projection of the average
        normalised response.  Returns (grid[d, grid_size], effect[d, grid_size]) float64, both in the caller's units."""
        d, G = self.fitted.d, int(grid_size)
        A = self._uniform_rows(n_samples, rng, bounds)
        lo = np.zeros(d) if bounds is None else np.array([b[0] for b in bounds], dtype=np.float64)
        hi = np.ones(d) if bounds is None else np.array([b[1] for b in bounds], dtype=np.float64)
        grid = lo[:, None] + (hi - lo)[:, None] * ((np.arange(G) + 0.5) / G)[None, :]
        effect = self.fitted.main_effects(A, grid.astype(self.dtype))
        return grid, self.y_norm.project_location_from_normalized(effect)

    # Leave-one-out diagnostics (opt-in; nothing the estimator suggests by default uses them).
    def loo_a(self):
        """Leave-one-out cross-validation of the surrogate on its own observations (FittedKernel.loo): per training row the
        prediction from all other rows, projected back like predict_mean_std_a -- (mean[n], std[n]) in y units -- and the
        standardised residuals (y_i - mu_i) / sqrt(var_i) in the normalised space (= alpha_i sqrt(var_i)), which a well
        specified model keeps near a standard normal.  var is the observation's: it includes the noise."""
        m, v, _, _ = self.fitted.loo()
        alpha, _ = self.fitted.arrays(want_kinv=False)
        resid = alpha * np.sqrt(v)
        return self.y_norm.project_mean_from_normalized(m, v), self.y_norm.project_std_from_normalized(m, v), resid

    def lgo_a(self, groups):
        """Leave-group-out cross-validation of the surrogate on its own observations (FittedKernel.lgo): per training row the
        prediction from all rows outside its group (`groups`: one int label per row, see replicate_groups), projected back
        like loo_a -- (mean[n], std[n]) in y units -- and the standardised residuals (y_i - mu_i) / sqrt(var_i) in the
        normalised space.  Where rows have twins, loo_a's residuals shrink towards zero and these do not."""
        m, v, _, _ = self.fitted.lgo(groups)
        resid = (np.asarray(self.fitted.y_train, dtype=np.float64) - m) / np.sqrt(v)
        return self.y_norm.project_mean_from_normalized(m, v), self.y_norm.project_std_from_normalized(m, v), resid

    # Batched forms of the scalar trait methods (the acquisition loops call these once per generation
    # instead of m single-point predicts, each of which reads all of K^-1).
    def predict_confidence_bound_a(self, x, cb):
        m, v = self._predict_norm(x)
        return self.y_norm.project_location_from_normalized(m + np.sqrt(v) * self.dtype.type(cb))

    def predict_mean_std_a(self, x):
        m, v = self._predict_norm(x)
        return self.y_norm.project_mean_from_normalized(m, v), self.y_norm.project_std_from_normalized(m, v)

    def predict_mean_ei(self, x, fmin):  # surrogate_model.rs:49-52
        mean, ei = self.predict_mean_ei_a(np.asarray(x, dtype=self.dtype)[None, :], fmin)
        return mean[0], ei[0]


def rank_parameters(model, n_samples, rng, bounds=None):
    """The features of `model` (a SurrogateModelGPR) ordered by their total Sobol index, the most influential first, ties to the
    lower index (SurrogateModelGPR.sobol_indices_a with n_samples rows per sample matrix).  Opt-in: nothing that is suggested by
    default changes.  Returns (order[d] int64, first[d], total[d])."""
    first, total = model.sobol_indices_a(n_samples, rng, bounds=bounds)
    order = np.argsort(-total, kind="stable").astype(np.int64)
    return order, first, total


def find_best_candidate_by_ei(candidates, model, fmin):
    """acquisition.rs:177-202 over a feature array: index, mean and EI of the candidate with maximal EI.
    One batched predict instead of a scalar `predict_mean_ei` per candidate.  Ties go to the LAST maximal element, as
    Rust's `Iterator::max_by` does; a NaN EI raises like the reference's panic."""
    means, eis = model.predict_mean_ei_a(np.asarray(candidates), fmin)
    return _pick(means, eis, _argmax_last(eis[None, :])[0])


def _argmax_last(eis2d):
    eis2d = np.asarray(eis2d)
    if np.isnan(eis2d).any():
        raise ValueError("EI should be comparable")  # acquisition.rs:193-195
    # index of the last maximum of every row
    rev = eis2d[:, ::-1]
    return eis2d.shape[1] - 1 - np.argmax(rev, axis=1)


def _pick(means, eis, i):
    return int(i), means[i], eis[i]


def acquire_by_mutation(candidates, model, fmin):
    """`MutationAcquisition::acquire` (acquisition.rs:86-116) after candidate generation: `candidates` is
    [n_parents, breadth, n_features] (the caller's `generate_nearby_samples`, projected into features); returns, per
    parent, the index of its best candidate and that candidate's mean and EI.  The whole generation is ONE batched
    predict instead of n_parents*breadth single-point predicts."""
    c = np.asarray(candidates)
    if c.ndim != 3:
        raise ValueError("candidates must be [n_parents, breadth, n_features]")
    npar, breadth, nf = c.shape
    means, eis = model.predict_mean_ei_a(c.reshape(npar * breadth, nf), fmin)
    means, eis = means.reshape(npar, breadth), eis.reshape(npar, breadth)
    idx = _argmax_last(eis)
    rows = np.arange(npar)
    return idx, means[rows, idx], eis[rows, idx]


def acquire_by_thompson(candidates, model, k, rng, jitter=0.0):
    """Batch Thompson sampling over a candidate set [m, n_features]: k joint posterior draws of the surrogate at the candidates
    (one device call), and for each draw the index of its minimum -- k indices, repeats allowed.  The y projection is monotone
    increasing, so the argmin of a normalised draw is the argmin of the projected one: only the k indices leave the device.
    Opt-in: nothing the estimator suggests by default calls it."""
    c = np.asarray(candidates, dtype=model.dtype)
    if c.ndim != 2:
        raise ValueError("candidates must be [m, n_features]")
    z = rng.standard_normal((int(k), c.shape[0])).astype(model.dtype)
    _, argmin = model.fitted.sample_posterior(c, z, jitter=jitter, want_samples=False)
    return np.asarray(argmin, dtype=np.int64)


def acquire_by_path_thompson(model, k, rng, bounds, n_features=1024, n_restarts=8, starts=None, maxeval=150, noise_draw=True):
    """Batch Thompson sampling without a candidate set: k posterior sample paths of the surrogate (sample_paths_a) and, for
    each, its minimiser in the box `bounds` = [(lo, hi)] per feature, found by n_restarts bounded L-BFGS descents per path from
    `starts` [k, n_restarts, d] (or [n_restarts, d], shared; default: uniform in the box from rng).  Returns x [k, n_features
    of the space], one point per path.  The y projection is monotone increasing, so the minimiser of a normalised path is the
    minimiser of the projected one.  Opt-in: the grid-free twin of acquire_by_thompson."""
    k = int(k)
    lo = np.array([b[0] for b in bounds], dtype=np.float64)
    hi = np.array([b[1] for b in bounds], dtype=np.float64)
    d = lo.shape[0]
    if starts is None:
        u = np.asarray(rng.uniform(0.0, 1.0, k * int(n_restarts) * d), dtype=np.float64).reshape(k, int(n_restarts), d)
        starts = lo + (hi - lo) * u
    paths = model.sample_paths_a(k, n_features, rng, noise_draw=noise_draw)
    try:
        x, _, _ = paths.minimize(_starts_in_box(starts, lo, hi, model.dtype), lo, hi, maxeval=maxeval)
    finally:
        paths.release()
    return x


def _starts_in_box(starts, lo, hi, dtype):
    """`starts` in the model's element type, rounded into the box [lo, hi] where the cast left it."""
    st = np.asarray(starts, dtype=dtype)
    st = np.where(st.astype(np.float64) > hi, np.nextafter(st, st.dtype.type(-np.inf)), st)
    return np.where(st.astype(np.float64) < lo, np.nextafter(st, st.dtype.type(np.inf)), st)


def acquire_by_max_value_entropy(model, k, rng, bounds, n_samples=64, n_starts=32, candidates=None, n_features=1024, n_restarts=8,
                                 maxeval=150, grid=None, starts=None):
    """Batch acquisition by max-value entropy search (Wang & Jegelka 2017): n_samples draws of the value of the global minimum
    over the box (model.sample_min_values: sample paths, or joint draws at `grid`), then the points where observing tells most
    about that value.  With `candidates` [m, n_features]: (idx[k] int64, mes[k]), the k rows of largest MES (model.mes_a), ties
    to the LAST index as find_best_candidate_by_ei breaks them; a NaN MES raises.  Without: (x[<= k, d], mes[<= k]), the best
    distinct end points of n_starts bounded L-BFGS ascents of MES (model.maximize_mes) from `starts` [n_starts, d] (default:
    uniform in the box from rng, drawn after the minimum values), best first; fewer than k rows only where fewer runs ended at
    distinct points.  The k points are chosen under ONE posterior: there is no fantasy between picks (joint MES is out of
    scope).  Opt-in: nothing the estimator suggests by default calls it."""
    k = int(k)
    ystar = model.sample_min_values(n_samples, rng, bounds, n_features=n_features, n_restarts=n_restarts, maxeval=maxeval, grid=grid)
    if candidates is not None:
        c = np.asarray(candidates, dtype=model.dtype)
        if c.ndim != 2:
            raise ValueError("candidates must be [m, n_features]")
        if not 0 <= k <= c.shape[0]:
            raise ValueError("k must lie in [0, m]")
        val, _ = model.mes_a(c, ystar)
        if np.isnan(val).any():
            raise ValueError("MES should be comparable")
        idx = np.lexsort((np.arange(len(val)), val))[::-1][:k].astype(np.int64)  # descending MES, the later index first among equals
        return idx, val[idx]
    lo = np.array([b[0] for b in bounds], dtype=np.float64)
    hi = np.array([b[1] for b in bounds], dtype=np.float64)
    if starts is None:
        u = np.asarray(rng.uniform(0.0, 1.0, int(n_starts) * lo.shape[0]), dtype=np.float64).reshape(int(n_starts), lo.shape[0])
        starts = lo + (hi - lo) * u
    x, val, _ = model.maximize_mes(_starts_in_box(starts, lo, hi, model.dtype), bounds, ystar, maxeval=maxeval)
    picks = []
    for r in np.lexsort((np.arange(len(val)), val))[::-1]:
        if len(picks) < k and not any((x[r] == x[p]).all() for p in picks):
            picks.append(int(r))
    return x[picks], val[picks]


def acquire_by_batch_ei(candidates, model, k, fmin, lie=None):
    """Deterministic batch acquisition over a candidate set [m, n_features]: k distinct candidates picked greedily by EI, the
    surrogate conditioned after every pick on a fantasy observation there -- its predicted mean (kriging believer) or the
    constant `lie` (constant liar, y units) -- so that later picks move away from earlier ones.  One device call; k = 1 is
    find_best_candidate_by_ei.  Returns (idx[k], projected means of the picks, ei[k]).  Opt-in: the twin of
    acquire_by_thompson."""
    c = np.asarray(candidates, dtype=model.dtype)
    if c.ndim != 2:
        raise ValueError("candidates must be [m, n_features]")
    return model.select_batch_a(c, int(k), fmin, lie=lie)


def acquire_by_knowledge_gradient(candidates, model, k, n_candidates=None, ctx=None):
    """Batch acquisition for a noisy objective by the knowledge gradient over a candidate set [m, n_features]: k distinct rows among
    the first n_candidates (all by default), each the row where one more noisy observation is expected to lower the minimum of the
    posterior mean over all m rows the most (FittedKernel.knowledge_gradient: closed form, no fmin, no random numbers).  After a
    pick the surrogate is conditioned on the kriging-believer fantasy (x_pick, its posterior mean) through extend_with at the same
    theta, and rows already picked leave the places to sample but stay in the minimum.  A composition of existing calls: k
    knowledge-gradient calls and k - 1 extends; k = 1 is knowledge_gradient_a's best.  Returns (idx[k] int64, the projected means
    of the picks at the time they were picked, kg[k] in the normalised space).  Opt-in: nothing the estimator suggests by default
    calls it."""
    c = np.asarray(candidates, dtype=model.dtype)
    if c.ndim != 2:
        raise ValueError("candidates must be [m, n_features]")
    m = c.shape[0]
    mc = m if n_candidates is None else int(n_candidates)
    k = int(k)
    if not 0 <= mc <= m:
        raise ValueError("n_candidates must lie in [0, number of rows]")
    if not 0 <= k <= mc:
        raise ValueError("k must lie in [0, n_candidates]")
    fk = model.fitted
    X, y = fk.x_train, fk.y_train
    if k > 1 and (X is None or y is None):
        raise ValueError("the model does not hold its training rows: it cannot be conditioned on a fantasy")
    avail = list(range(mc))
    rest = list(range(mc, m))
    idx, means, kgs = [], [], []
    try:
        for t in range(k):
            order = avail + idx + rest  # the places to sample first; every row takes part in the minimum
            kg, best, _, mean, _ = fk.knowledge_gradient(c[order], n_candidates=len(avail), want_posterior=True)
            j = avail.pop(best)
            idx.append(j)
            means.append(mean[best])
            kgs.append(kg[best])
            if t + 1 < k:
                X = np.vstack([X, c[j:j + 1]])
                y = np.concatenate([y, mean[best:best + 1]])
                nxt = fk.extend_with(X, y, ctx=ctx)
                if fk is not model.fitted:
                    fk.release()
                fk = nxt
    finally:
        if fk is not model.fitted:
            fk.release()
    means = np.array(means, dtype=model.dtype)
    return np.array(idx, dtype=np.int64), model.y_norm.project_location_from_normalized(means), np.array(kgs, dtype=np.float64)


def pareto_front(y2):
    """The non-dominated rows of y2 [N, 2] when both columns are minimised, sorted by the first column ascending (the second then
    descends strictly); duplicates appear once.  float64 [P, 2]."""
    y = np.asarray(y2, dtype=np.float64).reshape(-1, 2)
    y = y[np.lexsort((y[:, 1], y[:, 0]))]
    keep, bmin = [], math.inf
    for i in range(len(y)):
        if y[i, 1] < bmin:  # among equal first values the lowest second one comes first and dominates the others
            keep.append(i)
            bmin = y[i, 1]
    return y[keep]


def hypervolume_2d(front, ref):
    """The area that the points of front [..., P, 2] dominate inside the box below ref [2], both objectives minimised: a sweep
    over the points sorted by the first objective with the running minimum of the second.  Points need not be non-dominated, nor
    inside the box (those add nothing).  A leading shape is a batch of fronts: returns a float, or an array of that shape."""
    f = np.asarray(front, dtype=np.float64)
    r1, r2 = float(ref[0]), float(ref[1])
    if f.size == 0:
        return 0.0 if f.ndim <= 2 else np.zeros(f.shape[:-2])
    a = np.minimum(f[..., 0], r1)
    b = np.minimum(f[..., 1], r2)
    order = np.argsort(a, axis=-1, kind="stable")
    a = np.take_along_axis(a, order, axis=-1)
    b = np.minimum.accumulate(np.take_along_axis(b, order, axis=-1), axis=-1)
    nxt = np.concatenate([a[..., 1:], np.full(a.shape[:-1] + (1,), r1)], axis=-1)
    hv = ((nxt - a) * (r2 - b)).sum(axis=-1)
    return float(hv) if np.ndim(hv) == 0 else hv


def default_reference_point(front):
    """The reference point used where none is given: per objective the worst value of front [P >= 1, 2] plus 10 % of the front's
    range in that objective; where the range is 0 (a one-point front) plus 10 % of max(1, |value|)."""
    f = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    if len(f) < 1:
        raise ValueError("an empty front has no default reference point")
    worst, span = f.max(axis=0), f.max(axis=0) - f.min(axis=0)
    return worst + 0.1 * np.where(span > 0, span, np.maximum(1.0, np.abs(worst)))


def _ehvi_normalized(models, front, ref):
    """front [P, 2] and ref [2] in y units -> each column through that model's YNormalize (float64).  The projections are monotone
    increasing, so dominance, the front and the inside of the box are preserved."""
    if len(models) != 2:
        raise ValueError("EHVI takes exactly two models")
    f = np.asarray(front if front is not None else [], dtype=np.float64).reshape(-1, 2)
    r = np.asarray(ref, dtype=np.float64).reshape(2)
    fn = np.stack([np.asarray(mo.y_norm.project_into_normalized(f[:, k]), dtype=np.float64) for k, mo in enumerate(models)], axis=1)
    rn = np.array([float(mo.y_norm.project_into_normalized(r[k:k + 1])[0]) for k, mo in enumerate(models)])
    return fn, rn


# Two-objective expected hypervolume improvement (opt-in; nothing the estimator suggests by default uses it).
def ehvi_a(models, x, front, ref):
    """EHVI of the rows of x [m, d] under two SurrogateModelGPRs (objective 0, objective 1), both minimised and taken as
    independent (gpr.ehvi).  front [P, 2] and ref [2] are in y units; each column goes through that model's y projection.  The
    AREA is measured in the normalised units of the two models, as knowledge_gradient_a returns KG: under the logarithmic
    projection it is not an area in y units, but the front, the box and the ranking of dominance are those of the y units.
    Returns (ehvi[m] float64, best): best the last index of the maximum, -1 without rows."""
    fn, rn = _ehvi_normalized(models, front, ref)
    return gpr.ehvi([mo.fitted for mo in models], np.asarray(x, dtype=models[0].dtype), fn, rn)


def maximize_ehvi(models, starts, bounds, front, ref, maxeval=150):
    """Bounded L-BFGS ascents of ehvi_a from every row of `starts` (the box: `bounds` = [(lo, hi)] per feature), all runs in
    lockstep on the two device models (gpr.maximize_ehvi).  front and ref in y units.  Returns (x[S, d], ehvi[S], nevals[S])."""
    fn, rn = _ehvi_normalized(models, front, ref)
    return gpr.maximize_ehvi([mo.fitted for mo in models], np.asarray(starts, dtype=models[0].dtype), bounds, fn, rn, maxeval=maxeval)


def _ehvi_default_front(models):
    """pareto_front of the two models' training targets in y units; the models must have been trained on the very same rows."""
    fks = [mo.fitted for mo in models]
    xs = [fk.x_train for fk in fks]
    if any(x is None for x in xs) or any(fk.y_train is None for fk in fks):
        raise ValueError("the models do not hold their training rows: pass a front")
    if xs[0].shape != xs[1].shape or xs[0].tobytes() != xs[1].tobytes():
        raise ValueError("the models were not trained on the same rows: pass a front")
    y = [np.asarray(mo.y_norm.project_location_from_normalized(np.asarray(mo.fitted.y_train)), dtype=np.float64) for mo in models]
    return pareto_front(np.stack(y, axis=1))


def acquire_by_ehvi(candidates, models, k, front=None, ref=None, ctx=None):
    """Batch acquisition for two minimised objectives by the expected hypervolume improvement over a candidate set [m, n_features]:
    k distinct rows, each the row of largest EHVI (gpr.ehvi: closed form, no random numbers) under the two SurrogateModelGPRs
    `models`.  After a pick BOTH surrogates are conditioned on the kriging-believer fantasy (x_pick, that model's posterior mean)
    through extend_with at the same theta, as acquire_by_knowledge_gradient does, and the believed point joins the front.  front
    [P, 2] and ref [2] are in y units.  Without a front: pareto_front of the two models' training targets, which needs models
    trained on the very same rows (else ValueError).  Without a ref: default_reference_point of the front.  Returns (idx[k] int64,
    the projected means [k, 2] of the picks at the time they were picked, ehvi[k] and the believed hypervolume hv[k] after each
    pick, both in the normalised units of ehvi_a).  Opt-in: nothing the estimator suggests by default calls it."""
    if len(models) != 2:
        raise ValueError("EHVI takes exactly two models")
    dtype = models[0].dtype
    c = np.asarray(candidates, dtype=dtype)
    if c.ndim != 2:
        raise ValueError("candidates must be [m, n_features]")
    k = int(k)
    if not 0 <= k <= c.shape[0]:
        raise ValueError("k must lie in [0, number of rows]")
    if front is None:
        front = _ehvi_default_front(models)
    if ref is None:
        ref = default_reference_point(front)
    fn, rn = _ehvi_normalized(models, front, ref)
    fks = [mo.fitted for mo in models]
    data = [(fk.x_train, fk.y_train) for fk in fks]
    if k > 1 and any(X is None or y is None for X, y in data):
        raise ValueError("the models do not hold their training rows: they cannot be conditioned on a fantasy")
    avail = list(range(c.shape[0]))
    idx, means, vals, hvs = [], [], [], []
    try:
        for t in range(k):
            val, best, mean, _ = gpr.ehvi(fks, c[avail], fn, rn, want_posterior=True)
            idx.append(avail.pop(best))
            means.append(mean[best])
            vals.append(val[best])
            fn = np.vstack([fn, np.asarray(mean[best], dtype=np.float64)[None, :]])
            hvs.append(hypervolume_2d(fn, rn))
            if t + 1 < k:
                for o in range(2):
                    X, y = data[o]
                    data[o] = (np.vstack([X, c[idx[-1]:idx[-1] + 1]]), np.concatenate([y, mean[best, o:o + 1]]))
                    nxt = fks[o].extend_with(*data[o], ctx=ctx)
                    if fks[o] is not models[o].fitted:
                        fks[o].release()
                    fks[o] = nxt
    finally:
        for o in range(2):
            if fks[o] is not models[o].fitted:
                fks[o].release()
    means = np.array(means, dtype=dtype).reshape(-1, 2)
    proj = np.stack([models[o].y_norm.project_location_from_normalized(means[:, o]) for o in range(2)], axis=1)
    return np.array(idx, dtype=np.int64), proj, np.array(vals, dtype=np.float64), np.array(hvs, dtype=np.float64)


# Expected hypervolume improvement of two to four objectives (opt-in; nothing the estimator suggests by default uses it).
def pareto_front_nd(y):
    """The non-dominated rows of y [N, M] when every column is minimised, sorted lexicographically; duplicates appear once.  A row
    is dominated when another row is <= it in every column.  float64 [P, M]."""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 2:
        raise ValueError("y must be [N, M]")
    if len(y) == 0:
        return y.copy()
    y = np.unique(y, axis=0)  # sorted lexicographically: only an earlier row can dominate a later one
    keep = []
    for i in range(len(y)):
        if not any((y[j] <= y[i]).all() for j in keep):
            keep.append(i)
    return y[keep]


def hypervolume_nd(front, ref):
    """The volume that the points of front [..., P, M] dominate inside the box below ref [M], every objective minimised, exactly,
    by slicing: the points sorted by the last objective, each slice between two consecutive values has the depth of their
    difference and the (M - 1)-dimensional hypervolume of the points at or before it; M = 2 is hypervolume_2d, M = 1 the length
    below ref.  Points need not be non-dominated, nor inside the box.  A leading shape is a batch of fronts: returns a float, or an
    array of that shape."""
    f = np.asarray(front, dtype=np.float64)
    r = np.asarray(ref, dtype=np.float64).reshape(-1)
    M = len(r)
    if f.size == 0:
        return 0.0 if f.ndim <= 2 else np.zeros(f.shape[:-2])
    if f.shape[-1] != M:
        raise ValueError("front and ref differ in the number of objectives")
    if M == 1:
        hv = np.maximum(r[0] - f[..., 0].min(axis=-1), 0.0)
    elif M == 2:
        hv = hypervolume_2d(f, r)
    else:
        f = np.minimum(f, r)
        order = np.argsort(f[..., -1], axis=-1, kind="stable")
        f = np.take_along_axis(f, order[..., None], axis=-2)
        z = f[..., -1]
        depth = np.concatenate([z[..., 1:], np.full(z.shape[:-1] + (1,), r[-1])], axis=-1) - z
        hv = 0.0
        for i in range(f.shape[-2]):
            hv = hv + depth[..., i] * hypervolume_nd(f[..., :i + 1, :-1], r[:-1])
    return float(hv) if np.ndim(hv) == 0 else hv


def default_reference_point_nd(front):
    """default_reference_point's rule for front [P >= 1, M]: per objective the worst value plus 10 % of the front's range there;
    where the range is 0 plus 10 % of max(1, |value|)."""
    f = np.asarray(front, dtype=np.float64)
    if f.ndim != 2 or len(f) < 1:
        raise ValueError("an empty front has no default reference point")
    worst, span = f.max(axis=0), f.max(axis=0) - f.min(axis=0)
    return worst + 0.1 * np.where(span > 0, span, np.maximum(1.0, np.abs(worst)))


def _ehvi_nd_normalized(models, front, ref):
    """front [P, M] and ref [M] in y units -> each column through that model's YNormalize (float64), M = len(models) in 2 .. 4."""
    M = len(models)
    if not 2 <= M <= 4:
        raise ValueError("EHVI over boxes takes two, three or four models")
    f = np.asarray(front if front is not None else [], dtype=np.float64).reshape(-1, M)
    r = np.asarray(ref, dtype=np.float64).reshape(M)
    fn = np.stack([np.asarray(mo.y_norm.project_into_normalized(f[:, k]), dtype=np.float64) for k, mo in enumerate(models)], axis=1)
    rn = np.array([float(mo.y_norm.project_into_normalized(r[k:k + 1])[0]) for k, mo in enumerate(models)])
    return fn, rn


def ehvi_nd_a(models, x, front, ref):
    """EHVI of the rows of x [m, d] under two, three or four SurrogateModelGPRs (objective 0 first), all minimised and taken as
    independent (gpr.ehvi_nd).  front [P, M] and ref [M] are in y units; each column goes through that model's y projection, and
    the VOLUME is measured in the models' normalised units, as ehvi_a's area is.  Returns (ehvi[m] float64, best): best the last
    index of the maximum, -1 without rows."""
    fn, rn = _ehvi_nd_normalized(models, front, ref)
    return gpr.ehvi_nd([mo.fitted for mo in models], np.asarray(x, dtype=models[0].dtype), fn, rn)


def maximize_ehvi_nd(models, starts, bounds, front, ref, maxeval=150):
    """Bounded L-BFGS ascents of ehvi_nd_a from every row of `starts` (the box: `bounds` = [(lo, hi)] per feature), all runs in
    lockstep on the device models (gpr.maximize_ehvi_nd).  front and ref in y units.  Returns (x[S, d], ehvi[S], nevals[S])."""
    fn, rn = _ehvi_nd_normalized(models, front, ref)
    return gpr.maximize_ehvi_nd([mo.fitted for mo in models], np.asarray(starts, dtype=models[0].dtype), bounds, fn, rn, maxeval=maxeval)


def _ehvi_nd_default_front(models):
    """pareto_front_nd of the models' training targets in y units; the models must have been trained on the very same rows."""
    fks = [mo.fitted for mo in models]
    xs = [fk.x_train for fk in fks]
    if any(x is None for x in xs) or any(fk.y_train is None for fk in fks):
        raise ValueError("the models do not hold their training rows: pass a front")
    if any(x.shape != xs[0].shape or x.tobytes() != xs[0].tobytes() for x in xs[1:]):
        raise ValueError("the models were not trained on the same rows: pass a front")
    y = [np.asarray(mo.y_norm.project_location_from_normalized(np.asarray(mo.fitted.y_train)), dtype=np.float64) for mo in models]
    return pareto_front_nd(np.stack(y, axis=1))


def acquire_by_ehvi_nd(candidates, models, k, front=None, ref=None, ctx=None):
    """acquire_by_ehvi for two, three or four minimised objectives: k distinct rows of the candidate set [m, n_features], each the
    row of largest EHVI (gpr.ehvi_nd) under the SurrogateModelGPRs `models`.  After a pick ALL surrogates are conditioned on the
    kriging-believer fantasy (x_pick, that model's posterior mean) through extend_with at the same theta, and the believed point
    joins the front.  front [P, M] and ref [M] are in y units.  Without a front: pareto_front_nd of the models' training targets,
    which needs models trained on the very same rows (else ValueError).  Without a ref: default_reference_point_nd of the front.
    Returns (idx[k] int64, the projected means [k, M] of the picks at the time they were picked, ehvi[k] and the believed
    hypervolume hv[k] after each pick, both in the normalised units of ehvi_nd_a).  The models' own `fitted` handles are left as
    they were."""
    M = len(models)
    if not 2 <= M <= 4:
        raise ValueError("EHVI over boxes takes two, three or four models")
    dtype = models[0].dtype
    c = np.asarray(candidates, dtype=dtype)
    if c.ndim != 2:
        raise ValueError("candidates must be [m, n_features]")
    k = int(k)
    if not 0 <= k <= c.shape[0]:
        raise ValueError("k must lie in [0, number of rows]")
    if front is None:
        front = _ehvi_nd_default_front(models)
    if ref is None:
        ref = default_reference_point_nd(front)
    fn, rn = _ehvi_nd_normalized(models, front, ref)
    fks = [mo.fitted for mo in models]
    data = [(fk.x_train, fk.y_train) for fk in fks]
    if k > 1 and any(X is None or y is None for X, y in data):
        raise ValueError("the models do not hold their training rows: they cannot be conditioned on a fantasy")
    avail = list(range(c.shape[0]))
    idx, means, vals, hvs = [], [], [], []
    try:
        for t in range(k):
            val, best, mean, _ = gpr.ehvi_nd(fks, c[avail], fn, rn, want_posterior=True)
            idx.append(avail.pop(best))
            means.append(mean[best])
            vals.append(val[best])
            fn = np.vstack([fn, np.asarray(mean[best], dtype=np.float64)[None, :]])
            hvs.append(hypervolume_nd(fn, rn))
            if t + 1 < k:
                for o in range(M):
                    X, y = data[o]
                    data[o] = (np.vstack([X, c[idx[-1]:idx[-1] + 1]]), np.concatenate([y, mean[best, o:o + 1]]))
                    nxt = fks[o].extend_with(*data[o], ctx=ctx)
                    if fks[o] is not models[o].fitted:
                        fks[o].release()
                    fks[o] = nxt
    finally:
        for o in range(M):
            if fks[o] is not models[o].fitted:
                fks[o].release()
    means = np.array(means, dtype=dtype).reshape(-1, M)
    proj = np.stack([models[o].y_norm.project_location_from_normalized(means[:, o]) for o in range(M)], axis=1)
    return np.array(idx, dtype=np.int64), proj, np.array(vals, dtype=np.float64), np.array(hvs, dtype=np.float64)


# Constrained expected improvement (opt-in; nothing the estimator suggests by default uses it).
def feasible_fmin(y, g, limits):
    """The smallest objective y[i] among the rows whose constraint values all hold, g[i, k] <= limits[k] (a row exactly on a limit
    is feasible); math.inf when no row qualifies -- the "no feasible incumbent" input of constrained_ei_a.  y [N], g [N, C]."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    limits = np.asarray(limits, dtype=np.float64).reshape(-1)
    g = np.asarray(g, dtype=np.float64).reshape(len(y), len(limits))
    ok = (g <= limits[None, :]).all(axis=1)
    return float(y[ok].min()) if ok.any() else math.inf


def _cei_normalized(model, constraint_models, fmin, limits):
    """fmin and every limit in y units -> that model's normalised space (float64); an infinite fmin stays infinite."""
    limits = np.asarray(limits if limits is not None else [], dtype=np.float64).reshape(-1)
    if len(limits) != len(constraint_models):
        raise ValueError(f"{len(constraint_models)} constraint models but {len(limits)} limits")
    fn = math.inf if math.isinf(fmin) and fmin > 0 else float(model.y_norm.project_into_normalized(np.array([fmin], dtype=np.float64))[0])
    ln = np.array([float(mo.y_norm.project_into_normalized(limits[k:k + 1])[0]) for k, mo in enumerate(constraint_models)], dtype=np.float64)
    return fn, ln


def constrained_ei_a(model, constraint_models, x, fmin, limits):
    """Constrained EI of the rows of x [m, d]: the EI of SurrogateModelGPR `model` (minimised) below fmin times the probability that
    every constraint_models[k] stays at or below limits[k], the posteriors taken as independent (gpr.constrained_ei).  fmin and
    limits are in y units; each goes through its own model's y projection, and EI is measured in the objective's normalised units.
    fmin = math.inf (feasible_fmin without a feasible row): the probability of feasibility alone.  Returns (cei[m] float64, best):
    best the last index of the maximum, -1 without rows."""
    fn, ln = _cei_normalized(model, constraint_models, fmin, limits)
    return gpr.constrained_ei(model.fitted, [mo.fitted for mo in constraint_models], np.asarray(x, dtype=model.dtype), fn, ln)


def maximize_constrained_ei(model, constraint_models, starts, bounds, fmin, limits, maxeval=150):
    """Bounded L-BFGS ascents of constrained_ei_a from every row of `starts` (the box: `bounds` = [(lo, hi)] per feature), all runs
    in lockstep on the device models (gpr.maximize_constrained_ei).  fmin and limits in y units.  Returns (x[S, d], cei[S],
    nevals[S])."""
    fn, ln = _cei_normalized(model, constraint_models, fmin, limits)
    return gpr.maximize_constrained_ei(model.fitted, [mo.fitted for mo in constraint_models], np.asarray(starts, dtype=model.dtype), bounds,
                                       fn, ln, maxeval=maxeval)


def log_constrained_ei_a(model, constraint_models, x, fmin, limits):
    """constrained_ei_a in log space (gpr.log_constrained_ei): finite, with a usable ranking, where constrained_ei_a is exactly 0.
    fmin and limits in y units.  Returns (lcei[m] float64, best)."""
    fn, ln = _cei_normalized(model, constraint_models, fmin, limits)
    return gpr.log_constrained_ei(model.fitted, [mo.fitted for mo in constraint_models], np.asarray(x, dtype=model.dtype), fn, ln)


def maximize_log_constrained_ei(model, constraint_models, starts, bounds, fmin, limits, maxeval=150):
    """maximize_constrained_ei on log_constrained_ei_a (gpr.maximize_log_constrained_ei): the runs move where every start has a
    constrained EI of exactly 0.  fmin and limits in y units.  Returns (x[S, d], lcei[S], nevals[S])."""
    fn, ln = _cei_normalized(model, constraint_models, fmin, limits)
    return gpr.maximize_log_constrained_ei(model.fitted, [mo.fitted for mo in constraint_models], np.asarray(starts, dtype=model.dtype),
                                           bounds, fn, ln, maxeval=maxeval)


def _cei_default_fmin(models, limits):
    """feasible_fmin of the models' training targets in y units; the models must have been trained on the very same rows."""
    fks = [mo.fitted for mo in models]
    xs = [fk.x_train for fk in fks]
    if any(x is None for x in xs) or any(fk.y_train is None for fk in fks):
        raise ValueError("the models do not hold their training rows: pass fmin")
    if any(x.shape != xs[0].shape or x.tobytes() != xs[0].tobytes() for x in xs[1:]):
        raise ValueError("the models were not trained on the same rows: pass fmin")
    y = [np.asarray(mo.y_norm.project_location_from_normalized(np.asarray(mo.fitted.y_train)), dtype=np.float64) for mo in models]
    return feasible_fmin(y[0], np.stack(y[1:], axis=1) if len(y) > 1 else np.zeros((len(y[0]), 0)), limits)


def _acquire_by_cei(evaluate, candidates, model, constraint_models, k, limits, fmin, ctx):
    """The greedy loop behind acquire_by_constrained_ei (evaluate = gpr.constrained_ei) and acquire_by_log_constrained_ei
    (gpr.log_constrained_ei)."""
    models = [model] + list(constraint_models)
    K = len(models)
    dtype = model.dtype
    c = np.asarray(candidates, dtype=dtype)
    if c.ndim != 2:
        raise ValueError("candidates must be [m, n_features]")
    k = int(k)
    if not 0 <= k <= c.shape[0]:
        raise ValueError("k must lie in [0, number of rows]")
    if fmin is None:
        fmin = _cei_default_fmin(models, limits)
    fn, ln = _cei_normalized(model, models[1:], fmin, limits)
    fks = [mo.fitted for mo in models]
    data = [(fk.x_train, fk.y_train) for fk in fks]
    if k > 1 and any(X is None or y is None for X, y in data):
        raise ValueError("the models do not hold their training rows: they cannot be conditioned on a fantasy")
    avail = list(range(c.shape[0]))
    idx, means, vals, fmins = [], [], [], []
    try:
        for t in range(k):
            val, best, _, _, mean, _ = evaluate(fks[0], fks[1:], c[avail], fn, ln, want_details=True)
            idx.append(avail.pop(best))
            means.append(mean[best])
            vals.append(val[best])
            believed = np.asarray(mean[best], dtype=np.float64)
            if (believed[1:] <= ln).all() and believed[0] < fn:
                fn = float(believed[0])
            fmins.append(fn)
            if t + 1 < k:
                for o in range(K):
                    X, y = data[o]
                    data[o] = (np.vstack([X, c[idx[-1]:idx[-1] + 1]]), np.concatenate([y, mean[best, o:o + 1]]))
                    nxt = fks[o].extend_with(*data[o], ctx=ctx)
                    if fks[o] is not models[o].fitted:
                        fks[o].release()
                    fks[o] = nxt
    finally:
        for o in range(K):
            if fks[o] is not models[o].fitted:
                fks[o].release()
    means = np.array(means, dtype=dtype).reshape(-1, K)
    proj = np.stack([models[o].y_norm.project_location_from_normalized(means[:, o]) for o in range(K)], axis=1)
    return np.array(idx, dtype=np.int64), proj, np.array(vals, dtype=np.float64), np.array(fmins, dtype=np.float64)


def acquire_by_constrained_ei(candidates, model, constraint_models, k, limits, fmin=None, ctx=None):
    """Batch acquisition under constraints by constrained EI over a candidate set [m, n_features]: k distinct rows, each the row of
    largest cEI (gpr.constrained_ei: closed form, no random numbers).  After a pick EVERY surrogate is conditioned on the
    kriging-believer fantasy (x_pick, that model's posterior mean) through extend_with at the same theta, as acquire_by_ehvi does;
    when the believed constraint values all hold and the believed objective lies below fmin, fmin falls to it.  limits and fmin are
    in y units.  Without fmin: feasible_fmin of the models' training targets, which needs models trained on the very same rows (else
    ValueError); it is math.inf while no feasible row is known.  Returns (idx[k] int64, the projected means [k, 1 + C] of the picks
    at the time they were picked, cei[k], and the fmin in force after each pick, in the objective's normalised units).  Opt-in:
    nothing the estimator suggests by default calls it."""
    return _acquire_by_cei(gpr.constrained_ei, candidates, model, constraint_models, k, limits, fmin, ctx)


def acquire_by_log_constrained_ei(candidates, model, constraint_models, k, limits, fmin=None, ctx=None):
    """acquire_by_constrained_ei ranking by the log-space value (gpr.log_constrained_ei): the same greedy loop, fantasies and fmin
    rule, but a pick is the row of largest lcei, which still orders the rows where every cEI underflows to 0 (there
    acquire_by_constrained_ei falls back to the last row).  Returns (idx[k], the projected means [k, 1 + C], lcei[k], fmin after
    each pick).  Opt-in."""
    return _acquire_by_cei(gpr.log_constrained_ei, candidates, model, constraint_models, k, limits, fmin, ctx)


def _nei_baseline(fk, baseline, max_baseline, dtype):
    """The baseline of a noisy-EI call: `baseline` or the model's training rows; with max_baseline the rows of lowest posterior
    mean under fk (ties to the lower index), kept in their order."""
    b = fk.x_train if baseline is None else baseline
    if b is None:
        raise ValueError("the model does not hold its training rows: pass a baseline")
    b = np.asarray(b, dtype=dtype)
    if b.ndim != 2 or b.shape[0] < 1:
        raise ValueError("the baseline must be [mb >= 1, n_features]")
    if max_baseline is not None:
        if int(max_baseline) < 1:
            raise ValueError("max_baseline must be >= 1")
        if b.shape[0] > int(max_baseline):
            mean, _, _ = fk.predict(b, want_variance=False)
            b = b[np.sort(np.argsort(mean, kind="stable")[:int(max_baseline)])]
    return b


def acquire_by_noisy_ei(candidates, model, k, rng, n_samples=256, baseline=None, jitter=0.0, max_baseline=None, ctx=None):
    """Batch acquisition for a noisy objective by noisy EI over a candidate set [m, n_features]: k distinct rows, each the row of
    largest noisy EI (FittedKernel.noisy_ei; the incumbent is the minimum of a joint posterior draw at the baseline, not a
    plugged-in number).  The baseline defaults to the model's training rows, cut to the max_baseline rows of lowest posterior mean
    when that is given.  After a pick the surrogate is conditioned on the kriging-believer fantasy (x_pick, its posterior mean)
    through extend_with at the same theta, as acquire_by_knowledge_gradient does, and the picked point joins the baseline.  The
    normals z [n_samples, mb] come from rng.standard_normal once and are reused while the baseline keeps its size (max_baseline);
    otherwise they are drawn again.  k = 1 is noisy_ei_a's best.  Returns (idx[k] int64, the projected means of the picks at the
    time they were picked, nei[k] in the normalised space).  Opt-in: nothing the estimator suggests by default calls it."""
    c = np.asarray(candidates, dtype=model.dtype)
    if c.ndim != 2:
        raise ValueError("candidates must be [m, n_features]")
    k = int(k)
    if not 0 <= k <= c.shape[0]:
        raise ValueError("k must lie in [0, number of candidates]")
    fk = model.fitted
    X, y = fk.x_train, fk.y_train
    if k > 1 and (X is None or y is None):
        raise ValueError("the model does not hold its training rows: it cannot be conditioned on a fantasy")
    base = None if k == 0 else np.asarray(fk.x_train if baseline is None else baseline, dtype=model.dtype)
    avail = list(range(c.shape[0]))
    idx, means, neis = [], [], []
    z = None
    try:
        for t in range(k):
            b = _nei_baseline(fk, base, max_baseline, model.dtype)
            if z is None or z.shape[1] != b.shape[0]:
                z = rng.standard_normal((int(n_samples), b.shape[0])).astype(model.dtype)
            nei, best = fk.noisy_ei(b, c[avail], z, jitter=jitter)
            j = avail.pop(best)
            mean, _, _ = fk.predict(c, want_variance=False)  # the batched predict of every row, as predict_mean_a runs it
            idx.append(j)
            means.append(mean[j])
            neis.append(nei[best])
            if t + 1 < k:
                X = np.vstack([X, c[j:j + 1]])
                y = np.concatenate([y, mean[j:j + 1]])
                base = np.vstack([base, c[j:j + 1]])
                nxt = fk.extend_with(X, y, ctx=ctx)
                if fk is not model.fitted:
                    fk.release()
                fk = nxt
    finally:
        if fk is not model.fitted:
            fk.release()
    means = np.array(means, dtype=model.dtype)
    return np.array(idx, dtype=np.int64), model.y_norm.project_location_from_normalized(means), np.array(neis, dtype=np.float64)


def acquire_by_qei(candidates, model, q, fmin, rng, n_samples=512, n_restarts=8, maxeval=150, jitter=0.0):
    """Batch acquisition by Monte Carlo q-EI: the q points are optimised jointly in the box the candidates span.  The starts are the
    greedy kriging-believer batch over the candidates (select_batch_a) and n_restarts - 1 random q-subsets of them; each start is
    one bounded L-BFGS ascent of q-EI with the same normals z [n_samples, q] (rng.standard_normal).  Returns (x[q, n_features], the
    batch's q-EI in the normalised space).  Opt-in: nothing the estimator suggests by default calls it."""
    c = np.asarray(candidates, dtype=model.dtype)
    if c.ndim != 2:
        raise ValueError("candidates must be [m, n_features]")
    q = int(q)
    if not 1 <= q <= c.shape[0]:
        raise ValueError("q must lie in [1, number of candidates]")
    idx, _, _ = model.select_batch_a(c, q, fmin)
    starts = [c[idx]]
    for _ in range(max(0, int(n_restarts) - 1)):
        u = rng.uniform(0.0, 1.0, c.shape[0])
        starts.append(c[np.argsort(u, kind="stable")[:q]])
    bounds = list(zip(c.min(axis=0).astype(np.float64), c.max(axis=0).astype(np.float64)))
    x, qei, _ = model.maximize_qei(np.stack(starts), bounds, fmin, n_samples, rng, jitter=jitter, maxeval=maxeval)
    best = int(np.argmax(qei))  # ties to the first run: the greedy batch
    return x[best], float(qei[best])


class FitnessOperator:
    """`FitnessOperator(model, space, fitness_via)` (minimize.rs:653-678) over feature arrays.  The reference predicts the
    mean of ONE individual per `get_fitness` call -- twice per comparison inside `sort_by` / `select_next_population`
    (minimize.rs:509-514, 566-575), each an O(n^2) single-point predict.  Here the fitness of a whole population is ONE
    batched `predict_mean_a`; comparisons then run on the cached values with the same `partial_cmp` semantics."""

    def __init__(self, model, fitness_via="prediction"):
        if fitness_via not in ("prediction", "observation"):
            raise ValueError(fitness_via)
        self.model, self.fitness_via = model, fitness_via

    def get_fitness(self, features, observations=None):
        """fitness of every individual: predicted mean at its features, or its observation (minimize.rs:657-668)."""
        if self.fitness_via == "prediction":
            return np.asarray(self.model.predict_mean_a(np.asarray(features)))
        if observations is None:
            raise ValueError("individual has no observation")
        return np.asarray(observations)

    @staticmethod
    def compare(fa, fb):
        """`a.partial_cmp(&b)` (minimize.rs:670-677): -1 / 0 / 1, or None when not comparable (NaN)."""
        if math.isnan(fa) or math.isnan(fb):
            return None
        return int(fa > fb) - int(fa < fb)

    def sort_population(self, features, observations=None):
        """indices of the population sorted by fitness, best (lowest) first: `population.sort_by(compare)` in
        `resize_population` (minimize.rs:509-514; Rust's sort_by is stable).  Raises where the reference panics."""
        f = self.get_fitness(features, observations)
        if np.isnan(f).any():
            raise ValueError("individuals are comparable")
        return np.argsort(f, kind="stable"), f

    def select_next_population(self, parent_features, offspring_features, parent_obs=None, offspring_obs=None):
        """`select_next_population` (minimize.rs:722-747): each offspring competes against its one parent and is kept unless
        `compare(parent, offspring) == Some(Less)` (so an incomparable pair keeps the offspring).  Returns a boolean array:
        True where the offspring is selected.  Two batched predicts for the whole generation."""
        fp = self.get_fitness(parent_features, parent_obs)
        fo = self.get_fitness(offspring_features, offspring_obs)
        with np.errstate(invalid="ignore"):
            return ~(fp < fo)


def find_best_individual_by_confidence_bound(features, model, confidence_bound):
    """minimize.rs:680-714 over a feature array: the individual with the lowest confidence bound (the FIRST of several
    minimal ones: the reference replaces its suggestion only on a strictly lower bound) and the predicted mean there.  One
    batched `predict_confidence_bound_a` + one `predict_mean` instead of one single-point predict per individual."""
    features = np.asarray(features)
    if features.ndim != 2 or features.shape[0] < 1:
        raise ValueError("should have at least one individual")
    ucb = np.asarray(model.predict_confidence_bound_a(features, confidence_bound))
    best = 0
    for i in range(1, len(ucb)):
        if ucb[i] < ucb[best]:
            best = i
    return best, model.predict_mean(features[best])


def suggest_optimum(features, model, confidence_bound=1.0, bounds=None, n_starts=1, maxeval=150):
    """minimize.rs:588-621, up to the validation samples, over a feature array [n, d]: the individual with the lowest confidence
    bound (find_best_individual_by_confidence_bound), then the minimisation of the bound over the box from that individual --
    the model's lockstep bounded L-BFGS on the exact gradient (model.minimize_confidence_bound) where the reference runs BOBYQA
    over 150 single-point predicts -- then mean and EI at the minimiser (model.predict_mean_ei) against `suggestion_y`, the start
    individual's predicted mean.  `bounds` = [(lo, hi)] per feature, default the unit box the reference uses.  With n_starts > 1
    the individuals with the next-lowest bounds at distinct points start runs 1 .. n_starts - 1 (fewer where the population holds
    fewer distinct points); the lowest run is returned, ties to the lower run index.  Run 0 starts at the scan's winner and a run
    is never worse than its start, so the suggestion's bound is at most that individual's, whatever n_starts is.
    Returns (x[d], bound, mean, ei, start): the suggestion, its projected bound (float64), its projected mean, its EI and the index
    of the scan's winner.  The reference sends every point BOBYQA tries through the design space and back, which snaps integer
    parameters; this function works in the continuous feature box and leaves the snapping of x to the caller.  Running the
    validation samples, extend and the final predict_statistics stay with the caller."""
    features = np.asarray(features)
    start, suggestion_y = find_best_individual_by_confidence_bound(features, model, confidence_bound)
    d = features.shape[1]
    if bounds is None:
        bounds = [(0.0, 1.0)] * d
    lo = np.array([b[0] for b in bounds], dtype=np.float64)
    hi = np.array([b[1] for b in bounds], dtype=np.float64)
    rows = [start]
    if int(n_starts) > 1:
        ucb = np.asarray(model.predict_confidence_bound_a(features, confidence_bound))
        for i in np.argsort(ucb, kind="stable"):
            if len(rows) < int(n_starts) and not any((features[i] == features[r]).all() for r in rows):
                rows.append(int(i))
    x, bound, _ = model.minimize_confidence_bound(_starts_in_box(features[rows], lo, hi, model.dtype), bounds, confidence_bound, maxeval=maxeval)
    run = 0
    for r in range(1, len(rows)):
        if bound[r] < bound[run]:
            run = r
    mean, ei = model.predict_mean_ei(x[run], suggestion_y)
    return x[run], bound[run], mean, ei, start


def acquire_by_confidence_bound(candidates, model, k, cb):
    """The k rows of `candidates` [m, n_features] with the lowest confidence bound mean + cb * std
    (model.predict_confidence_bound_a: one batched predict), lowest first, equal bounds in the order of their indices (a stable
    sort); a NaN bound raises.  cb > 0 prefers points that are good even pessimistically, cb < 0 is GP-LCB (Srinivas et al.
    2010): optimism in the face of uncertainty.  Opt-in: nothing the estimator suggests by default calls it.
    Returns (idx[k] int64, bound[k])."""
    c = np.asarray(candidates)
    if c.ndim != 2:
        raise ValueError("candidates must be [m, n_features]")
    k = int(k)
    if not 0 <= k <= c.shape[0]:
        raise ValueError("k must lie in [0, m]")
    bound = np.asarray(model.predict_confidence_bound_a(c, cb))
    if np.isnan(bound).any():
        raise ValueError("confidence bounds should be comparable")
    idx = np.argsort(bound, kind="stable")[:k].astype(np.int64)
    return idx, bound[idx]


class EstimatorGPR:
    """gpr.rs:215-400: defaults, builders, estimate(), extend()."""

    def __init__(self, n_features, ctx=None):  # Estimator::new(space) gpr.rs:219-236
        self._noise_bounds = (1e-5, 1e5)
        self._length_scale_bounds = [(1e-3, 1e3)] * n_features
        self._n_restarts_optimizer = 2
        self._matern_nu = 2.5
        self._amplitude_bounds = None
        self._y_projection = "linear"
        self._known_optimum = None
        self._objective = "lml"
        self._input_warping = False
        self.ctx = ctx

    @staticmethod
    def new(space_or_dims, ctx=None):
        n = space_or_dims if isinstance(space_or_dims, int) else len(space_or_dims)
        return EstimatorGPR(n, ctx)

    # builders gpr.rs:351-400
    def noise_bounds(self, lo, hi):
        self._noise_bounds = (lo, hi)
        return self

    def length_scale_bounds(self, bounds):
        self._length_scale_bounds = list(bounds)
        return self

    def n_restarts_optimizer(self, n):
        self._n_restarts_optimizer = n
        return self

    def matern_nu(self, nu):
        self._matern_nu = nu
        return self

    def amplitude_bounds(self, bounds):
        self._amplitude_bounds = bounds
        return self

    def y_projection(self, projection):
        self._y_projection = projection
        return self

    def known_optimum(self, value):
        self._known_optimum = value
        return self

    def objective(self, name="lml"):
        """What `estimate` maximises over the hyper-parameters: "lml", the log marginal likelihood (the reference's and the
        default), "loo", the leave-one-out log pseudo-likelihood (FittedKernel.new_by_loo), or "lgo", the leave-group-out log
        predictive density over the `groups` that `estimate` is given (FittedKernel.new_by_lgo)."""
        if name not in ("lml", "loo", "lgo"):
            raise ValueError(name)
        self._objective = name
        return self

    def input_warping(self, on=True, bounds=(0.2, 5.0)):
        """Opt-in (off by default, not in the reference): `estimate` learns one Kumaraswamy warp of [0, 1] per feature jointly with
        the kernel parameters (FittedKernel.new_warped; features must lie in [0, 1]; objective "lml" only).  The model's `fitted`
        is then a gpr.WarpedKernel: a plain fit first, the warped fit from its optimum, so the lml is no worse than without.
        bounds: the box of every a_k and b_k."""
        self._input_warping = bool(on)
        self._warp_bounds = (float(bounds[0]), float(bounds[1]))
        return self

    def _theta_and_bounds(self, prior, y_train):  # get_kernel_or_default gpr.rs:402-427
        if prior is not None:
            lo = np.array([prior.noise_bounds[0], prior.amplitude_bounds[0]] + [b[0] for b in prior.length_scale_bounds])
            hi = np.array([prior.noise_bounds[1], prior.amplitude_bounds[1]] + [b[1] for b in prior.length_scale_bounds])
            return prior.fitted.theta.copy(), lo, hi
        amp, a_lo, a_hi = estimate_amplitude(y_train, self._amplitude_bounds)  # gpr.rs:262
        noise = _bounded("noise level", 1.0, *self._noise_bounds)
        ells = [_bounded("length scale", math.exp((math.log(lo) + math.log(hi)) / 2.0), lo, hi) for lo, hi in self._length_scale_bounds]
        theta0 = np.log(np.array([noise, amp] + ells))
        lo = np.array([self._noise_bounds[0], a_lo] + [b[0] for b in self._length_scale_bounds])
        hi = np.array([self._noise_bounds[1], a_hi] + [b[1] for b in self._length_scale_bounds])
        return theta0, lo, hi

    def estimate(self, x, y, prior, rng, y_variance=None, groups=None):  # gpr.rs:238-291
        """groups (opt-in, read by objective("lgo") only): one int label per observation; rows that share a label are held out
        together (replicate_groups labels equal rows).  None with that objective means singletons: leave-one-out.
        y_variance (opt-in, not in the reference): the known noise variance of every y in y's own units -- for means of
        replicates the variance of the mean (aggregate_replicates).  It is projected into the normalised space and rides on the
        diagonal next to the learned noise (FittedKernel.new(..., row_variance=))."""
        x = np.asarray(x)
        y = np.asarray(y, dtype=x.dtype)
        assert y.shape == (x.shape[0],), f"expected y values for {x.shape[0]} observations"
        y_train, y_norm = YNormalize.new_project_into_normalized(y, self._y_projection, self._known_optimum)
        row_variance = None if y_variance is None else y_norm.project_variance_into_normalized(y, y_variance)
        theta0, lo, hi = self._theta_and_bounds(prior, y_train)
        fork = rng.fork_random_state()  # gpr.rs:276
        p = len(theta0)
        starts = None
        if self._n_restarts_optimizer > 0:  # gradmin.rs:22-24: uniform in log-bounds
            u = fork.uniform(0.0, 1.0, self._n_restarts_optimizer * p).reshape(self._n_restarts_optimizer, p)
            starts = np.log(lo)[None, :] + (np.log(hi) - np.log(lo))[None, :] * u
        # a prior hands over its whole kernel -- theta, bounds AND the Matern nu (prior.kernel.clone(), gpr.rs:407-409);
        # the estimator's own nu only configures the default kernel
        nu = prior.fitted.nu if prior is not None else self._matern_nu
        fit = gpr.FittedKernel.new_by_loo if self._objective == "loo" else gpr.FittedKernel.new
        if self._input_warping:
            if self._objective != "lml":
                raise NotImplementedError("input warping is built for the lml objective only")

            def fit(*args, **kw):
                return gpr.FittedKernel.new_warped(*args, warp_bounds=self._warp_bounds, **kw)
        if self._objective == "lgo":
            def fit(*args, **kw):
                return gpr.FittedKernel.new_by_lgo(*args, groups=groups, **kw)
        if row_variance is None:
            fitted = fit(x, y_train.astype(x.dtype), theta0, lo, hi, starts, nu=nu, ctx=self.ctx)
        else:
            fitted = fit(x, y_train.astype(x.dtype), theta0, lo, hi, starts, nu=nu, ctx=self.ctx, row_variance=row_variance)
        return SurrogateModelGPR(fitted, (lo[0], hi[0]), (lo[1], hi[1]), list(zip(lo[2:], hi[2:])), y_norm, x.dtype)

    def extend(self, x, y, prior, rng=None, y_variance=None):  # gpr.rs:293-337
        """y_variance: as in `estimate`.  Without it the new model has no row variances, whatever the prior carried."""
        x = np.asarray(x)
        y = np.asarray(y, dtype=x.dtype)
        assert y.shape == (x.shape[0],), f"expected y values for {x.shape[0]} observations"
        y_train, y_norm = YNormalize.new_project_into_normalized(y, self._y_projection, self._known_optimum)
        row_variance = None if y_variance is None else y_norm.project_variance_into_normalized(y, y_variance)
        lo = np.array([prior.noise_bounds[0], prior.amplitude_bounds[0]] + [b[0] for b in prior.length_scale_bounds])
        hi = np.array([prior.noise_bounds[1], prior.amplitude_bounds[1]] + [b[1] for b in prior.length_scale_bounds])
        if isinstance(prior.fitted, gpr.WarpedKernel):
            # the warp is the prior's, fixed: the new rows go through it (incrementally where the leading rows are the prior's)
            ext = prior.fitted.extend_with if prior.fitted.dtype == x.dtype else prior.fitted.extend
            fitted = ext(x, y_train.astype(x.dtype), ctx=self.ctx, row_variance=row_variance)
        elif row_variance is not None:
            if prior.fitted.dtype == x.dtype:
                fitted = prior.fitted.extend_with(x, y_train.astype(x.dtype), ctx=self.ctx, row_variance=row_variance)
            else:
                fitted = gpr.FittedKernel.extend(x, y_train.astype(x.dtype), prior.fitted.theta, lo, hi, nu=prior.fitted.nu, ctx=self.ctx,
                                                 row_variance=row_variance)
        elif prior.fitted.dtype == x.dtype and getattr(prior.fitted, "row_variance", None) is None:
            # the kernel (incl. its nu) is the prior's (prior.kernel.clone(), gpr.rs:318-323)
            # the caller appends its validation samples to the rows the prior was built on (minimize.rs:629-644): the engine
            # reuses the prior's factorisation for the unchanged leading rows (falls back by itself when they differ)
            fitted = prior.fitted.extend_with(x, y_train.astype(x.dtype), ctx=self.ctx)
        else:
            fitted = gpr.FittedKernel.extend(x, y_train.astype(x.dtype), prior.fitted.theta, lo, hi, nu=prior.fitted.nu, ctx=self.ctx)
        return SurrogateModelGPR(fitted, prior.noise_bounds, prior.amplitude_bounds, prior.length_scale_bounds, y_norm, x.dtype)
