"""Host-side mirror of the reference's `src/gpr` interface over the C ABI (include/hbegp.h).

Names follow the reference: `FittedKernel.new / .extend` (src/gpr/fit.rs:18-68), `predict` (src/gpr/predict.rs:7-52),
`LmlWithGradient.of` (src/gpr/lml.rs:16-27).  All arithmetic happens in libhbegp.so on the GPU; this file only
marshals arrays.  Python is used here because the reference's own toolchain (Rust) is absent from the build image;
the Rust binding a maintainer would write is in INTEGRATION.md.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import HbegpError, NOT_PD, ALL_FAILED  # noqa: F401


def _suffix(dtype):
    dt = np.dtype(dtype)
    if dt == np.float64:
        return "f64"
    if dt == np.float32:
        return "f32"
    raise TypeError(f"element type must be float64 or float32, got {dt}")


class Context:
    """Owns the GPUs used by fits (hbegp_ctx)."""

    def __init__(self, n_devices=1, device_ids=None):
        lib = _lib.load()
        self._h = C.c_void_p()
        ids = None
        if device_ids is not None:
            ids = (C.c_int * len(device_ids))(*device_ids)
            n_devices = len(device_ids)
        _lib.check(lib.hbegp_ctx_create(n_devices, ids, C.byref(self._h)))
        self.n_devices = n_devices

    def close(self):
        if self._h:
            _lib.load().hbegp_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(1)
    return _default_ctx


def device_count():
    return _lib.load().hbegp_device_count()


def _row_variance(row_variance, n):
    """The caller's per-row noise variances as the C ABI takes them: float64 [n], or None."""
    if row_variance is None:
        return None
    rv = _lib.as_c(np.asarray(row_variance, dtype=np.float64).reshape(-1), np.float64)
    if rv.shape != (n,):
        raise ValueError(f"row_variance must have one entry per training row ({n}), got {rv.shape}")
    return rv


def _group_labels(groups, n):
    """The caller's group labels as the C ABI takes them: int32 [n], or None (every row its own group)."""
    if groups is None:
        return None
    g = np.asarray(groups).reshape(-1)
    if g.shape != (n,):
        raise ValueError(f"groups must have one label per training row ({n}), got {g.shape}")
    if not np.issubdtype(g.dtype, np.integer):
        raise ValueError(f"group labels must be integers, got {g.dtype}")
    return np.ascontiguousarray(g, dtype=np.int32)


def _iptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


class Warp:
    """The Kumaraswamy input warp u_k = 1 - (1 - x_k^a_k)^b_k of features in [0, 1] (hbegp_warp_apply / _invert: host fp64, no
    GPU).  ab = [a_1..a_d, b_1..b_d], all > 0; a = b = 1 is the identity."""

    def __init__(self, ab):
        self.ab = _lib.as_c(np.asarray(ab, dtype=np.float64).reshape(-1), np.float64)
        if self.ab.size < 2 or self.ab.size % 2:
            raise ValueError(f"a warp takes 2 d parameters [a_1..a_d, b_1..b_d], got {self.ab.size}")
        self.d = self.ab.size // 2
        if not (np.all(np.isfinite(self.ab)) and np.all(self.ab > 0)):
            raise ValueError("warp parameters must be finite and positive")

    @staticmethod
    def identity(d):
        return Warp(np.ones(2 * d))

    @property
    def a(self):
        return self.ab[:self.d]

    @property
    def b(self):
        return self.ab[self.d:]

    def _rows(self, x):
        x = np.asarray(x)
        rows = _lib.as_c(x.reshape(-1, self.d), np.float64)
        return x, rows

    def apply(self, x, want_param_gradients=False):
        """u = w(x) in fp64, shaped like x ([..., d]); with want_param_gradients also du/dln a and du/dln b."""
        x, rows = self._rows(x)
        u = np.empty_like(rows)
        da = np.empty_like(rows) if want_param_gradients else None
        db = np.empty_like(rows) if want_param_gradients else None
        _lib.check(_lib.load().hbegp_warp_apply(_lib.dptr(self.ab), self.d, _lib.dptr(rows), rows.shape[0], _lib.dptr(u), _lib.dptr(da),
                                                _lib.dptr(db), None))
        if want_param_gradients:
            return u.reshape(x.shape), da.reshape(x.shape), db.reshape(x.shape)
        return u.reshape(x.shape)

    def invert(self, u):
        """x with w(x) = u, shaped like u."""
        u, rows = self._rows(u)
        x = np.empty_like(rows)
        _lib.check(_lib.load().hbegp_warp_invert(_lib.dptr(self.ab), self.d, _lib.dptr(rows), rows.shape[0], _lib.dptr(x)))
        return x.reshape(u.shape)

    def jacobian(self, x):
        """du_k/dx_k, shaped like x (the map is per coordinate: the Jacobian is diagonal).  +inf at an end whose exponent is < 1."""
        x, rows = self._rows(x)
        dx = np.empty_like(rows)
        _lib.check(_lib.load().hbegp_warp_apply(_lib.dptr(self.ab), self.d, _lib.dptr(rows), rows.shape[0], None, None, None,
                                                _lib.dptr(dx)))
        return dx.reshape(x.shape)


class Problem:
    """X, y resident on the device; repeated lml/gradient evaluations (the optimiser's inner loop)."""

    def __init__(self, x_train, y_train, nu=2.5, n_slots=1, ctx=None, row_variance=None):
        """row_variance: known noise variances v_i >= 0 of the rows (normalised y scale), added to the diagonal next to the learned
        noise: K = c Matern + diag(s2 + v)."""
        lib = _lib.load()
        self.ctx = ctx or default_context()
        self.dtype = np.dtype(x_train.dtype)
        sfx = _suffix(self.dtype)
        self.x = _lib.as_c(x_train, self.dtype)
        self.y = _lib.as_c(y_train, self.dtype)
        assert self.x.ndim == 2 and self.y.shape == (self.x.shape[0],)
        self.n, self.d = self.x.shape
        self.p = self.d + 2
        self._sfx = sfx
        self._h = C.c_void_p()
        self.row_variance = _row_variance(row_variance, self.n)
        if self.row_variance is None:
            create = getattr(lib, f"hbegp_problem_create_{sfx}")
            _lib.check(create(self.ctx._h, _lib.aptr(self.x), _lib.aptr(self.y), self.n, self.d, float(nu), n_slots, C.byref(self._h)))
        else:
            create = getattr(lib, f"hbegp_problem_create_rv_{sfx}")
            _lib.check(create(self.ctx._h, _lib.aptr(self.x), _lib.aptr(self.y), _lib.dptr(self.row_variance), self.n, self.d, float(nu),
                              n_slots, C.byref(self._h)))

    def close(self):
        if self._h:
            _lib.load().hbegp_problem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lml_with_gradient(self, theta, lo=None, hi=None, want_grad=True, dev=0, slot=0):
        """LmlWithGradient::of (lml.rs:16-79) at log-space theta.  Returns (lml, grad) or None when not PD."""
        lib = _lib.load()
        theta = _lib.as_c(theta, np.float64)
        lo = None if lo is None else _lib.as_c(lo, np.float64)
        hi = None if hi is None else _lib.as_c(hi, np.float64)
        lml = C.c_double()
        grad = np.zeros(self.p) if want_grad else None
        code = lib.hbegp_problem_eval(self._h, dev, slot, _lib.dptr(theta), _lib.dptr(lo), _lib.dptr(hi), C.byref(lml), _lib.dptr(grad))
        if _lib.check(code, allow=(NOT_PD,)) == NOT_PD:
            return None
        return lml.value, grad

    def loo_with_gradient(self, theta, lo=None, hi=None, want_grad=True, dev=0, slot=0):
        """The leave-one-out log pseudo-likelihood at log-space theta and its gradient (hbegp_problem_eval_loo): the slot's
        evaluation, then the closed-form leave-one-out tail on its results.  Returns (loo, grad) or None when not PD."""
        lib = _lib.load()
        theta = _lib.as_c(theta, np.float64)
        lo = None if lo is None else _lib.as_c(lo, np.float64)
        hi = None if hi is None else _lib.as_c(hi, np.float64)
        loo = C.c_double()
        grad = np.zeros(self.p) if want_grad else None
        code = lib.hbegp_problem_eval_loo(self._h, dev, slot, _lib.dptr(theta), _lib.dptr(lo), _lib.dptr(hi), C.byref(loo), _lib.dptr(grad))
        if _lib.check(code, allow=(NOT_PD,)) == NOT_PD:
            return None
        return loo.value, grad

    def lgo_with_gradient(self, theta, groups, lo=None, hi=None, want_grad=True, dev=0, slot=0):
        """The leave-group-out log predictive density at log-space theta and its gradient (hbegp_problem_eval_lgo): the slot's
        evaluation, then the closed-form leave-group-out tail over `groups` (one int label per row; None: singletons, which is
        leave-one-out).  Returns (lgo, grad) or None when not PD."""
        lib = _lib.load()
        theta = _lib.as_c(theta, np.float64)
        lo = None if lo is None else _lib.as_c(lo, np.float64)
        hi = None if hi is None else _lib.as_c(hi, np.float64)
        g = _group_labels(groups, self.n)
        lgo = C.c_double()
        grad = np.zeros(self.p) if want_grad else None
        code = lib.hbegp_problem_eval_lgo(self._h, dev, slot, _lib.dptr(theta), _lib.dptr(lo), _lib.dptr(hi), _iptr(g), C.byref(lgo),
                                          _lib.dptr(grad))
        if _lib.check(code, allow=(NOT_PD,)) == NOT_PD:
            return None
        return lgo.value, grad

    def lml_with_x_gradient(self, theta, lo=None, hi=None, want_grad=True, dev=0, slot=0):
        """lml_with_gradient plus gx [n, d] = d lml / d x_train in fp64 (hbegp_problem_eval_xgrad): the slot's evaluation, then
        the input-gradient tail on its results.  Returns (lml, grad, gx) or None when not PD."""
        lib = _lib.load()
        theta = _lib.as_c(theta, np.float64)
        lo = None if lo is None else _lib.as_c(lo, np.float64)
        hi = None if hi is None else _lib.as_c(hi, np.float64)
        lml = C.c_double()
        grad = np.zeros(self.p) if want_grad else None
        gx = np.zeros((self.n, self.d))
        code = lib.hbegp_problem_eval_xgrad(self._h, dev, slot, _lib.dptr(theta), _lib.dptr(lo), _lib.dptr(hi), C.byref(lml),
                                            _lib.dptr(grad), _lib.dptr(gx))
        if _lib.check(code, allow=(NOT_PD,)) == NOT_PD:
            return None
        return lml.value, grad, gx

    def warped_lml_with_gradient(self, theta, warp, lo=None, hi=None, want_grad=True, dev=0, slot=0):
        """lml(w(x_train; a, b), theta) and its gradient [p + 2 d]: theta's entries, then d/dln a_k, then d/dln b_k
        (hbegp_problem_eval_warped; single-slot problems with features in [0, 1] only).  `warp` is a Warp or its 2 d parameters.
        Returns (lml, grad) or None when not PD."""
        lib = _lib.load()
        ab = warp.ab if isinstance(warp, Warp) else _lib.as_c(np.asarray(warp, dtype=np.float64).reshape(-1), np.float64)
        if ab.shape != (2 * self.d,):
            raise ValueError(f"the warp must have 2 d = {2 * self.d} parameters, got {ab.shape}")
        theta = _lib.as_c(theta, np.float64)
        lo = None if lo is None else _lib.as_c(lo, np.float64)
        hi = None if hi is None else _lib.as_c(hi, np.float64)
        lml = C.c_double()
        grad = np.zeros(self.p + 2 * self.d) if want_grad else None
        code = lib.hbegp_problem_eval_warped(self._h, dev, slot, _lib.dptr(theta), _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(ab),
                                             C.byref(lml), _lib.dptr(grad))
        if _lib.check(code, allow=(NOT_PD,)) == NOT_PD:
            return None
        return lml.value, grad

    def debug_rows(self, dev=0):
        """The rows [n, d] the device's feature buffer holds at the moment (hbegp_problem_debug_rows_*)."""
        out = np.zeros((self.n, self.d), dtype=self.dtype)
        _lib.check(getattr(_lib.load(), f"hbegp_problem_debug_rows_{self._sfx}")(self._h, dev, _lib.aptr(out)))
        return out

    def results(self, want_kinv=True, dev=0, slot=0):
        """(alpha, k_inv, diag(L)) of the most recent evaluation."""
        lib = _lib.load()
        alpha = np.zeros(self.n, dtype=self.dtype)
        ldiag = np.zeros(self.n, dtype=self.dtype)
        kinv = np.zeros((self.n, self.n), dtype=self.dtype) if want_kinv else None
        get = getattr(lib, f"hbegp_problem_get_{self._sfx}")
        _lib.check(get(self._h, dev, slot, _lib.aptr(alpha), _lib.aptr(kinv), _lib.aptr(ldiag)))
        return alpha, kinv, ldiag

    def debug_work_matrix(self, which, dev=0, slot=0):
        """Raw copy of W1 (which=1) or W2 (which=2) after the last evaluation: [np, np] with np = n rounded up to 128."""
        npad = (self.n + 127) // 128 * 128
        out = np.zeros((npad, npad), dtype=self.dtype)
        get = getattr(_lib.load(), f"hbegp_problem_debug_get_{self._sfx}")
        _lib.check(get(self._h, dev, slot, which, _lib.aptr(out)))
        return out

    def kernel_matrix(self, theta, lo=None, hi=None, dev=0, slot=0):
        lib = _lib.load()
        theta = _lib.as_c(theta, np.float64)
        lo = None if lo is None else _lib.as_c(lo, np.float64)
        hi = None if hi is None else _lib.as_c(hi, np.float64)
        K = np.zeros((self.n, self.n), dtype=self.dtype)
        kmat = getattr(lib, f"hbegp_problem_kmat_{self._sfx}")
        _lib.check(kmat(self._h, dev, slot, _lib.dptr(theta), _lib.dptr(lo), _lib.dptr(hi), _lib.aptr(K)))
        return K

    def time_eval(self, theta, reps=5, dev=0, slot=0):
        lib = _lib.load()
        theta = _lib.as_c(theta, np.float64)
        phases = np.zeros(24)
        _lib.check(lib.hbegp_problem_time_eval(self._h, dev, slot, _lib.dptr(theta), reps, _lib.dptr(phases)))
        keys = ["kmat_ms", "chol_gemm_ms", "leaf_ms", "lauum_ms", "alpha_ms", "gradtrace_ms", "eval_graph_ms", "n_gemm",
                "gemm128_ms", "gemm128_gflop", "gemm64_ms", "gemm64_gflop", "gemm32_ms", "gemm32_gflop", "eval_eager_ms", "n_leaf",
                "n_gemm128", "n_gemm64", "n_gemm32", "dag_ms", "dag_gflop", "r1", "r2", "r3"]
        return dict(zip(keys, phases.tolist()))

    def time_concurrent(self, theta, reps=5, dev=0):
        """Every slot evaluating at once (the configuration a fit runs in): wall time per round and per-kernel-class times
        from hipEvents on each slot's stream."""
        lib = _lib.load()
        theta = _lib.as_c(theta, np.float64)
        out = np.zeros(16)
        _lib.check(lib.hbegp_problem_time_concurrent(self._h, dev, _lib.dptr(theta), reps, _lib.dptr(out)))
        keys = ["round_ms", "n_slots", "round_eager_ms", "kmat_ms", "factor_ms", "factor_gflop", "lauum_ms", "lauum_gflop", "alpha_ms",
                "gradtrace_ms", "task_queue_workgroups", "factor_launches"]
        return dict(zip(keys, out.tolist()))


class FittedKernel:
    """Mirror of `FittedKernel<K, A>` (fit.rs:6-12): kernel parameters, noise, alpha, k_inv, lml + the model handle."""

    def __init__(self, handle, dtype, n, d, nu):
        self._h = handle
        self.dtype = np.dtype(dtype)
        self.n, self.d, self.nu = n, d, nu
        self.x_train = self.y_train = None  # the host copies of the training rows (normalised y), set by new / extend / extend_with
        self._sfx = _suffix(dtype)
        lml = C.c_double()
        _lib.check(_lib.load().hbegp_model_info(self._h, None, None, None, None, C.byref(lml)))
        self.lml = lml.value
        self.theta = np.zeros(d + 2)
        get = getattr(_lib.load(), f"hbegp_model_get_{self._sfx}")
        _lib.check(get(self._h, _lib.dptr(self.theta), None, None))

    # -- parameters in the reference's terms --
    @property
    def noise(self):
        return math.exp(self.theta[0])

    @property
    def amplitude(self):
        return math.exp(self.theta[1])

    @property
    def length_scale(self):
        return np.exp(self.theta[2:])

    @property
    def row_variance(self):
        """The per-row noise variances the model works with (hbegp_model_row_variance), float64 [n] -- for a float32 model the
        rounded values, widened; None for a model without them."""
        lib = _lib.load()
        if lib.hbegp_model_row_variance(self._h, None) != 1:
            return None
        out = np.zeros(self.n)
        lib.hbegp_model_row_variance(self._h, _lib.dptr(out))
        return out

    def device_params(self):
        """(noise, amplitude, length_scale) as the model's posterior queries use them (hbegp_model_debug_params): for a
        device-driven fit the captured evaluation's own numbers, which may differ from exp(theta) in the last bit."""
        out = np.zeros(self.d + 2)
        _lib.check(_lib.load().hbegp_model_debug_params(self._h, _lib.dptr(out)))
        return float(out[0]), float(out[1]), out[2:].copy()

    def arrays(self, want_kinv=True):
        """(alpha, k_inv) copied from the device; k_inv is the full symmetric matrix (fit.rs:60,168)."""
        alpha = np.zeros(self.n, dtype=self.dtype)
        kinv = np.zeros((self.n, self.n), dtype=self.dtype) if want_kinv else None
        get = getattr(_lib.load(), f"hbegp_model_get_{self._sfx}")
        _lib.check(get(self._h, None, _lib.aptr(alpha), _lib.aptr(kinv)))
        return alpha, kinv

    @staticmethod
    def new(x_train, y_train, theta0, lo, hi, starts=None, nu=2.5, ctx=None, maxeval=150, fixed_work=False, trace=False,
            row_variance=None):
        """FittedKernel::new (fit.rs:18-31, 71-176): 1 + len(starts) bounded L-BFGS runs, capture the best lml.

        trace=True records (theta, lml, gradient, run) of every evaluation; a fit that records gradients evaluates every
        line-search trial whole.  trace="lml" records (theta, lml, run) only and leaves the evaluation as an untraced fit's:
        trials the optimiser rejects end after their lml (`n_lml_only` counts them; HBEGP_LAZY_GRAD=0 turns that off).

        row_variance: known noise variances v_i >= 0 of the rows in the normalised y scale (hbegp_fit_rv_*): data, not a
        hyper-parameter -- K = c Matern + diag(s2 + v), and s2 is still learned as the homoscedastic remainder."""
        return FittedKernel._fit("hbegp_fit", x_train, y_train, theta0, lo, hi, starts, nu, ctx, maxeval, fixed_work, trace, row_variance)

    @staticmethod
    def new_by_loo(x_train, y_train, theta0, lo, hi, starts=None, nu=2.5, ctx=None, maxeval=150, fixed_work=False, trace=False,
                   row_variance=None):
        """`new` with the leave-one-out log pseudo-likelihood as the objective (hbegp_fit_loo_*): the same runs, options and
        trace (trace["lml"] holds loo), capture of the best loo in `.loo_best`; the model is `extend` at the captured theta."""
        return FittedKernel._fit("hbegp_fit_loo", x_train, y_train, theta0, lo, hi, starts, nu, ctx, maxeval, fixed_work, trace, row_variance)

    @staticmethod
    def new_by_lgo(x_train, y_train, theta0, lo, hi, starts=None, nu=2.5, ctx=None, maxeval=150, fixed_work=False, trace=False,
                   groups=None, row_variance=None):
        """`new_by_loo` with the leave-group-out log predictive density over `groups` (one int label per row, at most 64 rows
        per group; None: singletons) as the objective (hbegp_fit_lgo_*): rows that are replicates or near-duplicates of each
        other are held out together.  Capture of the best lgo in `.lgo_best`; the model is `extend` at the captured theta."""
        return FittedKernel._fit("hbegp_fit_lgo", x_train, y_train, theta0, lo, hi, starts, nu, ctx, maxeval, fixed_work, trace, row_variance,
                                 groups)

    @staticmethod
    def _fit(symbol, x_train, y_train, theta0, lo, hi, starts, nu, ctx, maxeval, fixed_work, trace, row_variance=None, groups=None):
        lib = _lib.load()
        ctx = ctx or default_context()
        dtype = np.dtype(x_train.dtype)
        sfx = _suffix(dtype)
        x = _lib.as_c(x_train, dtype)
        y = _lib.as_c(y_train, dtype)
        n, d = x.shape
        p = d + 2
        theta0 = _lib.as_c(theta0, np.float64)
        lo = _lib.as_c(lo, np.float64)
        hi = _lib.as_c(hi, np.float64)
        assert theta0.shape == (p,) and lo.shape == (p,) and hi.shape == (p,)
        n_restarts = 0 if starts is None else len(starts)
        starts_c = None if n_restarts == 0 else _lib.as_c(np.asarray(starts).reshape(n_restarts, p), np.float64)
        opt = _lib.FitOptions()
        opt.maxeval = maxeval
        opt.fixed_work = 1 if fixed_work else 0
        n_evals, n_not_pd = C.c_int(0), C.c_int(0)
        opt.n_evals = C.pointer(n_evals)
        opt.n_not_pd = C.pointer(n_not_pd)
        tr = None
        if trace:
            cap = (1 + n_restarts) * maxeval
            tr = dict(theta=np.zeros((cap, p)), lml=np.zeros(cap), grad=np.zeros((cap, p)), run=np.zeros(cap, dtype=np.int32),
                      count=C.c_int(0))
            opt.trace_cap = cap
            opt.trace_theta = _lib.dptr(tr["theta"])
            opt.trace_lml = _lib.dptr(tr["lml"])
            if trace != "lml":
                opt.trace_grad = _lib.dptr(tr["grad"])
            opt.trace_run = tr["run"].ctypes.data_as(C.POINTER(C.c_int))
            opt.trace_count = C.pointer(tr["count"])
        handle = C.c_void_p()
        theta_best = np.zeros(p)
        lml_best = C.c_double()
        rv = _row_variance(row_variance, n)
        tail = (n, d, float(nu), _lib.dptr(theta0), _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(starts_c), n_restarts, C.byref(opt),
                _lib.dptr(theta_best), C.byref(lml_best), C.byref(handle))
        if symbol == "hbegp_fit_lgo":  # one entry point: rv and the labels are both nullable arguments
            g = _group_labels(groups, n)
            _lib.check(getattr(lib, f"{symbol}_{sfx}")(ctx._h, _lib.aptr(x), _lib.aptr(y), _lib.dptr(rv), _iptr(g), *tail))
        elif rv is None:
            _lib.check(getattr(lib, f"{symbol}_{sfx}")(ctx._h, _lib.aptr(x), _lib.aptr(y), *tail))
        else:
            _lib.check(getattr(lib, f"{symbol}_rv_{sfx}")(ctx._h, _lib.aptr(x), _lib.aptr(y), _lib.dptr(rv), *tail))
        fk = FittedKernel(handle, dtype, n, d, nu)
        fk.x_train, fk.y_train = x, y
        fk.n_evals, fk.n_not_pd = n_evals.value, n_not_pd.value
        stats = _lib.FitStats()
        _lib.check(lib.hbegp_last_fit_stats(C.byref(stats)))  # this thread's fit, the one above
        fk.n_lml_only = stats.n_lml_only
        # per optimiser run (hbegp_fit_stats): when its last evaluation was over, in ms since the fit was called, and what it launched
        k = stats.n_runs
        fk.run_end_ms = np.array(stats.run_end_ms[:k], dtype=np.float64)
        fk.run_counts = {name: np.array(getattr(stats, "run_" + name)[:k], dtype=np.int64)
                         for name in ("fused", "lml_only", "phase2", "lead", "lag")}
        fk.theta_best = theta_best
        if symbol == "hbegp_fit_loo":
            fk.loo_best = lml_best.value
        if symbol == "hbegp_fit_lgo":
            fk.lgo_best = lml_best.value
        if trace:
            k = tr["count"].value
            fk.trace = dict(theta=tr["theta"][:k], lml=tr["lml"][:k], run=tr["run"][:k])
            if trace != "lml":
                fk.trace["grad"] = tr["grad"][:k]
        return fk

    @staticmethod
    def new_warped(x_train, y_train, theta0, lo, hi, starts=None, nu=2.5, ctx=None, maxeval=150, fixed_work=False, trace=False,
                   row_variance=None, warp_bounds=(0.2, 5.0), warp_starts=None, plain=None):
        """`new` with one Kumaraswamy input warp per feature learned jointly with theta (hbegp_fit_warped_*; features in [0, 1]).

        A plain `new` runs first (or `plain`, a FittedKernel from the same arguments, is taken); run 0 of the warped fit starts at
        its optimum with the identity warp, so the result's lml is no worse than the plain fit's.  starts: [R, p] as for `new`; each
        also starts a warped run, from warp_starts[r] ([R, 2 d], ln a then ln b; default: the identity).  The runs go one after
        another on one slot.  Returns a WarpedKernel: `.inner` the u-space FittedKernel, `.warp` the learned Warp, `.plain_lml`
        the plain fit's lml.  With trace: `.trace` rows hold the p + 2 d log-space variables."""
        lib = _lib.load()
        ctx = ctx or default_context()
        dtype = np.dtype(x_train.dtype)
        sfx = _suffix(dtype)
        x = _lib.as_c(x_train, dtype)
        y = _lib.as_c(y_train, dtype)
        n, d = x.shape
        p, q = d + 2, 3 * d + 2
        lo = _lib.as_c(lo, np.float64)
        hi = _lib.as_c(hi, np.float64)
        own_plain = plain is None
        if own_plain:
            plain = FittedKernel.new(x, y, theta0, lo, hi, starts=starts, nu=nu, ctx=ctx, maxeval=maxeval, fixed_work=fixed_work,
                                     row_variance=row_variance)
        plain_lml, plain_theta = plain.lml, plain.theta.copy()
        if own_plain:
            plain.release()
        n_restarts = 0 if starts is None else len(starts)
        starts_c = None
        if n_restarts:
            ws = np.zeros((n_restarts, 2 * d)) if warp_starts is None else np.asarray(warp_starts, dtype=np.float64).reshape(n_restarts, 2 * d)
            starts_c = _lib.as_c(np.concatenate([np.asarray(starts, dtype=np.float64).reshape(n_restarts, p), ws], axis=1), np.float64)
        ab_lo = _lib.as_c(np.broadcast_to(np.asarray(warp_bounds[0], dtype=np.float64), (2 * d,)), np.float64)
        ab_hi = _lib.as_c(np.broadcast_to(np.asarray(warp_bounds[1], dtype=np.float64), (2 * d,)), np.float64)
        opt = _lib.FitOptions()
        opt.maxeval = maxeval
        opt.fixed_work = 1 if fixed_work else 0
        n_evals, n_not_pd = C.c_int(0), C.c_int(0)
        opt.n_evals = C.pointer(n_evals)
        opt.n_not_pd = C.pointer(n_not_pd)
        tr = None
        if trace:
            cap = (1 + n_restarts) * maxeval
            tr = dict(theta=np.zeros((cap, q)), lml=np.zeros(cap), grad=np.zeros((cap, q)), run=np.zeros(cap, dtype=np.int32),
                      count=C.c_int(0))
            opt.trace_cap = cap
            opt.trace_theta = _lib.dptr(tr["theta"])
            opt.trace_lml = _lib.dptr(tr["lml"])
            opt.trace_grad = _lib.dptr(tr["grad"])
            opt.trace_run = tr["run"].ctypes.data_as(C.POINTER(C.c_int))
            opt.trace_count = C.pointer(tr["count"])
        handle = C.c_void_p()
        theta_best, ab_best, lml_best = np.zeros(p), np.zeros(2 * d), C.c_double()
        rv = _row_variance(row_variance, n)
        theta_start = _lib.as_c(plain_theta, np.float64)
        _lib.check(getattr(lib, f"hbegp_fit_warped_{sfx}")(
            ctx._h, _lib.aptr(x), _lib.aptr(y), _lib.dptr(rv), n, d, float(nu), _lib.dptr(theta_start), _lib.dptr(lo), _lib.dptr(hi), None,
            _lib.dptr(ab_lo), _lib.dptr(ab_hi), _lib.dptr(starts_c), n_restarts, C.byref(opt), _lib.dptr(theta_best), _lib.dptr(ab_best),
            C.byref(lml_best), C.byref(handle)))
        inner = FittedKernel(handle, dtype, n, d, nu)
        warp = Warp(ab_best)
        inner.x_train, inner.y_train = warp.apply(x.astype(np.float64)).astype(dtype), y
        inner.n_evals, inner.n_not_pd = n_evals.value, n_not_pd.value
        inner.theta_best = theta_best
        wk = WarpedKernel(inner, warp)
        wk.x_train, wk.lml_best, wk.plain_lml, wk.plain_theta = x, lml_best.value, plain_lml, plain_theta
        if trace:
            k = tr["count"].value
            wk.trace = dict(theta=tr["theta"][:k], lml=tr["lml"][:k], grad=tr["grad"][:k], run=tr["run"][:k])
        return wk

    @property
    def warp_parameters(self):
        """[a_1..a_d, b_1..b_d] of the input warp a model from hbegp_fit_warped_* carries (hbegp_model_warp); None for every other
        model."""
        lib = _lib.load()
        if lib.hbegp_model_warp(self._h, None) != 1:
            return None
        ab = np.zeros(2 * self.d)
        lib.hbegp_model_warp(self._h, _lib.dptr(ab))
        return ab

    @staticmethod
    def extend(x_train, y_train, theta, lo=None, hi=None, nu=2.5, ctx=None, row_variance=None):
        """FittedKernel::extend (fit.rs:33-68): one evaluation at fixed theta + K^-1.  Raises where the reference panics.
        row_variance: as in `new` (hbegp_extend_rv_*)."""
        lib = _lib.load()
        ctx = ctx or default_context()
        dtype = np.dtype(x_train.dtype)
        sfx = _suffix(dtype)
        x = _lib.as_c(x_train, dtype)
        y = _lib.as_c(y_train, dtype)
        n, d = x.shape
        theta = _lib.as_c(theta, np.float64)
        lo = None if lo is None else _lib.as_c(lo, np.float64)
        hi = None if hi is None else _lib.as_c(hi, np.float64)
        handle = C.c_void_p()
        rv = _row_variance(row_variance, n)
        tail = (n, d, float(nu), _lib.dptr(theta), _lib.dptr(lo), _lib.dptr(hi), C.byref(handle))
        if rv is None:
            _lib.check(getattr(lib, f"hbegp_extend_{sfx}")(ctx._h, _lib.aptr(x), _lib.aptr(y), *tail))
        else:
            _lib.check(getattr(lib, f"hbegp_extend_rv_{sfx}")(ctx._h, _lib.aptr(x), _lib.aptr(y), _lib.dptr(rv), *tail))
        fk = FittedKernel(handle, dtype, n, d, nu)
        fk.x_train, fk.y_train = x, y
        return fk

    def extend_with(self, x_train, y_train, ctx=None, row_variance=None):
        """FittedKernel::extend (fit.rs:33-68) at this model's theta on data whose leading rows are this model's training
        rows (minimize.rs:629-644 appends the validation samples): reuses the factorisation of the kept 128-blocks, O(n^2 k)
        instead of O(n^3).  Falls back to the full path when the prefix differs.  Sets `.incremental` on the result.
        row_variance: the rows' known noise variances (hbegp_extend_from_rv_*); their prefix must equal this model's too (a
        model without them counts as zeros).  A model that carries them needs the argument."""
        lib = _lib.load()
        ctx = ctx or default_context()
        x = _lib.as_c(x_train, self.dtype)
        y = _lib.as_c(y_train, self.dtype)
        n, d = x.shape
        assert d == self.d
        handle = C.c_void_p()
        inc = C.c_int(0)
        rv = _row_variance(row_variance, n)
        if rv is None:
            ext = getattr(lib, f"hbegp_extend_from_{self._sfx}")
            _lib.check(ext(ctx._h, self._h, _lib.aptr(x), _lib.aptr(y), n, C.byref(handle), C.byref(inc)))
        else:
            ext = getattr(lib, f"hbegp_extend_from_rv_{self._sfx}")
            _lib.check(ext(ctx._h, self._h, _lib.aptr(x), _lib.aptr(y), _lib.dptr(rv), n, C.byref(handle), C.byref(inc)))
        fk = FittedKernel(handle, self.dtype, n, d, self.nu)
        fk.x_train, fk.y_train = x, y
        fk.incremental = bool(inc.value)
        return fk

    def loo(self, want_grad=False):
        """Leave-one-out cross-validation of the model on its own training rows in closed form (hbegp_model_loo_*), in the
        normalised y space: returns (mean[n], var[n], lpd[n], loo) and, with want_grad, d loo / d theta [p] at the model's
        theta.  var is the predictive variance of the observation y_i: it includes the noise (predict() excludes it)."""
        mean = np.zeros(self.n, dtype=self.dtype)
        var = np.zeros(self.n, dtype=self.dtype)
        lpd = np.zeros(self.n, dtype=self.dtype)
        loo = C.c_double()
        grad = np.zeros(self.d + 2) if want_grad else None
        fn = getattr(_lib.load(), f"hbegp_model_loo_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(mean), _lib.aptr(var), _lib.aptr(lpd), C.byref(loo), _lib.dptr(grad)))
        return (mean, var, lpd, loo.value, grad) if want_grad else (mean, var, lpd, loo.value)

    def lgo(self, groups, want_grad=False):
        """Leave-group-out cross-validation of the model on its own training rows in closed form (hbegp_model_lgo_*), in the
        normalised y space.  groups: one int label per row (any values; at most 64 rows share one; None: singletons).  Returns
        (mean[n], var[n], lpd[G], lgo) and, with want_grad, d lgo / d theta [p]; lpd is indexed by the labels' dense ids in order
        of first appearance.  var is the diagonal of the group's predictive covariance of the observations: it includes the noise."""
        g = _group_labels(groups, self.n)
        mean = np.zeros(self.n, dtype=self.dtype)
        var = np.zeros(self.n, dtype=self.dtype)
        lpd = np.zeros(self.n, dtype=self.dtype)
        n_groups = C.c_int(0)
        lgo = C.c_double()
        grad = np.zeros(self.d + 2) if want_grad else None
        fn = getattr(_lib.load(), f"hbegp_model_lgo_{self._sfx}")
        _lib.check(fn(self._h, _iptr(g), _lib.aptr(mean), _lib.aptr(var), _lib.aptr(lpd), C.byref(n_groups), C.byref(lgo), _lib.dptr(grad)))
        lpd = lpd[:n_groups.value].copy()
        return (mean, var, lpd, lgo.value, grad) if want_grad else (mean, var, lpd, lgo.value)

    def predict(self, x, want_variance=True):
        """predict() (predict.rs:7-52): returns (mean, variance or None, n_warn)."""
        lib = _lib.load()
        x = _lib.as_c(x, self.dtype)
        assert x.ndim == 2 and x.shape[1] == self.d
        m = x.shape[0]
        mean = np.zeros(m, dtype=self.dtype)
        var = np.zeros(m, dtype=self.dtype) if want_variance else None
        n_warn = C.c_int(0)
        pred = getattr(lib, f"hbegp_predict_{self._sfx}")
        _lib.check(pred(self._h, _lib.aptr(x), m, _lib.aptr(mean), _lib.aptr(var), C.byref(n_warn)))
        return mean, var, n_warn.value

    def predict_with_gradient(self, x, want_variance=True):
        """predict() plus the gradients w.r.t. the query points (hbegp_predict_grad_*): returns
        (mean[m], var[m] or None, dmean[m, d], dvar[m, d] or None, n_warn), gradients in the units of the feature space."""
        lib = _lib.load()
        x = _lib.as_c(x, self.dtype)
        assert x.ndim == 2 and x.shape[1] == self.d
        m = x.shape[0]
        mean = np.zeros(m, dtype=self.dtype)
        dmean = np.zeros((m, self.d), dtype=self.dtype)
        var = np.zeros(m, dtype=self.dtype) if want_variance else None
        dvar = np.zeros((m, self.d), dtype=self.dtype) if want_variance else None
        n_warn = C.c_int(0)
        fn = getattr(lib, f"hbegp_predict_grad_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(x), m, _lib.aptr(mean), _lib.aptr(var), _lib.aptr(dmean), _lib.aptr(dvar), C.byref(n_warn)))
        return mean, var, dmean, dvar, n_warn.value

    def maximize_ei(self, starts, lo, hi, fmin_normalized, maxeval=150):
        """S bounded L-BFGS runs maximising EI in the normalised y space (hbegp_maximize_ei_*), one batched gradient predict
        per round.  starts: [S, d] inside [lo, hi].  Returns (x[S, d], ei[S], nevals[S]): each run's best point."""
        lib = _lib.load()
        starts = _lib.as_c(np.atleast_2d(starts), self.dtype)
        assert starts.shape[1] == self.d
        S = starts.shape[0]
        lo = _lib.as_c(lo, np.float64)
        hi = _lib.as_c(hi, np.float64)
        assert lo.shape == (self.d,) and hi.shape == (self.d,)
        x = np.zeros((S, self.d), dtype=self.dtype)
        ei = np.zeros(S)
        nevals = np.zeros(S, dtype=np.int32)
        fn = getattr(lib, f"hbegp_maximize_ei_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(starts), S, _lib.dptr(lo), _lib.dptr(hi), float(fmin_normalized), int(maxeval), _lib.aptr(x),
                      _lib.dptr(ei), nevals.ctypes.data_as(C.POINTER(C.c_int))))
        return x, ei, nevals

    def log_ei(self, x, fmin_normalized, want_grad=False):
        """log EI below fmin_normalized at the rows of x (log_constrained_ei without constraints): (lei[m] float64, best), then
        grad[m, d] with want_grad.  Finite where EI itself underflows."""
        return log_constrained_ei(self, [], x, fmin_normalized, None, want_grad=want_grad)

    def maximize_log_ei(self, starts, lo, hi, fmin_normalized, maxeval=150):
        """maximize_ei's runs on log EI (maximize_log_constrained_ei without constraints).  Returns (x[S, d], lei[S], nevals[S])."""
        bounds = np.stack([np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)], axis=1)
        return maximize_log_constrained_ei(self, [], starts, bounds, fmin_normalized, None, maxeval=maxeval)

    def mes(self, x, ystar, want_grad=False, want_posterior=False):
        """Max-value entropy search at the rows of x (hbegp_mes_*), in the normalised y space of a minimised function: the
        information an observation is expected to give about the VALUE of the global minimum, from the sampled minimum values
        ystar [S] (PosteriorPaths.minimize's f_best, or the row minima of sample_posterior over a grid; S <= MES_MAX_SAMPLES).
        Returns (mes[m] float64 >= 0, best) -- best the last index of the maximum, -1 for m = 0 -- then grad[m, d] with want_grad,
        then (mean[m], var[m]) with want_posterior: predict()'s batched numbers bit for bit (predict_with_gradient()'s with
        want_grad).  A sigma = 0 row has mes = 0 and a zero gradient."""
        x = _lib.as_c(np.asarray(x, dtype=self.dtype).reshape(-1, self.d), self.dtype)
        ystar = _lib.as_c(np.asarray(ystar, dtype=np.float64).reshape(-1), np.float64)
        m = x.shape[0]
        val = np.zeros(m)
        best = C.c_int(-1)
        grad = np.zeros((m, self.d), dtype=self.dtype) if want_grad else None
        mean = np.zeros(m, dtype=self.dtype) if want_posterior else None
        var = np.zeros(m, dtype=self.dtype) if want_posterior else None
        fn = getattr(_lib.load(), f"hbegp_mes_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(x), m, _lib.dptr(ystar), len(ystar), _lib.dptr(val), _lib.aptr(grad), C.byref(best),
                      _lib.aptr(mean), _lib.aptr(var)))
        out = (val, best.value)
        if want_grad:
            out += (grad,)
        if want_posterior:
            out += (mean, var)
        return out

    def maximize_mes(self, starts, lo, hi, ystar, maxeval=150):
        """R bounded L-BFGS runs maximising mes() over the box (hbegp_maximize_mes_*), one batched gradient predict per round.
        starts: [R, d] inside [lo, hi].  Returns (x[R, d], mes[R], nevals[R]): each run's best point, never worse than its start;
        mes(x, ystar) reproduces the values bit for bit."""
        starts = _lib.as_c(np.atleast_2d(starts), self.dtype)
        assert starts.shape[1] == self.d
        R = starts.shape[0]
        lo = _lib.as_c(lo, np.float64)
        hi = _lib.as_c(hi, np.float64)
        assert lo.shape == (self.d,) and hi.shape == (self.d,)
        ystar = _lib.as_c(np.asarray(ystar, dtype=np.float64).reshape(-1), np.float64)
        x = np.zeros((R, self.d), dtype=self.dtype)
        val = np.zeros(R)
        nevals = np.zeros(R, dtype=np.int32)
        fn = getattr(_lib.load(), f"hbegp_maximize_mes_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(starts), R, _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(ystar), len(ystar), int(maxeval),
                      _lib.aptr(x), _lib.dptr(val), nevals.ctypes.data_as(C.POINTER(C.c_int))))
        return x, val, nevals

    def confidence_bound(self, x, kappa, want_grad=False, want_posterior=False):
        """The confidence bound mu + kappa sigma at the rows of x (hbegp_confidence_bound_*), in the normalised y space: kappa > 0
        is the reference's predict_confidence_bound, kappa < 0 GP-LCB, kappa = 0 the mean.  Returns (cb[m] float64, best) -- best the
        FIRST index of the minimum, -1 for m = 0 or where every row is NaN -- then grad[m, d] with want_grad, then (mean[m], var[m])
        with want_posterior: predict()'s batched numbers bit for bit (predict_with_gradient()'s with want_grad).  A sigma = 0 row has
        cb = mean and grad = dmean."""
        x = _lib.as_c(np.asarray(x, dtype=self.dtype).reshape(-1, self.d), self.dtype)
        m = x.shape[0]
        val = np.zeros(m)
        best = C.c_int(-1)
        grad = np.zeros((m, self.d), dtype=self.dtype) if want_grad else None
        mean = np.zeros(m, dtype=self.dtype) if want_posterior else None
        var = np.zeros(m, dtype=self.dtype) if want_posterior else None
        fn = getattr(_lib.load(), f"hbegp_confidence_bound_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(x), m, float(kappa), _lib.dptr(val), _lib.aptr(grad), C.byref(best), _lib.aptr(mean),
                      _lib.aptr(var)))
        out = (val, best.value)
        if want_grad:
            out += (grad,)
        if want_posterior:
            out += (mean, var)
        return out

    def minimize_confidence_bound(self, starts, lo, hi, kappa, maxeval=150):
        """S bounded L-BFGS runs minimising confidence_bound() over the box (hbegp_minimize_confidence_bound_*), one batched gradient
        predict per round.  starts: [S, d] inside [lo, hi].  Returns (x[S, d], cb[S], nevals[S]): each run's best point, never worse
        than its start; confidence_bound(x, kappa) reproduces the values bit for bit.  A start with a NaN coordinate fails its own
        run alone: it comes back as it is with cb = +inf."""
        starts = _lib.as_c(np.atleast_2d(starts), self.dtype)
        assert starts.shape[1] == self.d
        S = starts.shape[0]
        lo = _lib.as_c(lo, np.float64)
        hi = _lib.as_c(hi, np.float64)
        assert lo.shape == (self.d,) and hi.shape == (self.d,)
        x = np.zeros((S, self.d), dtype=self.dtype)
        val = np.zeros(S)
        nevals = np.zeros(S, dtype=np.int32)
        fn = getattr(_lib.load(), f"hbegp_minimize_confidence_bound_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(starts), S, _lib.dptr(lo), _lib.dptr(hi), float(kappa), int(maxeval), _lib.aptr(x),
                      _lib.dptr(val), nevals.ctypes.data_as(C.POINTER(C.c_int))))
        return x, val, nevals

    def predict_cov(self, x, jitter=0.0):
        """Joint posterior at the query points (hbegp_predict_cov_*): returns (mean[m], cov[m, m]) in the normalised y space,
        cov = K** + (1e-5 + jitter) I - K*^T K^-1 K* (unclamped; its diagonal is predict()'s variance before clamping)."""
        lib = _lib.load()
        x = _lib.as_c(np.atleast_2d(x), self.dtype)
        assert x.ndim == 2 and x.shape[1] == self.d
        m = x.shape[0]
        mean = np.zeros(m, dtype=self.dtype)
        cov = np.zeros((m, m), dtype=self.dtype)
        fn = getattr(lib, f"hbegp_predict_cov_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(x), m, float(jitter), _lib.aptr(mean), _lib.aptr(cov)))
        return mean, cov

    def sample_posterior(self, x, z, jitter=0.0, want_samples=True):
        """S joint draws mean + L z_s from N(mean, cov) of predict_cov (hbegp_sample_posterior_*), z[S, m] the caller's standard
        normals.  Returns (samples[S, m] or None, argmin[S]): argmin = each draw's smallest entry, ties to the lowest index.
        Raises HbegpError with code NOT_PD when cov is not positive definite (retry with a larger jitter)."""
        lib = _lib.load()
        x = _lib.as_c(np.atleast_2d(x), self.dtype)
        assert x.ndim == 2 and x.shape[1] == self.d
        m = x.shape[0]
        z = _lib.as_c(np.atleast_2d(z), self.dtype)
        assert z.ndim == 2 and z.shape[1] == m, (z.shape, m)
        S = z.shape[0]
        samples = np.zeros((S, m), dtype=self.dtype) if want_samples else None
        argmin = np.zeros(S, dtype=np.int32)
        fn = getattr(lib, f"hbegp_sample_posterior_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(x), m, _lib.aptr(z), S, float(jitter), _lib.aptr(samples),
                      argmin.ctypes.data_as(C.POINTER(C.c_int)), None))
        return samples, argmin

    def select_batch(self, x, k, fmin_normalized, lie=None):
        """Greedy batch selection by EI with fantasised observations (hbegp_select_batch_*), in the normalised y space: k rows of
        x picked one after another, each by the largest EI (ties to the last index), the posterior then conditioned on a noisy
        observation at the pick -- its mean (kriging believer, lie=None) or `lie` (constant liar).  Returns (idx[k] int64, ei[k],
        mean[m], var[m]): mean / var after the k conditionings, var clamped at 0 like predict()."""
        lib = _lib.load()
        x = _lib.as_c(np.atleast_2d(x), self.dtype)
        assert x.ndim == 2 and x.shape[1] == self.d
        m, k = x.shape[0], int(k)
        idx = np.zeros(k, dtype=np.int32)
        ei = np.zeros(k)
        mean = np.zeros(m, dtype=self.dtype)
        var = np.zeros(m, dtype=self.dtype)
        lie_c = None if lie is None else C.byref(C.c_double(float(lie)))
        fn = getattr(lib, f"hbegp_select_batch_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(x), m, k, float(fmin_normalized), lie_c, idx.ctypes.data_as(C.POINTER(C.c_int)), _lib.dptr(ei),
                      _lib.aptr(mean), _lib.aptr(var)))
        return idx.astype(np.int64), ei, mean, var

    def knowledge_gradient(self, x, n_candidates=None, want_posterior=False):
        """Knowledge gradient over a candidate set (hbegp_knowledge_gradient_*), in the normalised y space: for each of the first
        n_candidates rows of x (all of them by default) the expected drop of min_i mean_i over ALL rows of x after one more noisy
        sample there.  It needs no fmin.  Returns (kg[n_candidates] float64, best, imin): best the last index of the maximum of kg
        (-1 without candidates), imin the lowest index of the minimum of the posterior mean -- the row to recommend.  With
        want_posterior also (mean[m], var[m]): predict_cov()'s mean and its diagonal clamped at 0, bit for bit."""
        lib = _lib.load()
        x = _lib.as_c(np.atleast_2d(x), self.dtype)
        assert x.ndim == 2 and x.shape[1] == self.d
        m = x.shape[0]
        mc = m if n_candidates is None else int(n_candidates)
        kg = np.zeros(max(mc, 0))
        best, imin = C.c_int(-1), C.c_int(-1)
        mean = np.zeros(m, dtype=self.dtype) if want_posterior else None
        var = np.zeros(m, dtype=self.dtype) if want_posterior else None
        fn = getattr(lib, f"hbegp_knowledge_gradient_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(x), m, mc, _lib.dptr(kg), C.byref(best), C.byref(imin), _lib.aptr(mean), _lib.aptr(var)))
        if want_posterior:
            return kg, best.value, imin.value, mean, var
        return kg, best.value, imin.value

    def noisy_ei(self, baseline, candidates, z, jitter=0.0, want_details=False):
        """Noisy expected improvement over a candidate set (hbegp_noisy_ei_*; Letham et al. 2019), in the normalised y space: EI
        of every row of candidates [mc, d] averaged over the S joint posterior draws of the latent function at baseline [mb, d]
        that the caller's standard normals z [S, mb] select, each draw with its own incumbent and its own conditioned belief about
        the candidate.  It needs no fmin.  Only the baseline's covariance is factored: candidates may repeat.  Returns
        (nei[mc] float64, best): best the last index of the maximum of nei, -1 without candidates.  With want_details also
        (fmin_draws[S], rho[mc]): each draw's incumbent and the candidates' variance given the baseline's latent values.  Raises
        HbegpError with code NOT_PD when the baseline's covariance is not positive definite (retry with a larger jitter)."""
        lib = _lib.load()
        b = _lib.as_c(np.atleast_2d(baseline), self.dtype)
        assert b.ndim == 2 and b.shape[1] == self.d
        c = np.asarray(candidates, dtype=self.dtype).reshape(-1, self.d)
        mb, mc = b.shape[0], c.shape[0]
        x = _lib.as_c(np.vstack([b, c]), self.dtype)
        z = _lib.as_c(np.atleast_2d(z), self.dtype)
        assert z.ndim == 2 and z.shape[1] == mb, (z.shape, mb)
        S = z.shape[0]
        nei = np.zeros(mc)
        best = C.c_int(-1)
        fmin_draws = np.zeros(S) if want_details else None
        rho = np.zeros(mc) if want_details else None
        fn = getattr(lib, f"hbegp_noisy_ei_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(x), mb + mc, mb, _lib.aptr(z), S, float(jitter), _lib.dptr(nei), C.byref(best),
                      _lib.dptr(fmin_draws), _lib.dptr(rho), None))
        if want_details:
            return nei, best.value, fmin_draws, rho
        return nei, best.value

    def sobol_indices(self, A, B, want_values=False):
        """Variance-based (Sobol) indices of the posterior mean by pick-freeze sampling (hbegp_sobol_*), in the normalised y space:
        A, B [N, d] two independent sample matrices in the feature coordinates of the fit, drawn by the caller.  Returns
        (first[d], total[d], f0, variance): the first-order indices (Saltelli et al. 2010), the total indices (Jansen 1999), the
        mean and the variance of the posterior mean over the 2N rows.  With want_values also (f_a[N], f_b[N], f_ab[d, N]): the
        means at A, at B and at A with column k taken from B, in the element type -- the numbers the indices were formed from."""
        lib = _lib.load()
        A = _lib.as_c(np.atleast_2d(A), self.dtype)
        B = _lib.as_c(np.atleast_2d(B), self.dtype)
        assert A.ndim == 2 and A.shape[1] == self.d and B.shape == A.shape, (A.shape, B.shape)
        N = A.shape[0]
        first, total = np.zeros(self.d), np.zeros(self.d)
        f0, var = C.c_double(), C.c_double()
        f_a = np.zeros(N, dtype=self.dtype) if want_values else None
        f_b = np.zeros(N, dtype=self.dtype) if want_values else None
        f_ab = np.zeros((self.d, N), dtype=self.dtype) if want_values else None
        fn = getattr(lib, f"hbegp_sobol_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(A), _lib.aptr(B), N, _lib.dptr(first), _lib.dptr(total), C.byref(f0), C.byref(var),
                      _lib.aptr(f_a), _lib.aptr(f_b), _lib.aptr(f_ab)))
        if want_values:
            return first, total, f0.value, var.value, f_a, f_b, f_ab
        return first, total, f0.value, var.value

    def main_effects(self, A, grid, want_base=False):
        """Main-effect (partial dependence) curves of the posterior mean (hbegp_main_effects_*; Friedman 2001), in the normalised
        y space: effect[k, g] = the mean over the rows of A [N, d] of the posterior mean with feature k set to grid[k, g].  grid
        [d, G], or [G]: the same values for every feature.  N = 1 gives that row's conditional curves.  Returns effect[d, G]
        (float64); with want_base (effect, f_a[N]): the posterior mean at the rows themselves."""
        lib = _lib.load()
        A = _lib.as_c(np.atleast_2d(A), self.dtype)
        assert A.ndim == 2 and A.shape[1] == self.d, A.shape
        grid = np.asarray(grid, dtype=self.dtype)
        if grid.ndim == 1:
            grid = np.broadcast_to(grid, (self.d, grid.shape[0]))
        grid = _lib.as_c(grid, self.dtype)
        assert grid.ndim == 2 and grid.shape[0] == self.d, grid.shape
        N, G = A.shape[0], grid.shape[1]
        effect = np.zeros((self.d, G))
        f_a = np.zeros(N, dtype=self.dtype) if want_base else None
        fn = getattr(lib, f"hbegp_main_effects_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(A), N, _lib.aptr(grid), G, _lib.dptr(effect), _lib.aptr(f_a)))
        return (effect, f_a) if want_base else effect

    def qei(self, x, z, fmin_normalized, jitter=0.0, want_grad=True, raise_not_pd=False):
        """Batch expected improvement by Monte Carlo (hbegp_qei_*) in the normalised y space: x [B, q, d] (or [q, d]: B = 1) batches
        of q points, z [S, q] the caller's standard normals, shared by every batch.  Returns (qei[B], grad[B, q, d] or None,
        info[B]): a batch whose Sigma is not positive definite has qei NaN, a zero gradient and info = 1 + the failed column; that
        raises HbegpError (code NOT_PD) only with raise_not_pd."""
        lib = _lib.load()
        x = _lib.as_c(x, self.dtype)
        if x.ndim == 2:
            x = x[None]
        assert x.ndim == 3 and x.shape[2] == self.d, x.shape
        B, q = x.shape[0], x.shape[1]
        z = _lib.as_c(np.atleast_2d(z), self.dtype)
        assert z.ndim == 2 and z.shape[1] == q, (z.shape, q)
        qei = np.zeros(B)
        grad = np.zeros((B, q, self.d), dtype=self.dtype) if want_grad else None
        info = np.zeros(B, dtype=np.int32)
        fn = getattr(lib, f"hbegp_qei_{self._sfx}")
        rc = fn(self._h, _lib.aptr(x), B, q, _lib.aptr(z), z.shape[0], float(fmin_normalized), float(jitter), _lib.dptr(qei),
                _lib.aptr(grad), info.ctypes.data_as(C.POINTER(C.c_int)))
        _lib.check(rc, allow=() if raise_not_pd else (_lib.NOT_PD,))
        return qei, grad, info

    def maximize_qei(self, starts, lo, hi, z, fmin_normalized, jitter=0.0, maxeval=150):
        """R bounded L-BFGS ascents of q-EI (hbegp_maximize_qei_*), each over a whole batch of q points in the box [lo, hi], with
        the same z [S, q] every round.  starts: [R, q, d] inside the box.  Returns (x[R, q, d], qei[R], nevals[R]): each run's best
        batch."""
        lib = _lib.load()
        starts = _lib.as_c(starts, self.dtype)
        if starts.ndim == 2:
            starts = starts[None]
        assert starts.ndim == 3 and starts.shape[2] == self.d, starts.shape
        R, q = starts.shape[0], starts.shape[1]
        lo = _lib.as_c(lo, np.float64)
        hi = _lib.as_c(hi, np.float64)
        assert lo.shape == (self.d,) and hi.shape == (self.d,)
        z = _lib.as_c(np.atleast_2d(z), self.dtype)
        assert z.ndim == 2 and z.shape[1] == q, (z.shape, q)
        x = np.zeros_like(starts)
        qei = np.zeros(R)
        nevals = np.zeros(R, dtype=np.int32)
        fn = getattr(lib, f"hbegp_maximize_qei_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(starts), R, q, _lib.dptr(lo), _lib.dptr(hi), _lib.aptr(z), z.shape[0], float(fmin_normalized),
                      float(jitter), int(maxeval), _lib.aptr(x), _lib.dptr(qei), nevals.ctypes.data_as(C.POINTER(C.c_int))))
        return x, qei, nevals

    def sample_paths(self, omega0, phase, w, eps=None):
        """Posterior sample paths (hbegp_paths_create_*) in the normalised y space: draws of the posterior that are functions,
        f_s(x) = phi(x) . w_s + k(x, X) . v_s (pathwise conditioning on a random-Fourier-feature prior draw).  omega0 [F, d] and
        phase [F] from draw_spectral, w [S, F] standard normals, eps [S, n] standard normals or None (no noise draw).  Returns
        a PosteriorPaths, which keeps the model alive."""
        lib = _lib.load()
        omega0 = _lib.as_c(omega0, self.dtype)
        phase = _lib.as_c(phase, self.dtype)
        w = _lib.as_c(np.atleast_2d(w), self.dtype)
        assert omega0.ndim == 2 and omega0.shape[1] == self.d, omega0.shape
        F, S = omega0.shape[0], w.shape[0]
        assert phase.shape == (F,) and w.shape == (S, F), (phase.shape, w.shape)
        if eps is not None:
            eps = _lib.as_c(np.atleast_2d(eps), self.dtype)
            assert eps.shape == (S, self.n), eps.shape
        h = C.c_void_p()
        fn = getattr(lib, f"hbegp_paths_create_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(omega0), _lib.aptr(phase), _lib.aptr(w), _lib.aptr(eps), F, S, C.byref(h)))
        return PosteriorPaths(h, self.dtype, self.d, F, S)

    def release(self):
        if self._h:
            _lib.load().hbegp_model_release(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class WarpedKernel:
    """A model behind a fixed input warp: `.inner` is a FittedKernel on the warped rows u = w(x) (u-space), `.warp` the Warp.  The
    methods below take and return points in x-space; anything else the inner model offers is reached through `.inner` with
    `.warp.apply(x)` rows (gradients it returns are with respect to u: multiply by `.warp.jacobian(x)`)."""

    def __init__(self, inner, warp):
        assert warp.d == inner.d
        self.inner, self.warp = inner, warp
        self.dtype, self.n, self.d, self.nu = inner.dtype, inner.n, inner.d, inner.nu
        self.x_train = None

    lml = property(lambda self: self.inner.lml)
    theta = property(lambda self: self.inner.theta)
    noise = property(lambda self: self.inner.noise)
    amplitude = property(lambda self: self.inner.amplitude)
    length_scale = property(lambda self: self.inner.length_scale)
    y_train = property(lambda self: self.inner.y_train)
    row_variance = property(lambda self: self.inner.row_variance)

    def _u(self, x, dtype=None):
        """The warped rows in the model's element type: hbegp_warp_apply in fp64, rounded once."""
        return self.warp.apply(np.asarray(x, dtype=np.float64).reshape(-1, self.d)).astype(dtype or self.dtype)

    def _x(self, u):
        return self.warp.invert(np.asarray(u, dtype=np.float64)).astype(self.dtype)

    def predict(self, x, want_variance=True):
        return self.inner.predict(self._u(x), want_variance)

    def predict_with_gradient(self, x, want_variance=True):
        """inner.predict_with_gradient at w(x), the gradients multiplied by du/dx: with respect to x.  Where du/dx is infinite (an
        end of [0, 1] whose exponent is below 1) so is the gradient, unless the u-gradient is 0 there (then NaN)."""
        mean, var, dmean, dvar, n_warn = self.inner.predict_with_gradient(self._u(x), want_variance)
        jac = self.warp.jacobian(np.asarray(x, dtype=np.float64).reshape(-1, self.d))
        dmean = (dmean * jac).astype(self.dtype)
        if dvar is not None:
            dvar = (dvar * jac).astype(self.dtype)
        return mean, var, dmean, dvar, n_warn

    def predict_cov(self, x, jitter=0.0):
        return self.inner.predict_cov(self._u(x), jitter)

    def sample_posterior(self, x, z, jitter=0.0, want_samples=True):
        return self.inner.sample_posterior(self._u(x), z, jitter, want_samples)

    def select_batch(self, x, k, fmin_normalized, lie=None):
        return self.inner.select_batch(self._u(x), k, fmin_normalized, lie)

    def confidence_bound(self, x, kappa, want_grad=False, want_posterior=False):
        out = self.inner.confidence_bound(self._u(x), kappa, want_grad, want_posterior)
        if want_grad:
            jac = self.warp.jacobian(np.asarray(x, dtype=np.float64).reshape(-1, self.d))
            out = out[:2] + ((out[2] * jac).astype(self.dtype),) + out[3:]
        return out

    def _box(self, lo, hi):
        """A monotone map per coordinate sends boxes to boxes: the corners' images."""
        lo = np.asarray(lo, dtype=np.float64).reshape(1, self.d)
        hi = np.asarray(hi, dtype=np.float64).reshape(1, self.d)
        return self.warp.apply(lo)[0], self.warp.apply(hi)[0]

    def _maximise(self, method, starts, lo, hi, *args, **kw):
        ulo, uhi = self._box(lo, hi)
        # (the starts in the element type, clipped into the image box: rounding may put a warped start a last place outside it)
        ustarts = np.clip(self._u(np.atleast_2d(starts)), ulo.astype(self.dtype), uhi.astype(self.dtype))
        ulo, uhi = np.minimum(ulo, ustarts.min(axis=0)), np.maximum(uhi, ustarts.max(axis=0))
        u, val, nevals = method(ustarts, ulo, uhi, *args, **kw)
        x = np.clip(self._x(u), np.asarray(lo, dtype=self.dtype), np.asarray(hi, dtype=self.dtype))
        return x, val, nevals

    def maximize_ei(self, starts, lo, hi, fmin_normalized, maxeval=150):
        """inner.maximize_ei over the image of the box, from the warped starts; the points come back through the inverse warp
        (inside [lo, hi]), the values are the u-space maximiser's."""
        return self._maximise(self.inner.maximize_ei, starts, lo, hi, fmin_normalized, maxeval=maxeval)

    def maximize_log_ei(self, starts, lo, hi, fmin_normalized, maxeval=150):
        return self._maximise(self.inner.maximize_log_ei, starts, lo, hi, fmin_normalized, maxeval=maxeval)

    def minimize_confidence_bound(self, starts, lo, hi, kappa, maxeval=150):
        return self._maximise(self.inner.minimize_confidence_bound, starts, lo, hi, kappa, maxeval=maxeval)

    def extend_with(self, x_train, y_train, ctx=None, row_variance=None):
        """inner.extend_with on the rows warped by the fixed warp (the leading rows are this model's: the same function gives the
        same bits, so the incremental path applies)."""
        wk = WarpedKernel(self.inner.extend_with(self._u(x_train), y_train, ctx=ctx, row_variance=row_variance), self.warp)
        wk.x_train = _lib.as_c(x_train, self.dtype)
        return wk

    def extend(self, x_train, y_train, ctx=None, row_variance=None):
        """FittedKernel.extend at this model's theta on the rows warped by the fixed warp (the full path)."""
        dtype = np.dtype(np.asarray(x_train).dtype)  # (the new rows' element type: a model may change it, as FittedKernel.extend allows)
        inner = FittedKernel.extend(self._u(x_train, dtype), _lib.as_c(y_train, dtype), self.inner.theta, nu=self.nu, ctx=ctx,
                                    row_variance=row_variance)
        wk = WarpedKernel(inner, self.warp)
        wk.x_train = _lib.as_c(x_train, dtype)
        return wk

    def release(self):
        self.inner.release()

    def __getattr__(self, name):
        if name.startswith("_") or name in ("inner", "warp"):
            raise AttributeError(name)
        if hasattr(FittedKernel, name):
            raise NotImplementedError(f"WarpedKernel.{name} is not wrapped: call .inner.{name} in u-space with .warp.apply(x) rows "
                                      "(its gradients are with respect to u; .warp.jacobian(x) is du/dx)")
        raise AttributeError(name)


class PosteriorPaths:
    """S posterior sample paths of one model (the hbegp_paths handle; FittedKernel.sample_paths)."""

    def __init__(self, handle, dtype, d, n_features, n_paths):
        self._h = handle
        self.dtype = np.dtype(dtype)
        self.d, self.n_features, self.n_paths = d, n_features, n_paths
        self._sfx = _suffix(dtype)

    def evaluate(self, x, want_grad=True):
        """x [m, d]: every path at the same m points; x [S, m, d]: path s at its own points x[s].  Returns (f[S, m], df[S, m, d]
        or None).  The same (path, point) gives the same bits either way, alone or in a batch."""
        x = _lib.as_c(x, self.dtype)
        assert x.ndim in (2, 3) and x.shape[-1] == self.d, x.shape
        per_path = x.ndim == 3
        if per_path:
            assert x.shape[0] == self.n_paths, x.shape
        m = x.shape[-2]
        f = np.zeros((self.n_paths, m), dtype=self.dtype)
        df = np.zeros((self.n_paths, m, self.d), dtype=self.dtype) if want_grad else None
        fn = getattr(_lib.load(), f"hbegp_paths_eval_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(x), m, 1 if per_path else 0, _lib.aptr(f), _lib.aptr(df)))
        return f, df

    def minimize(self, starts, lo, hi, maxeval=150):
        """Bounded L-BFGS descents of every path from its own starts [S, R, d] (or [R, d]: the same starts for every path) inside
        the box [lo, hi], all S R runs in lockstep.  Returns (x_best[S, d], f_best[S], nevals[S]): per path the best point any of
        its runs evaluated."""
        starts = _lib.as_c(starts, self.dtype)
        if starts.ndim == 2:
            starts = np.ascontiguousarray(np.broadcast_to(starts, (self.n_paths,) + starts.shape))
        assert starts.ndim == 3 and starts.shape[0] == self.n_paths and starts.shape[2] == self.d, starts.shape
        lo = _lib.as_c(lo, np.float64)
        hi = _lib.as_c(hi, np.float64)
        assert lo.shape == (self.d,) and hi.shape == (self.d,)
        x = np.zeros((self.n_paths, self.d), dtype=self.dtype)
        fb = np.zeros(self.n_paths)
        nevals = np.zeros(self.n_paths, dtype=np.int32)
        fn = getattr(_lib.load(), f"hbegp_paths_minimize_{self._sfx}")
        _lib.check(fn(self._h, _lib.aptr(starts), starts.shape[1], _lib.dptr(lo), _lib.dptr(hi), int(maxeval), _lib.aptr(x), _lib.dptr(fb),
                      nevals.ctypes.data_as(C.POINTER(C.c_int))))
        return x, fb, nevals

    def release(self):
        if self._h:
            _lib.load().hbegp_paths_release(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def draw_spectral(nu, n_features, d, rng):
    """Random Fourier frequencies and phases of the Matern-nu kernel at unit length scale, from rng.standard_normal and
    rng.uniform only: omega0 [F, d] and phase [F] in [0, 2 pi).  nu = inf (the squared-exponential kernel): standard normals.
    Matern nu (2 nu in {1, 3, 5}): a multivariate Student-t with 2 nu degrees of freedom -- a standard normal vector divided by
    sqrt(chi2_{2 nu} / (2 nu)), the chi-square being a sum of 2 nu squared standard normals."""
    F, d = int(n_features), int(d)
    z = np.asarray(rng.standard_normal((F, d)), dtype=np.float64)
    if math.isinf(nu):
        omega0 = z
    else:
        dof = int(round(2 * nu))
        if dof not in (1, 3, 5) or abs(2 * nu - dof) > 1e-12:
            raise ValueError("nu must be 0.5, 1.5, 2.5 or inf")
        g = (np.asarray(rng.standard_normal((F, dof)), dtype=np.float64) ** 2).sum(axis=1)
        omega0 = z * np.sqrt(dof / g)[:, None]
    phase = 2.0 * math.pi * np.asarray(rng.uniform(0.0, 1.0, F), dtype=np.float64)
    return omega0, phase


def _ehvi_args(models, front, ref):
    """(handle array, suffix, dtype, d, front [P, 2] float64, ref [2] float64) of a two-objective call."""
    models = list(models)
    handles = (C.c_void_p * max(len(models), 1))(*[fk._h for fk in models])
    fk = models[0]
    front = _lib.as_c(np.asarray(front if front is not None else [], dtype=np.float64).reshape(-1, 2), np.float64)
    ref = _lib.as_c(np.asarray(ref, dtype=np.float64).reshape(2), np.float64)
    return models, handles, fk._sfx, fk.dtype, fk.d, front, ref


def ehvi(models, x, front, ref, want_grad=False, want_posterior=False):
    """Expected hypervolume improvement of two minimised objectives (hbegp_ehvi_*), in the models' normalised y spaces:
    models = (objective 0, objective 1), two FittedKernels of the same d, element type and device, taken as independent;
    front [P, 2] the points reached so far, in any order (dominated points, duplicates and points outside the box change nothing);
    ref [2] the reference point.  Returns (ehvi[m] float64, best) -- best the last index of the maximum, -1 for m = 0 -- then
    grad[m, d] with want_grad, then (mean[m, 2], var[m, 2]) with want_posterior: predict()'s numbers, bit for bit."""
    models, handles, sfx, dtype, d, front, ref = _ehvi_args(models, front, ref)
    x = _lib.as_c(np.asarray(x, dtype=dtype).reshape(-1, d), dtype)
    m = x.shape[0]
    val = np.zeros(m)
    best = C.c_int(-1)
    grad = np.zeros((m, d), dtype=dtype) if want_grad else None
    mean = np.zeros((m, 2), dtype=dtype) if want_posterior else None
    var = np.zeros((m, 2), dtype=dtype) if want_posterior else None
    fn = getattr(_lib.load(), f"hbegp_ehvi_{sfx}")
    _lib.check(fn(handles, len(models), _lib.aptr(x), m, _lib.dptr(front), front.shape[0], _lib.dptr(ref), _lib.dptr(val),
                  _lib.aptr(grad), C.byref(best), _lib.aptr(mean), _lib.aptr(var)))
    out = (val, best.value)
    if want_grad:
        out += (grad,)
    if want_posterior:
        out += (mean, var)
    return out


def maximize_ehvi(models, starts, bounds, front, ref, maxeval=150):
    """S bounded L-BFGS runs maximising ehvi() over the box (hbegp_maximize_ehvi_*), one batched gradient predict per model and
    round.  starts: [S, d] inside the box; bounds: d pairs (lo, hi).  Returns (x[S, d], ehvi[S], nevals[S]): each run's best
    point, never worse than its start; ehvi(models, x, front, ref) reproduces the values bit for bit."""
    models, handles, sfx, dtype, d, front, ref = _ehvi_args(models, front, ref)
    starts = _lib.as_c(np.atleast_2d(starts), dtype)
    assert starts.shape[1] == d
    S = starts.shape[0]
    bounds = np.asarray(bounds, dtype=np.float64).reshape(d, 2)
    lo = _lib.as_c(bounds[:, 0], np.float64)
    hi = _lib.as_c(bounds[:, 1], np.float64)
    x = np.zeros((S, d), dtype=dtype)
    val = np.zeros(S)
    nevals = np.zeros(S, dtype=np.int32)
    fn = getattr(_lib.load(), f"hbegp_maximize_ehvi_{sfx}")
    _lib.check(fn(handles, len(models), _lib.aptr(starts), S, _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(front), front.shape[0],
                  _lib.dptr(ref), int(maxeval), _lib.aptr(x), _lib.dptr(val), nevals.ctypes.data_as(C.POINTER(C.c_int))))
    return x, val, nevals


def _ehvi_nd_args(models, front, ref):
    """(models, handle array, suffix, dtype, d, front [P, n_obj] float64, ref [n_obj] float64) of an n_obj-objective call."""
    models = list(models)
    n_obj = max(len(models), 1)
    handles = (C.c_void_p * n_obj)(*[fk._h for fk in models])
    fk = models[0]
    front = _lib.as_c(np.asarray(front if front is not None else [], dtype=np.float64).reshape(-1, n_obj), np.float64)
    ref = _lib.as_c(np.asarray(ref, dtype=np.float64).reshape(n_obj), np.float64)
    return models, handles, fk._sfx, fk.dtype, fk.d, front, ref


def ehvi_nd(models, x, front, ref, want_grad=False, want_posterior=False):
    """Expected hypervolume improvement of n_obj = len(models) = 2, 3 or 4 minimised objectives (hbegp_ehvi_nd_*), in the models'
    normalised y spaces: models = (objective 0, ..), FittedKernels of the same d, element type and device, taken as independent;
    front [P, n_obj] the points reached so far, in any order (dominated points, duplicates and points outside the box change
    nothing); ref [n_obj] the reference point.  Returns what ehvi() returns, with mean[m, n_obj] and var[m, n_obj].  A front whose
    free region splits into more than _lib.EHVI_ND_MAX_BOXES boxes is refused (HbegpError, ENOMEM)."""
    models, handles, sfx, dtype, d, front, ref = _ehvi_nd_args(models, front, ref)
    n_obj = len(models)
    x = _lib.as_c(np.asarray(x, dtype=dtype).reshape(-1, d), dtype)
    m = x.shape[0]
    val = np.zeros(m)
    best = C.c_int(-1)
    grad = np.zeros((m, d), dtype=dtype) if want_grad else None
    mean = np.zeros((m, n_obj), dtype=dtype) if want_posterior else None
    var = np.zeros((m, n_obj), dtype=dtype) if want_posterior else None
    fn = getattr(_lib.load(), f"hbegp_ehvi_nd_{sfx}")
    _lib.check(fn(handles, n_obj, _lib.aptr(x), m, _lib.dptr(front), front.shape[0], _lib.dptr(ref), _lib.dptr(val),
                  _lib.aptr(grad), C.byref(best), _lib.aptr(mean), _lib.aptr(var)))
    out = (val, best.value)
    if want_grad:
        out += (grad,)
    if want_posterior:
        out += (mean, var)
    return out


def maximize_ehvi_nd(models, starts, bounds, front, ref, maxeval=150):
    """S bounded L-BFGS runs maximising ehvi_nd() over the box (hbegp_maximize_ehvi_nd_*), one batched gradient predict per model
    and round; the front is decomposed once.  starts: [S, d] inside the box; bounds: d pairs (lo, hi).  Returns (x[S, d], ehvi[S],
    nevals[S]): each run's best point, never worse than its start; ehvi_nd(models, x, front, ref) reproduces the values bit for
    bit."""
    models, handles, sfx, dtype, d, front, ref = _ehvi_nd_args(models, front, ref)
    starts = _lib.as_c(np.atleast_2d(starts), dtype)
    assert starts.shape[1] == d
    S = starts.shape[0]
    bounds = np.asarray(bounds, dtype=np.float64).reshape(d, 2)
    lo = _lib.as_c(bounds[:, 0], np.float64)
    hi = _lib.as_c(bounds[:, 1], np.float64)
    x = np.zeros((S, d), dtype=dtype)
    val = np.zeros(S)
    nevals = np.zeros(S, dtype=np.int32)
    fn = getattr(_lib.load(), f"hbegp_maximize_ehvi_nd_{sfx}")
    _lib.check(fn(handles, len(models), _lib.aptr(starts), S, _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(front), front.shape[0],
                  _lib.dptr(ref), int(maxeval), _lib.aptr(x), _lib.dptr(val), nevals.ctypes.data_as(C.POINTER(C.c_int))))
    return x, val, nevals


def ehvi_boxes(front, ref):
    """The box decomposition hbegp_ehvi_nd_* sums over (hbegp_debug_ehvi_boxes; host only, no device): front [P, n_obj], ref [n_obj].
    Returns (thr, boxes): thr a list of n_obj float64 arrays -- -inf, the reduced front's distinct coordinates ascending, r_k -- and
    boxes [n_boxes, n_obj, 2] int32, per box and objective the indices (l, u) into thr[k] (0 = -inf)."""
    ref = _lib.as_c(np.asarray(ref, dtype=np.float64).reshape(-1), np.float64)
    n_obj = len(ref)
    front = _lib.as_c(np.asarray(front if front is not None else [], dtype=np.float64).reshape(-1, max(n_obj, 1)), np.float64)
    fn = _lib.load().hbegp_debug_ehvi_boxes
    ip = C.POINTER(C.c_int)
    counts = np.zeros(max(n_obj, 1), dtype=np.int32)
    nb = C.c_int(0)
    _lib.check(fn(_lib.dptr(front), front.shape[0], n_obj, _lib.dptr(ref), counts.ctypes.data_as(ip), None, 0, C.byref(nb), None, 0))
    thr = np.zeros(int(counts.sum()))
    boxes = np.zeros((nb.value, n_obj, 2), dtype=np.int32)
    _lib.check(fn(_lib.dptr(front), front.shape[0], n_obj, _lib.dptr(ref), counts.ctypes.data_as(ip), _lib.dptr(thr), len(thr),
                  C.byref(nb), boxes.ctypes.data_as(ip), nb.value))
    return np.split(thr, np.cumsum(counts)[:-1]), boxes


def _cei_args(objective, constraints, limits):
    """(constraints as a list, their handle array, limits [C] float64) of a constrained-EI call."""
    constraints = list(constraints)
    handles = (C.c_void_p * max(len(constraints), 1))(*[fk._h for fk in constraints])
    limits = _lib.as_c(np.asarray(limits if limits is not None else [], dtype=np.float64).reshape(-1), np.float64)
    if len(limits) != len(constraints):
        raise ValueError(f"{len(constraints)} constraint models but {len(limits)} limits")
    return constraints, handles, limits


def _constrained_ei(symbol, objective, constraints, x, fmin_normalized, limits, want_grad, want_details):
    """The call behind constrained_ei and log_constrained_ei: `symbol` without its element-type suffix."""
    constraints, handles, limits = _cei_args(objective, constraints, limits)
    dtype, d, K = objective.dtype, objective.d, 1 + len(constraints)
    x = _lib.as_c(np.asarray(x, dtype=dtype).reshape(-1, d), dtype)
    m = x.shape[0]
    val = np.zeros(m)
    best = C.c_int(-1)
    grad = np.zeros((m, d), dtype=dtype) if want_grad else None
    ei = np.zeros(m) if want_details else None
    pof = np.zeros(m) if want_details else None
    mean = np.zeros((m, K), dtype=dtype) if want_details else None
    var = np.zeros((m, K), dtype=dtype) if want_details else None
    fn = getattr(_lib.load(), f"{symbol}_{objective._sfx}")
    _lib.check(fn(objective._h, handles, len(constraints), _lib.aptr(x), m, float(fmin_normalized), _lib.dptr(limits), _lib.dptr(val),
                  _lib.aptr(grad), C.byref(best), _lib.dptr(ei), _lib.dptr(pof), _lib.aptr(mean), _lib.aptr(var)))
    out = (val, best.value)
    if want_grad:
        out += (grad,)
    if want_details:
        out += (ei, pof, mean, var)
    return out


def constrained_ei(objective, constraints, x, fmin_normalized, limits, want_grad=False, want_details=False):
    """Constrained expected improvement (hbegp_constrained_ei_*), in the models' normalised y spaces: the EI of the minimised
    `objective` below fmin_normalized times the probability that every constraints[k] stays at or below limits[k].  objective and
    constraints are FittedKernels of the same d, element type and device, taken as independent; at most CEI_MAX_CONSTRAINTS
    constraints.  fmin_normalized = math.inf: no feasible point is known, EI counts as 1 and cei is the probability of
    feasibility.  Returns (cei[m] float64, best) -- best the last index of the maximum, -1 for m = 0 -- then grad[m, d] with
    want_grad, then (ei[m], pof[m], mean[m, 1 + C], var[m, 1 + C]) with want_details: the objective first, predict()'s numbers
    bit for bit."""
    return _constrained_ei("hbegp_constrained_ei", objective, constraints, x, fmin_normalized, limits, want_grad, want_details)


def log_constrained_ei(objective, constraints, x, fmin_normalized, limits, want_grad=False, want_details=False):
    """The logarithm of constrained_ei by stable forms (hbegp_log_constrained_ei_*): lcei = lei + lpof with lei = log EI (0 for
    fmin_normalized = math.inf) and lpof the sum of the log feasibility probabilities.  Value and gradient stay finite and
    informative where constrained_ei underflows to exactly 0 (|z| beyond 38); a sigma = 0 row on the wrong side is -inf.
    Arguments and returns as constrained_ei: (lcei[m] float64, best), then grad[m, d] -- the gradient of lcei -- with want_grad,
    then (lei[m], lpof[m], mean[m, 1 + C], var[m, 1 + C]) with want_details.  Without constraints it is log EI."""
    return _constrained_ei("hbegp_log_constrained_ei", objective, constraints, x, fmin_normalized, limits, want_grad, want_details)


def _maximize_constrained_ei(symbol, objective, constraints, starts, bounds, fmin_normalized, limits, maxeval):
    """The call behind maximize_constrained_ei and maximize_log_constrained_ei: `symbol` without its element-type suffix."""
    constraints, handles, limits = _cei_args(objective, constraints, limits)
    dtype, d = objective.dtype, objective.d
    starts = _lib.as_c(np.atleast_2d(starts), dtype)
    assert starts.shape[1] == d
    S = starts.shape[0]
    bounds = np.asarray(bounds, dtype=np.float64).reshape(d, 2)
    lo = _lib.as_c(bounds[:, 0], np.float64)
    hi = _lib.as_c(bounds[:, 1], np.float64)
    x = np.zeros((S, d), dtype=dtype)
    val = np.zeros(S)
    nevals = np.zeros(S, dtype=np.int32)
    fn = getattr(_lib.load(), f"{symbol}_{objective._sfx}")
    _lib.check(fn(objective._h, handles, len(constraints), _lib.aptr(starts), S, _lib.dptr(lo), _lib.dptr(hi), float(fmin_normalized),
                  _lib.dptr(limits), int(maxeval), _lib.aptr(x), _lib.dptr(val), nevals.ctypes.data_as(C.POINTER(C.c_int))))
    return x, val, nevals


def maximize_constrained_ei(objective, constraints, starts, bounds, fmin_normalized, limits, maxeval=150):
    """S bounded L-BFGS runs maximising constrained_ei() over the box (hbegp_maximize_constrained_ei_*), one batched gradient
    predict per model and round.  starts: [S, d] inside the box; bounds: d pairs (lo, hi).  Returns (x[S, d], cei[S], nevals[S]):
    each run's best point, never worse than its start; constrained_ei(objective, constraints, x, ...) reproduces the values bit
    for bit."""
    return _maximize_constrained_ei("hbegp_maximize_constrained_ei", objective, constraints, starts, bounds, fmin_normalized, limits,
                                    maxeval)


def maximize_log_constrained_ei(objective, constraints, starts, bounds, fmin_normalized, limits, maxeval=150):
    """maximize_constrained_ei on log_constrained_ei (hbegp_maximize_log_constrained_ei_*): the runs move where every start has
    cei = 0 in plain space.  Returns (x[S, d], lcei[S], nevals[S]); log_constrained_ei at x reproduces the values bit for bit.
    A row at -inf counts as a failed evaluation."""
    return _maximize_constrained_ei("hbegp_maximize_log_constrained_ei", objective, constraints, starts, bounds, fmin_normalized,
                                    limits, maxeval)


def minimize_by_gradient(objective, x0, bounds, maxeval=150):
    """util::minimize_by_gradient (gradmin.rs:35-60) through the library's bounded L-BFGS."""
    lib = _lib.load()
    x = _lib.as_c(np.array(x0, dtype=np.float64), np.float64).copy()
    n = len(x)
    lo = _lib.as_c([b[0] for b in bounds], np.float64)
    hi = _lib.as_c([b[1] for b in bounds], np.float64)

    def cb(xp, gp, _user):
        xs = np.ctypeslib.as_array(xp, shape=(n,))
        f, g = objective(xs.copy())
        gv = np.ctypeslib.as_array(gp, shape=(n,))
        gv[:] = g
        return float(f)

    fn = _lib.OBJECTIVE_FN(cb)
    f = lib.hbegp_minimize_by_gradient(fn, None, _lib.dptr(x), _lib.dptr(lo), _lib.dptr(hi), n, maxeval)
    return f, x
