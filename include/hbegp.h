/*
 * hbegp.h — C ABI of the MI355X-native Gaussian-process surrogate engine (libhbegp.so).
 *
 * Drop-in boundary for hbetune's `src/gpr` hot path.  The reference has no C ABI of its own; its seam
 * is the pair of Rust traits `Estimator<A>` / `SurrogateModel<A>` (src/core/surrogate_model.rs:6-65),
 * implemented for the CPU by `EstimatorGPR` / `SurrogateModelGPR<A>` (src/core/gpr.rs:54-63, 215-338),
 * which call `FittedKernel::new/extend` (src/gpr/fit.rs:18-68) and `predict` (src/gpr/predict.rs:7-52).
 * Every entry point below replaces one of those calls; the Rust-side binding a maintainer would add is
 * shown in INTEGRATION.md.
 *
 * Conventions
 *   - Plain C: host pointers and sizes only, no callbacks, no exceptions cross the boundary.
 *   - Element type A is f64 (default) or f32 (`--use-32`, src/bin/hbetune/main.rs:240-244); entry points
 *     that move arrays of A come in `_f64` / `_f32` pairs.  Hyper-parameters, bounds, lml and its
 *     gradient are always f64 (src/gpr/lml.rs:9-10, src/util/bounded_value.rs).
 *   - X is n x d row-major, features in [0,1] (src/core/space.rs:141-159); y has n entries and is
 *     already y-normalised by the caller (src/core/ynormalize.rs stays in the adapter).
 *   - Kernel = ConstantKernel(c) * Matern(nu, ell_1..ell_d) + white noise s2 (src/core/gpr.rs:51, 402-427),
 *     nu in {0.5, 1.5, 2.5} (src/gpr/matern_kernel.rs:65-80).  Extension: nu = +infinity selects the squared-exponential
 *     kernel exp(-r^2/2) (the reference has none: matern_kernel.rs:79 is unimplemented! for other nu; oracle: sklearn RBF).
 *   - theta is log-space, p = d + 2 entries ordered [ln s2, ln c, ln ell_1 .. ln ell_d]
 *     (src/gpr/fit.rs:140-144; gradient order src/gpr/lml.rs:67-68).  `lo`/`hi` are the linear-space
 *     bounds in the same order.  Kernel parameters are clamped into their bounds after exp()
 *     (`with_clamped_theta`, src/gpr/fit.rs:95); the noise is not (src/gpr/fit.rs:96).
 *   - Return value: one of HBEGP_* below.  Negative = usage/runtime error (see hbegp_last_error()).
 *   - All compute runs in hand-written HIP kernels on gfx950; there is no CPU fallback.  Without a GPU
 *     hbegp_ctx_create() fails with HBEGP_ENODEV.
 *   - Accuracy against the reference's CPU arithmetic (ndarray + LAPACK potrf/potrs/potri), relative to max(1, scale), the
 *     predictive variance relative to the amplitude: f64 1e-8 on lml, gradient, alpha, K^-1, mean and variance.  Where cond(K)
 *     puts LAPACK's own digits beyond that (the corners of the box an optimiser visits: cond(K) ~ 1e9 .. 1e12) the statement is
 *     made against the truth (an extended-precision referee, oracle/referee.c: kernel matrix in binary128, refined solves):
 *     |result - truth| <= max(1e-8, 2 |LAPACK - truth|) -- the engine is at most twice as far from the truth as the reference's
 *     own arithmetic.  Measured at the end of a fit of config M (cond(K) = 6.7e11): lml 7e-9 (LAPACK 1e-9), mean 1.9e-8 (2.5e-8),
 *     variance 2e-14 (LAPACK's K^-1 form: 3.9e-6).
 *     f32 (`--use-32`) 1e-4 on lml, gradient, mean and variance; alpha and K^-1 meet 1e-4 up to cond(K) ~ 7e4 on the paths a
 *     caller gets by default (the task queue's right-looking order from n = 641 on, for fits and single evaluations alike;
 *     the single launch up to n = 128), and max(1e-4, 2 x the deviation of LAPACK's own f32 path) otherwise -- between
 *     n = 129 and n = 640 f32 panel solves go through the explicit inverse of the whole left half, which costs K^-1 ~20 %
 *     more deviation at cond(K) = 7e4 (1.2e-4; LAPACK f32: 1.7e-4).  tests/test_gpu_fullsize.py holds both statements.
 *     Beyond cond(K) ~ 1e5 every f32 result is dominated by the rounding of the kernel matrix itself (tests/parity_rules.py).
 *   - Threads: the library is re-entrant per context.  Any number of host threads may call hbegp_fit_*, hbegp_extend_* and
 *     hbegp_predict_* on ONE context at the same time (replicas: independent fits side by side on one GPU); every fit owns its
 *     workspaces, streams and graphs, nothing on those paths uses the null stream or synchronises the whole device, and the
 *     launches are sized for the optimiser runs in flight over all fits of the process.  A concurrent fit returns the same
 *     bits as the same fit alone.  One hbegp_problem / one hbegp_model must not be used from two threads at once (a model
 *     serialises its own predictions).
 *   - Problems of at most 128 rows and 32 features (the reference's own regime, src/core/minimize.rs:118-120) take a path of
 *     their own: one evaluation is one launch that keeps K, L, L^-1, K^-1 and alpha in a compute unit's LDS, and one optimiser
 *     run of a fit is one persistent launch (evaluation + bounded L-BFGS step + capture on the device); the host only starts
 *     the runs side by side and collects.  Same entry points, same contracts; HBEGP_SMALL=0 / HBEGP_SMALL_FIT=0 select the
 *     general path / the host-driven optimiser for comparison.  Such fits issued by several threads at the same time share
 *     their launches (one grid carries the runs of all fits that arrive within a few milliseconds of each other; a thread
 *     alone never waits), and the host-side phases of such fits take turns while at most 16 threads are inside them (the HIP
 *     runtime's locks do worse): 16 native threads reach ~1,140 fits/s at n = 128 where one reaches 95, each fit bit for bit its
 *     solo result.
 */
#ifndef HBEGP_H
#define HBEGP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBEGP_VERSION 200 /* 0.2.0: hbegp_fit_options starts with struct_size (the struct may grow at its end without breaking
                             callers built against an older header); hbegp_problem_debug_get which = 3, 4 */

enum {
  HBEGP_OK = 0,
  HBEGP_NOT_PD = 1,     /* Cholesky failed: reference returns None -> objective +inf, gradient 0 (lml.rs:47-50, fit.rs:105-112) */
  HBEGP_ALL_FAILED = 2, /* every evaluation of a fit failed: the reference would panic (fit.rs:161) */
  HBEGP_EINVAL = -1,
  HBEGP_EHIP = -2,      /* a HIP call failed */
  HBEGP_ENODEV = -3,    /* no usable gfx950 device */
  HBEGP_ENOMEM = -4
};

typedef struct hbegp_ctx hbegp_ctx;         /* devices, streams, workspace pools */
typedef struct hbegp_problem hbegp_problem; /* X, y resident on the device(s) + evaluation workspaces */
typedef struct hbegp_model hbegp_model;     /* fitted model: mirrors FittedKernel (fit.rs:6-12) + x_train */

/* ---- context ------------------------------------------------------------------------------------ */
int hbegp_version(void);
/* Number of visible gfx950 devices (0 when there is none); does not initialise a context. */
int hbegp_device_count(void);
/* n_devices > 0; device_ids may be NULL (= 0..n_devices-1).  One process may own several GPUs: optimiser
 * runs of one fit are sharded run r -> device r mod n_devices (restart axis, src/util/gradmin.rs:19-31). */
int hbegp_ctx_create(int n_devices, const int* device_ids, hbegp_ctx** out);
void hbegp_ctx_destroy(hbegp_ctx* ctx);
/* Thread-local text of the last error raised through any handle (never NULL). */
const char* hbegp_last_error(void);

/* ---- problem: upload X, y once, evaluate many theta (the L-BFGS inner loop, fit.rs:93-134) ------- */
/* n_slots >= 1 independent evaluation workspaces per device (one optimiser run uses one slot). */
int hbegp_problem_create_f64(hbegp_ctx* ctx, const double* X, const double* y, int n, int d, double nu,
                             int n_slots, hbegp_problem** out);
int hbegp_problem_create_f32(hbegp_ctx* ctx, const float* X, const float* y, int n, int d, double nu,
                             int n_slots, hbegp_problem** out);
void hbegp_problem_destroy(hbegp_problem* prob);

/* One evaluation of lml_with_gradient (src/gpr/lml.rs:29-79) on slot `slot` of device index `dev`.
 * theta/lo/hi as above (lo/hi may be NULL = no clamping).  grad may be NULL (skips the gradient pass).
 * Returns HBEGP_OK, or HBEGP_NOT_PD (then *lml = -inf and grad = 0). */
int hbegp_problem_eval(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo,
                       const double* hi, double* lml, double* grad);

/* The leave-one-out log pseudo-likelihood (see hbegp_model_loo_* below) at theta as an evaluation, next to hbegp_problem_eval:
 * the slot's normal evaluation at theta (without the lml gradient), then the leave-one-out tail on its results.  theta/lo/hi and
 * the clamping as hbegp_problem_eval; grad[p] (may be NULL: skips the n^3 product and the trace) = d loo / d theta in the order and
 * with the clamping convention of the gradient hbegp_problem_eval returns (a clamped parameter's entry is the derivative at the
 * clamped value).  Returns HBEGP_NOT_PD with *loo = -inf and grad = 0 where hbegp_problem_eval does.  Afterwards the slot is in
 * the state hbegp_problem_eval at that theta leaves it in: hbegp_problem_get_* returns the same bits, and a following
 * hbegp_problem_eval is undisturbed.  Every evaluation path (the single launch of at most 128 rows, the launch path, the task
 * queue; f64 and f32) leaves L^-1 in the slot, so m_i is always the column sum of squares of L^-1, never the diagonal of the stored
 * K^-1.  Two work matrices of n_p^2 elements are borrowed for a call with a gradient (HBEGP_ENOMEM as in hbegp_predict_cov_*).
 * Slots may be evaluated from several threads at once, one thread per slot; the same call gives the same bits. */
int hbegp_problem_eval_loo(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                           double* loo, double* grad);

/* The leave-group-out log predictive density (see hbegp_model_lgo_* below) at theta as an evaluation: hbegp_problem_eval_loo with
 * the groups group[n] (NULL: singletons).  The slot's normal evaluation without the lml gradient, then the leave-group-out tail on
 * the slot's stream; clamping, grad, HBEGP_NOT_PD, the slot's state afterwards and threading as hbegp_problem_eval_loo. */
int hbegp_problem_eval_lgo(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                           const int* group, double* lgo, double* grad);

/* ---- input warping -----------------------------------------------------------------------------------
 * The Kumaraswamy warp of feature k, u = 1 - (1 - x^a_k)^b_k, maps [0, 1] onto itself monotonically (a = b = 1: the identity).
 * ab = [a_1..a_d, b_1..b_d] in linear space.  Pure host fp64, no context: U[m*d] = the warped rows, dU_dlna / dU_dlnb = du/dln a,
 * du/dln b, dU_dx = du/dx, each [m*d] and each may be NULL.  At x = 0 and x = 1: u is exactly 0 / 1 and both parameter derivatives
 * are exactly 0 (the limits); du/dx = a b x^(a-1) (1 - x^a)^(b-1) is +inf at an end whose exponent (a at 0, b at 1) is below 1.
 * hbegp_warp_invert is the closed-form inverse x = (1 - (1 - u)^(1/b))^(1/a).  HBEGP_EINVAL for a parameter that is not finite and
 * positive and for an input outside [0, 1] (NaN included); nothing is written then.  The device (hbegp_problem_eval_warped) warps
 * with the same function: the rows it evaluates are bit for bit hbegp_warp_apply's U rounded once to the element type. */
int hbegp_warp_apply(const double* ab, int d, const double* X, int m, double* U, double* dU_dlna, double* dU_dlnb, double* dU_dx);
int hbegp_warp_invert(const double* ab, int d, const double* U, int m, double* X);

/* hbegp_problem_eval plus the gradient of the lml with respect to the training inputs: gx[n*d], row-major,
 *   gx[i][k] = d lml / d x_ik = sum_j (alpha alpha^T - K^-1)_ij c psi(r_ij) (x_ik - x_jk) / ell_k^2,  psi = phi'(r) / r,
 * always fp64, at the clamped parameters the evaluation ran with.  Terms with r = 0 (the diagonal, duplicate rows) contribute 0, as
 * in hbegp_predict_grad_*; neither the noise nor known row variances enter.  The slot's normal evaluation (lml, and grad[p] when
 * it is not NULL: the bits hbegp_problem_eval returns), then the tail on the slot's stream.  Clamping, HBEGP_NOT_PD (lml = -inf,
 * grad and gx zero), the state the slot is left in, the evaluation paths and element types covered and the threading contract are
 * hbegp_problem_eval_loo's.  The same call gives the same bits. */
int hbegp_problem_eval_xgrad(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                             double* lml, double* grad, double* gx);

/* The warped objective lml(w(X; a, b), theta) and its gradient grad[p + 2d] (may be NULL: skips the gradient and the tail): the p
 * entries of hbegp_problem_eval at the warped rows, then d lml / d ln a_k and d lml / d ln b_k.  Only for a problem created with
 * n_slots == 1 whose features lie in [0, 1] (checked on first use): the call rewrites the device's feature buffer, which a
 * problem's slots share -- HBEGP_EINVAL otherwise, with a message that says so.  On first use the problem keeps the caller's rows
 * in a second buffer; every call warps them into the feature buffer, evaluates, runs the hbegp_problem_eval_xgrad tail and the chain
 * rule, and copies the caller's rows back, all ordered on the slot's stream: a later hbegp_problem_eval returns the bits it returned
 * before.  HBEGP_NOT_PD: lml = -inf, grad zero.  hbegp_problem_debug_rows_* copies out the rows [n*d] the device's feature buffer
 * holds at the moment (tests; with HBEGP_WARP_DEBUG_KEEP=1 in the environment a call leaves the warped rows there instead of the
 * caller's, and the next call without it puts the caller's back). */
int hbegp_problem_eval_warped(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo, const double* hi,
                              const double* ab, double* lml, double* grad);
int hbegp_problem_debug_rows_f64(hbegp_problem* prob, int dev, double* out);
int hbegp_problem_debug_rows_f32(hbegp_problem* prob, int dev, float* out);

/* Copy out device results of the most recent successful evaluation on (dev, slot); any pointer may be NULL.
 * alpha[n]; kinv[n*n] full symmetric row-major (what invc() returns, lml.rs:62); ldiag[n] = diag(L). */
int hbegp_problem_get_f64(hbegp_problem* prob, int dev, int slot, double* alpha, double* kinv, double* ldiag);
int hbegp_problem_get_f32(hbegp_problem* prob, int dev, int slot, float* alpha, float* kinv, float* ldiag);

/* Kernel-matrix assembly only: K = c*Matern(X,X) + s2*I, full symmetric n*n row-major (lml.rs:40-44). */
int hbegp_problem_kmat_f64(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo,
                           const double* hi, double* K);
int hbegp_problem_kmat_f32(hbegp_problem* prob, int dev, int slot, const double* theta, const double* lo,
                           const double* hi, float* K);

/* Timed evaluations for bench.py: runs `reps` evaluations at theta on (dev, slot) bracketed by hipEvents on the
 * slot's stream.  phase_ms (may be NULL) receives per-phase averages measured with events in eager mode:
 * [0] kmat, [1] chol+trtri GEMM launches (sum), [2] leaf (diag-block) launches (sum), [3] lauum GEMM,
 * [4] alpha/lml reductions, [5] gradtrace, [6] whole evaluation (graph replay), [7] number of GEMM launches/eval,
 * [8..13] (ms, algorithmic GFLOP) of the 128-, 64- and 32-tile GEMM launches, [14] eager evaluation, [15] leaf launches,
 * [16..18] launches per evaluation of the 128-, 64-, 32-tile GEMM, [19] the factorisation's task-queue launch (ms),
 * [20] its algorithmic GFLOP.  phase_ms must have room for 24 doubles. */
int hbegp_problem_time_eval(hbegp_problem* prob, int dev, int slot, const double* theta, int reps,
                            double* phase_ms);

/* Timed evaluations in the configuration a fit runs in: `reps` evaluations at theta on EVERY slot of device index `dev` at
 * once, one host thread per slot.  out must have room for 16 doubles:
 * [0] wall ms per round (every slot finishes one evaluation) with graph replay, [1] number of slots,
 * [2] the same with eager launches and one hipEvent pair per launch group, on each slot's stream; per evaluation, mean over
 * slots and repetitions, from those events: [3] kmat ms, [4] factorisation ms (task-queue launch, or diagonal-block +
 * tile-GEMM launches), [5] its algorithmic GFLOP, [6] lauum ms, [7] its GFLOP, [8] alpha/lml ms, [9] gradtrace ms,
 * [10] workgroups of the task-queue launch (0: launch-per-product path), [11] launches of [4] per evaluation. */
int hbegp_problem_time_concurrent(hbegp_problem* prob, int dev, const double* theta, int reps, double* out);

/* ---- fit / extend: mirrors FittedKernel::new / ::extend (fit.rs:18-68, 71-176) --------------------- */
typedef struct hbegp_fit_options {
  /* sizeof(hbegp_fit_options) in the header the CALLER was compiled against (use HBEGP_FIT_OPTIONS_INIT).  The library reads
   * and writes through min(struct_size, its own sizeof) bytes only: members beyond the caller's struct are taken as zero /
   * NULL, so the struct can grow at its end.  0 or a size that does not cover `maxeval` is HBEGP_EINVAL. */
  size_t struct_size;
  int maxeval;      /* evaluations per optimiser run; the reference uses 150 (gradmin.rs:54) */
  int fixed_work;   /* 0: stop a run when the optimiser converges; 1: keep evaluating up to maxeval (bench).  A fixed-work run still
                     * makes maxeval objective evaluations, and each returns the lml the optimiser reads.  K^-1 and the gradient are
                     * computed where they are read: at a run's start point, at line-search trials the Armijo test accepts, at trials
                     * that become the fit's new best (their K^-1 and alpha are the model's), and at the burn evaluations at the
                     * incumbent.  A rejected trial ends after its lml (HBEGP_LAZY_GRAD=0 in the environment when the fit starts:
                     * every trial whole, as before; so does a fit whose trace records gradients, trace_grad != NULL).  The values
                     * the optimiser reads, hence its iterates and the fitted model, are bit for bit the same either way -- with one
                     * exception: an evaluation whose lml is finite and whose gradient is not used to fail as a whole (objective +inf,
                     * counted in n_not_pd); as a rejected trial that is no new best its gradient is no longer formed, so its finite
                     * lml is what the line search sees and n_not_pd does not count it. */
  int lbfgs_memory; /* history pairs, 0 = default (10) */
  int trace_cap;    /* capacity (in evaluations) of the trace buffers below, 0 = no trace */
  /* optional trace of the evaluations, for replay parity against the oracle: trace_theta[trace_cap*p],
   * trace_lml[trace_cap] (-inf when not PD), trace_grad[trace_cap*p], trace_run[trace_cap].  Concurrent runs record as
   * their evaluations complete (the first trace_cap of them are kept); on return the records are sorted by run, and
   * within a run they are in evaluation order (problems of at most 128 rows: the first trace_cap records in that order).  Sorting needs trace_run; without it the order is completion order. */
  double* trace_theta;
  double* trace_lml;
  double* trace_grad;
  int* trace_run;
  int* trace_count; /* out: number of evaluations recorded */
  int* n_evals;     /* out (may be NULL): evaluations run, all optimiser runs together */
  int* n_not_pd;    /* out (may be NULL): evaluations whose kernel matrix was not positive definite (objective +inf, fit.rs:105-112) */
} hbegp_fit_options;
#define HBEGP_FIT_OPTIONS_INIT { sizeof(hbegp_fit_options) }

/* Statistics of the calling thread's most recent hbegp_fit_* / hbegp_fit_loo_* call (zeros before the first).  struct_size as in
 * hbegp_fit_options: the library writes min(struct_size, its own sizeof) bytes, so the struct can grow at its end.
 * n_evals / n_not_pd: as the fit options' outputs of the same names.  n_lml_only: the evaluations among n_evals that computed the
 * lml alone -- line-search trials that the optimiser rejected and the capture rule did not keep, so that nobody would have read
 * their K^-1 or gradient (0 with HBEGP_LAZY_GRAD=0, for fits of at most 128 rows, leave-one-out fits, and fits that trace
 * gradients). */
#define HBEGP_STATS_MAX_RUNS 16
typedef struct hbegp_fit_stats {
  size_t struct_size;
  int n_evals;
  int n_not_pd;
  int n_lml_only;
  /* Per optimiser run, for the first n_runs = min(1 + n_restarts, HBEGP_STATS_MAX_RUNS) runs.  run_end_ms: wall time from the call
   * of the fit to the end of the run's last evaluation (fits of at most 128 rows: to the moment the host saw the run's result; the
   * runs are waited for in run order).  run_fused: evaluations launched whole; run_lml_only: line-search trials that ended after
   * their first phase; run_phase2: trials whose second phase (K^-1 and the gradient) ran.  run_lead / run_lag: evaluations among
   * those that ran with a lead / a lag share of the compute units (HBEGP_RUN_BALANCE); 0 where every launch had
   * the even share. */
  int n_runs;
  double run_end_ms[HBEGP_STATS_MAX_RUNS];
  int run_fused[HBEGP_STATS_MAX_RUNS];
  int run_lml_only[HBEGP_STATS_MAX_RUNS];
  int run_phase2[HBEGP_STATS_MAX_RUNS];
  int run_lead[HBEGP_STATS_MAX_RUNS];
  int run_lag[HBEGP_STATS_MAX_RUNS];
} hbegp_fit_stats;
#define HBEGP_FIT_STATS_INIT { sizeof(hbegp_fit_stats) }
int hbegp_last_fit_stats(hbegp_fit_stats* out);

/* Maximise the log marginal likelihood over theta in [ln lo, ln hi] with 1 + n_restarts bounded L-BFGS runs:
 * run 0 starts at theta0, run r>0 at starts[(r-1)*p .. ] (uniform draws in log-bounds made by the caller's RNG,
 * gradmin.rs:22-24).  Capture rule = arg-max lml over every evaluation of every run (fit.rs:116-125), ties broken
 * by the lowest (run, eval) index.  On success *model owns X, y, alpha, K^-1, theta_best (clamped, fit.rs:155-164).
 * theta_best[p] and lml_best may be NULL.  Returns HBEGP_ALL_FAILED when no evaluation succeeded. */
int hbegp_fit_f64(hbegp_ctx* ctx, const double* X, const double* y, int n, int d, double nu, const double* theta0,
                  const double* lo, const double* hi, const double* starts, int n_restarts,
                  const hbegp_fit_options* opt, double* theta_best, double* lml_best, hbegp_model** model);
int hbegp_fit_f32(hbegp_ctx* ctx, const float* X, const float* y, int n, int d, double nu, const double* theta0,
                  const double* lo, const double* hi, const double* starts, int n_restarts,
                  const hbegp_fit_options* opt, double* theta_best, double* lml_best, hbegp_model** model);

/* The same fit with the leave-one-out log pseudo-likelihood as the objective (Rasmussen & Williams 5.4.2: the standard alternative
 * to maximising the marginal likelihood, more robust when the kernel family is wrong): 1 + n_restarts bounded L-BFGS runs on -loo
 * over [ln lo, ln hi] with hbegp_problem_eval_loo's value and gradient, always driven by the host state machine
 * (csrc/lbfgs_step.hpp; the persistent small-fit kernel is not used), one slot per run, run r on device r mod n_devices.  Same
 * signature, options and trace as hbegp_fit_*: maxeval, fixed_work and lbfgs_memory are honoured, trace_lml records loo and
 * trace_grad its gradient.  Capture rule = arg-max loo over every evaluation of every run, ties to the lowest (run, eval).
 * theta_best as in hbegp_fit_*; *loo_best = the best loo.  *model is what hbegp_extend_*(X, y, theta_best, lo = hi = NULL) returns, bit
 * for bit (it is built through that path; hbegp_model_info's lml is the log marginal likelihood there).  Deterministic: the same
 * call gives the same theta and the same model bits. */
int hbegp_fit_loo_f64(hbegp_ctx* ctx, const double* X, const double* y, int n, int d, double nu, const double* theta0,
                      const double* lo, const double* hi, const double* starts, int n_restarts,
                      const hbegp_fit_options* opt, double* theta_best, double* loo_best, hbegp_model** model);
int hbegp_fit_loo_f32(hbegp_ctx* ctx, const float* X, const float* y, int n, int d, double nu, const double* theta0,
                      const double* lo, const double* hi, const double* starts, int n_restarts,
                      const hbegp_fit_options* opt, double* theta_best, double* loo_best, hbegp_model** model);

/* One evaluation at fixed theta + K^-1 (fit.rs:33-68).  HBEGP_NOT_PD where the reference panics (fit.rs:55).  For f64 the result is
 * bit for bit what an evaluation of the same theta inside hbegp_fit_f64 produces (one order of operations for one theta). */
int hbegp_extend_f64(hbegp_ctx* ctx, const double* X, const double* y, int n, int d, double nu, const double* theta,
                     const double* lo, const double* hi, hbegp_model** model);
int hbegp_extend_f32(hbegp_ctx* ctx, const float* X, const float* y, int n, int d, double nu, const double* theta,
                     const double* lo, const double* hi, hbegp_model** model);

/* extend at the theta of `prior`, a model fitted on a PREFIX of these rows (the caller appends its validation samples
 * to the data the last model was built from, minimize.rs:629-644).  The leading floor(n_prior/128) diagonal blocks of L,
 * L^-1 and K^-1 are reused: O(n^2 k) instead of the reference's O(n^3) refactorisation (fit.rs:33-68); same results to
 * rounding.  Falls back to the full path when the prefix differs, n < n_prior or n_prior < 128.  *incremental (may be
 * NULL) reports which path ran.  HBEGP_NOT_PD where the reference panics (fit.rs:55). */
int hbegp_extend_from_f64(hbegp_ctx* ctx, hbegp_model* prior, const double* X, const double* y, int n, hbegp_model** model,
                          int* incremental);
int hbegp_extend_from_f32(hbegp_ctx* ctx, hbegp_model* prior, const float* X, const float* y, int n, hbegp_model** model,
                          int* incremental);

/* ---- row variances: known per-row noise on the diagonal (stochastic kriging) --------------------------
 * A caller who repeats measurements holds, per row, a mean and the variance of that mean.  The `_rv` entry points take those
 * variances as data: K = c Matern + diag(s2 + v_i), v_i = rv[i] >= 0 in the y-normalised scale.  theta, its order, bounds and
 * clamping and p = d + 2 are unchanged; s2 is still learned, as the homoscedastic remainder.  A diagonal entry is formed as
 * (c k(0) + s2) + v_i, each + rounded once, so v = 0 everywhere gives the bits of the call without rv.
 *   rv       n doubles for both element types (like bounds and theta), converted once to the element type on upload.  NULL:
 *            the `_rv` call is its plain counterpart, bit for bit.  A negative or non-finite rv[i] (non-finite also: after the
 *            conversion to float) is HBEGP_EINVAL with the index in the message, before any device call; nothing is written.
 *   problem  hbegp_problem_eval, _eval_loo, _get_* and _kmat_* of such a problem work with v on the diagonal.
 *   fit      the signatures of hbegp_fit_* / hbegp_fit_loo_* / hbegp_extend_* with rv behind y; every path decision (single
 *            launch up to 128 rows, launches, task queue) is taken as without rv.
 *   extend_from  the incremental path runs only when the prefix of X, of y's rows and of v equals the prior's (a prior without
 *            v counts as zeros), else the full path.  Plain hbegp_extend_from_* on a prior that carries v is HBEGP_EINVAL, and so
 *            is hbegp_extend_from_rv_* with rv = NULL on such a prior: it is the plain call, refusals included.
 * Everything downstream reads K^-1, L^-1 and alpha and is unchanged: predictions stay those of the latent function and exclude
 * s2 and v.  What the model's v does change:
 *   hbegp_paths_create_*   the noise draw of row i is sqrt(s2 + v_i) eps (a call without eps is unaffected);
 *   hbegp_model_loo_*      var is that of the left-out noisy observation, 1 / K^-1_ii, which now contains s2 + v_i.
 * What stays homoscedastic: hbegp_select_batch_*, hbegp_knowledge_gradient_* and hbegp_qei_* keep s2 alone as the noise of the
 * observation they imagine at a NEW point (no v is known there). */
int hbegp_problem_create_rv_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, int n, int d, double nu,
                                int n_slots, hbegp_problem** out);
int hbegp_problem_create_rv_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, int n, int d, double nu,
                                int n_slots, hbegp_problem** out);
int hbegp_fit_rv_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, int n, int d, double nu,
                     const double* theta0, const double* lo, const double* hi, const double* starts, int n_restarts,
                     const hbegp_fit_options* opt, double* theta_best, double* lml_best, hbegp_model** model);
int hbegp_fit_rv_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, int n, int d, double nu,
                     const double* theta0, const double* lo, const double* hi, const double* starts, int n_restarts,
                     const hbegp_fit_options* opt, double* theta_best, double* lml_best, hbegp_model** model);
/* Fit by maximising the leave-group-out log predictive density over group[n] (NULL: singletons): hbegp_fit_loo_* with
 * hbegp_problem_eval_lgo's value and gradient -- host-driven for every n, capture by arg-max, *model what hbegp_extend_* (with rv:
 * hbegp_extend_rv_*) returns at theta_best, bit for bit.  rv (may be NULL) as in hbegp_fit_rv_*.  The group lists are checked and
 * built once and uploaded once per device. */
int hbegp_fit_lgo_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, const int* group, int n, int d, double nu,
                      const double* theta0, const double* lo, const double* hi, const double* starts, int n_restarts,
                      const hbegp_fit_options* opt, double* theta_best, double* lgo_best, hbegp_model** model);
int hbegp_fit_lgo_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, const int* group, int n, int d, double nu,
                      const double* theta0, const double* lo, const double* hi, const double* starts, int n_restarts,
                      const hbegp_fit_options* opt, double* theta_best, double* lgo_best, hbegp_model** model);
int hbegp_fit_loo_rv_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, int n, int d, double nu,
                         const double* theta0, const double* lo, const double* hi, const double* starts, int n_restarts,
                         const hbegp_fit_options* opt, double* theta_best, double* loo_best, hbegp_model** model);
int hbegp_fit_loo_rv_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, int n, int d, double nu,
                         const double* theta0, const double* lo, const double* hi, const double* starts, int n_restarts,
                         const hbegp_fit_options* opt, double* theta_best, double* loo_best, hbegp_model** model);
int hbegp_extend_rv_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, int n, int d, double nu,
                        const double* theta, const double* lo, const double* hi, hbegp_model** model);
int hbegp_extend_rv_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, int n, int d, double nu,
                        const double* theta, const double* lo, const double* hi, hbegp_model** model);
int hbegp_extend_from_rv_f64(hbegp_ctx* ctx, hbegp_model* prior, const double* X, const double* y, const double* rv, int n,
                             hbegp_model** model, int* incremental);
int hbegp_extend_from_rv_f32(hbegp_ctx* ctx, hbegp_model* prior, const float* X, const float* y, const double* rv, int n,
                             hbegp_model** model, int* incremental);
/* 1 and, with rv != NULL, the n variances the model works with (for an f32 model the rounded values, widened); 0 for a model
 * without them (rv is not written). */
int hbegp_model_row_variance(const hbegp_model* model, double* rv);

/* The warped fit: theta and one warp per feature learned jointly.  A host-driven bounded L-BFGS over the p + 2d log-space
 * variables [theta, ln a_1..ln a_d, ln b_1..ln b_d] with hbegp_problem_eval_warped's value and gradient, on ONE single-slot problem
 * with a fit's path selection, 1 + n_restarts runs ONE AFTER ANOTHER.  Run 0 starts at (theta0, ab0), ab0 NULL = the identity: with
 * a plain fit's optimum as theta0 the result is no worse than the plain fit.  starts[n_restarts * (p + 2d)] in log space; rv (may
 * be NULL) as in hbegp_fit_rv_*; ab_lo / ab_hi [2d] (each may be NULL = 0.2 / 5 throughout) bound a and b as lo / hi bound theta.
 * maxeval, fixed_work, lbfgs_memory and the trace come from opt (rows of trace_theta / trace_grad have p + 2d entries here; the
 * other statistics of hbegp_last_fit_stats are not kept).  Capture as in hbegp_fit_*: the best lml wins, ties go to the lowest (run,
 * evaluation); an HBEGP_NOT_PD evaluation counts as +inf with a zero gradient; HBEGP_ALL_FAILED when every evaluation failed.
 * theta_best[p] (clamped, log space), ab_best[2d] (linear space, inside its bounds), *lml_best.  *model (may be NULL) is, bit for
 * bit, hbegp_extend_* (hbegp_extend_rv_* with rv) at theta_best on the rows hbegp_warp_apply gives for ab_best, rounded once to the
 * element type; it carries ab_best: hbegp_model_warp returns 1 and fills ab[2d] (may be NULL) for such a model, 0 for every other
 * model.  All posterior entry points take a warped model as they take any model: they work in u-space, so their query points are
 * warped rows and the gradients they return are with respect to u (multiply by hbegp_warp_apply's dU_dx for x).  HBEGP_EINVAL for
 * features outside [0, 1] and for warp bounds or ab0 that are not finite and positive.  Not built here: runs side by side (they
 * need a feature buffer per slot), the device-driven fit of at most 128 rows, leave-one-out / leave-group-out objectives. */
int hbegp_fit_warped_f64(hbegp_ctx* ctx, const double* X, const double* y, const double* rv, int n, int d, double nu,
                         const double* theta0, const double* lo, const double* hi, const double* ab0, const double* ab_lo,
                         const double* ab_hi, const double* starts, int n_restarts, const hbegp_fit_options* opt,
                         double* theta_best, double* ab_best, double* lml_best, hbegp_model** model);
int hbegp_fit_warped_f32(hbegp_ctx* ctx, const float* X, const float* y, const double* rv, int n, int d, double nu,
                         const double* theta0, const double* lo, const double* hi, const double* ab0, const double* ab_lo,
                         const double* ab_hi, const double* starts, int n_restarts, const hbegp_fit_options* opt,
                         double* theta_best, double* ab_best, double* lml_best, hbegp_model** model);
int hbegp_model_warp(const hbegp_model* model, double* ab);

/* ---- model: mirrors predict() (predict.rs:7-52) and the FittedKernel fields -------------------------- */
/* mean[m]; var[m] or NULL.  var = c + 1e-5 - rowsum((K* K^-1) o K*), negatives clamped to 0 (predict.rs:25-48);
 * it excludes s2 (the reference predicts the latent function).  *n_warn (may be NULL) = number of variances below
 * -sqrt(1e-5) before clamping (the reference prints a warning for those, predict.rs:39-48). */
int hbegp_predict_f64(hbegp_model* model, const double* Xs, int m, double* mean, double* var, int* n_warn);
int hbegp_predict_f32(hbegp_model* model, const float* Xs, int m, float* mean, float* var, int* n_warn);

/* Posterior gradient at m query points.  mean[m], var[m], n_warn as hbegp_predict_* computes them on its batched path (m > 8;
 * the gradient call takes that path for every m); dmean[m*d], dvar[m*d] row-major: d mean / d x*_k and d var / d x*_k, in the
 * units of the feature space the model was fitted on (the coordinates of Xs, not the length-scaled ones).  var and dvar may be
 * NULL together (mean and its gradient only); one of them alone is HBEGP_EINVAL.  m = 0 is a no-op.
 *   k(x*, x_j) = c phi_nu(r),  r^2 = sum_k ((x*_k - x_jk) / ell_k)^2  (no noise term),  psi = phi'(r) / r:
 *     nu = 1/2: -exp(-r)/r,  nu = 3/2: -3 exp(-sqrt3 r),  nu = 5/2: -(5/3)(1 + sqrt5 r) exp(-sqrt5 r),  nu = inf: -exp(-r^2/2)
 *   dk_j/dx*_k = c psi(r) (x*_k - x_jk) / ell_k^2
 *   dmean_k = sum_j dk_j/dx*_k alpha_j,   dvar_k = -2 (d k* / d x*_k)^T K^-1 k*, evaluated as -2 (L^-1 d k* / d x*_k) . (L^-1 k*)
 *   like the variance itself (an explicit K^-1 k* loses digits in proportion to cond(K))
 * A training point at r = 0 (the query point equals it) contributes 0 for every nu: the exact limit for nu >= 3/2; for
 * nu = 1/2 the kernel has a kink there and has no derivative, and 0 is the chosen value (the mean of the one-sided slopes).
 * Where the variance was clamped to 0 (predict.rs:39-48) dvar is 0.  A NaN in a query row gives NaN in that row's outputs
 * only.  Sums are fp64 for both element types, in a fixed order: the same call gives the same bits. */
int hbegp_predict_grad_f64(hbegp_model* model, const double* Xs, int m, double* mean, double* var, double* dmean, double* dvar,
                           int* n_warn);
int hbegp_predict_grad_f32(hbegp_model* model, const float* Xs, int m, float* mean, float* var, float* dmean, float* dvar,
                           int* n_warn);

/* Maximise the expected improvement EI(x) (acquisition.rs:141-171) in the model's normalised y space over the box
 * [lo, hi] (d entries each, feature space) with S bounded L-BFGS runs on -EI (the fit optimiser's method and constants,
 * lbfgs_step.hpp), run s from starts[s*d ..] (inside the box).  The runs advance in lockstep: every round is ONE batched
 * hbegp_predict_grad over the runs still going.  EI and its gradient are computed on the host in double:
 *   dEI/dx = -Phi(z) dmean + phi(z) dsigma,  dsigma = dvar / (2 sigma);  sigma = 0: -dmean where mean < fmin, else 0.
 * x_out[S*d] receives each run's best evaluated point, ei_out[S] its EI (never below the EI at the start),
 * nevals_out[S] (may be NULL) the evaluations each run used (<= maxeval).  HBEGP_EINVAL for S < 1, maxeval < 1, lo > hi,
 * a start outside the box, a non-finite fmin_normalized or a model of the other element type; nothing runs on the device then. */
int hbegp_maximize_ei_f64(hbegp_model* model, const double* starts, int S, const double* lo, const double* hi, double fmin_normalized,
                          int maxeval, double* x_out, double* ei_out, int* nevals_out);
int hbegp_maximize_ei_f32(hbegp_model* model, const float* starts, int S, const double* lo, const double* hi, double fmin_normalized,
                          int maxeval, float* x_out, double* ei_out, int* nevals_out);

/* Joint posterior of the latent function at m query points (predict.rs:7-52 extended to pairs), in the model's normalised
 * y space like hbegp_predict_*:
 *   cov[i*m + j] = c phi_nu(r(x*_i, x*_j)) + (1e-5 + jitter) [i == j] - q_i . q_j,   q_i = L^-1 k*_i
 * full symmetric m x m, row-major, exactly symmetric (the lower triangle mirrored, not computed twice).  1e-5 is the reference's
 * min_noise (predict.rs:25-29), so the diagonal is hbegp_predict's variance before clamping; with jitter = 0 it matches it to
 * rounding.  No clamping: a clamped diagonal would not be a covariance.  mean[m] as hbegp_predict_* (may be NULL).
 * jitter >= 0 and finite.  m = 0 is a no-op.  A non-finite query coordinate is HBEGP_EINVAL (one NaN row would poison the
 * factor of every other row in the sampling call), checked on the host before any device work.  Threads may call these on
 * one model at once (serialised per model, like predict).  Work matrices of m_p^2 elements (m_p = m rounded up to 128) are
 * borrowed for the call; an m whose work does not fit in device memory is HBEGP_ENOMEM. */
int hbegp_predict_cov_f64(hbegp_model* model, const double* Xs, int m, double jitter, double* mean, double* cov);
int hbegp_predict_cov_f32(hbegp_model* model, const float* Xs, int m, double jitter, float* mean, float* cov);

/* S joint draws from N(mean, cov) as above, from the CALLER's standard normals (the RNG stays on the caller side, DESIGN
 * section 7): z[S*m], draw s = row s.  samples[S*m] (may be NULL): samples[s] = mean + L_S z_s, where L_S is the lower Cholesky
 * factor of cov (unique, so the result does not depend on how the library factors it).
 * argmin[S] (may be NULL): the index of the smallest entry of draw s, ties to the lowest index (Thompson sampling for a
 * minimiser).  samples and argmin must not both be NULL.  *info (may be NULL): 0, or 1 + the first column of the 16-column
 * panel whose pivot failed (the fit's convention).  Returns HBEGP_NOT_PD when cov is not positive definite in the element
 * type; nothing is written to samples / argmin then.  The caller can retry with a larger jitter: the library never raises it
 * by itself.  HBEGP_EINVAL (before any device call) for a NULL model, m < 0, S < 1, a NULL z with m > 0, a jitter < 0 or
 * not finite, samples and argmin both NULL, a model of the other element type or a non-finite query coordinate.
 * The same call gives the same bits (fixed-order sums, no atomics). */
int hbegp_sample_posterior_f64(hbegp_model* model, const double* Xs, int m, const double* z, int S, double jitter,
                               double* samples, int* argmin, int* info);
int hbegp_sample_posterior_f32(hbegp_model* model, const float* Xs, int m, const float* z, int S, double jitter,
                               float* samples, int* argmin, int* info);

/* Greedy batch selection by expected improvement with fantasised observations (kriging believer / constant liar), in the
 * normalised y space like hbegp_predict_*.  Start: mu = the posterior mean, v = diag Sigma of hbegp_predict_cov at jitter 0
 * (hbegp_predict's variance before clamping), fmin_0 = fmin_normalized.  For t = 0 .. k-1:
 *   j_t = argmax over the rows not yet picked of EI(mu_i, sqrt(max(v_i, 0)), fmin_t) (acquisition.rs:141-171, fp64), ties to
 *         the LAST maximal index as Rust's max_by (k = 1 is find_best_candidate_by_ei); ei[t] = that EI;
 *   f_t = mu_{j_t} (lie == NULL: kriging believer) or *lie (constant liar); fmin_{t+1} = min(fmin_t, f_t);
 *   condition on a noisy observation f_t at x_{j_t} with the model's noise s2: r_i = Sigma_{i,j_t} - sum_{s<t} c_s[i] c_s[j_t],
 *         r_{j_t} = v_{j_t} - 1e-5, c_t = r / sqrt(max(r_{j_t}, 0) + s2), v -= c_t^2, mu += c_t (f_t - mu_{j_t}) / sqrt(..).
 * After t picks (mu, max(v, 0)) is hbegp_predict of the model extended at the same theta with the rows (x_{j_s}, f_s), s < t.
 * idx[k] (required for k > 0); ei[k], mean_out[m], var_out[m] (each may be NULL): the state after all k conditionings,
 * var_out clamped at 0 like hbegp_predict.  k = 0 is a no-op.  HBEGP_EINVAL (before any device call) for a NULL model, m < 0,
 * k < 0, k > m, a NULL idx with k > 0, a non-finite fmin_normalized or *lie, a model of the other element type or a non-finite
 * query coordinate.  Serialised per model like predict; the same call gives the same bits, and a call with k = t returns the
 * first t entries of idx / ei of any call with a larger k.  Sigma (m_p^2 elements) and an fp64 workspace of k m_p are
 * borrowed for the call; work that does not fit in device memory is HBEGP_ENOMEM. */
int hbegp_select_batch_f64(hbegp_model* model, const double* Xs, int m, int k, double fmin_normalized, const double* lie, int* idx,
                           double* ei, double* mean_out, double* var_out);
int hbegp_select_batch_f32(hbegp_model* model, const float* Xs, int m, int k, double fmin_normalized, const double* lie, int* idx,
                           double* ei, float* mean_out, float* var_out);

/* Knowledge gradient over a candidate set (Frazier, Powell, Dayanik 2009: correlated normal beliefs), in the normalised y space
 * like hbegp_predict_*: the value of ONE more noisy sample at row j, measured by how much it is expected to lower the minimum of
 * the posterior mean over the m rows of Xs.  It needs no fmin.  The first mc <= m rows are the places a sample may be taken; the
 * minimum runs over all m rows (mc = m: the classic correlated KG).  With mu and Sigma of hbegp_predict_cov at jitter 0 and the
 * model's noise s2, for j < mc:
 *   r_i = Sigma_ij (i != j),  r_j = Sigma_jj - 1e-5 (the latent variance),  d_j = max(r_j, 0) + s2,  st_i = r_i / sqrt(d_j)
 *   (hbegp_select_batch's first conditioning with f = mu_j + sqrt(d_j) Z: the mean after the sample is mu + st Z, Z ~ N(0, 1));
 *   kg[j] = min_i mu_i - E_Z[ min_i (mu_i + st_i Z) ] >= 0,
 * in closed form by the paper's Algorithm 1 on the lines a_i = -mu_i, b_i = -st_i: sorted by (b, a), of equal slopes the largest a
 * kept, the upper envelope with strictly increasing breakpoints c_k, kg[j] = sum_k (b_{k+1} - b_k) f(-|c_k|), f(z) = phi(z) + z Phi(z).
 * A single surviving line (m = 1, all slopes equal) gives exactly 0.  All of it is fp64 for both element types, so kg is double.
 * kg[mc] (required for mc > 0); best (may be NULL): the LAST index of the maximum of kg, as Rust's max_by and hbegp_select_batch
 * (-1 for mc = 0); imin (may be NULL): the lowest index of the minimum of mu over all m rows -- what a noisy tuner should
 * recommend instead of its best observation; mean_out[m], var_out[m] (may be NULL): mu and max(diag Sigma, 0), bit for bit
 * hbegp_predict_cov's mean and clamped diagonal (the mean is hbegp_predict's too for m > 16).  mc = 0 still fills imin / mean_out / var_out; m = 0 is a no-op (best = imin = -1).
 * HBEGP_EINVAL (before any device call) for a NULL model, m < 0, mc < 0, mc > m, a NULL kg with mc > 0, a model of the other
 * element type or a non-finite query coordinate.  Serialised per model like predict; fixed-order sums and no atomics: the same
 * call gives the same bits, and kg[j] does not depend on mc.  Sigma (m_p^2 elements) is borrowed for the call, and for m > 8192 a
 * workspace of at most 512 x 16 P bytes (P the power of two at or above m); work that does not fit in device memory is
 * HBEGP_ENOMEM. */
int hbegp_knowledge_gradient_f64(hbegp_model* model, const double* Xs, int m, int mc, double* kg, int* best, int* imin,
                                 double* mean_out, double* var_out);
int hbegp_knowledge_gradient_f32(hbegp_model* model, const float* Xs, int m, int mc, double* kg, int* best, int* imin,
                                 float* mean_out, float* var_out);

/* Noisy expected improvement over a candidate set (Letham, Karrer, Ottoni, Bakshy 2019), in the normalised y space like
 * hbegp_predict_*: EI averaged over joint posterior draws of the latent function at the BASELINE, each draw with its own incumbent
 * and its own conditioned belief about the candidate.  It needs no fmin.  Xs[m*d]: the first mb rows are the baseline (normally the
 * training rows), the other mc = m - mb rows the candidates; z[S*mb] the CALLER's standard normals, one row per draw (the RNG stays
 * on the caller side).  With mu and Sigma of hbegp_predict_cov for the m rows at the same jitter, split into b and c parts:
 *   L_b = chol(Sigma_bb), lower;   A = Sigma_cb L_b^-T;   rho_j = max(Sigma_jj - sum_k A_jk^2, 0)
 *   draw s:  f_s = mu_b + L_b z_s,   fmin_s = min_i f_s,i,   mu_js = mu_j + A_j . z_s
 *   nei[j] = (1/S) sum_s EI(mu_js, sqrt(rho_j), fmin_s) >= 0
 * with EI of acquisition.rs:141-171 (its std == 0 branch included): the exact expectation over f(x_j) given each draw of the
 * baseline, no inner sampling.  Sigma, L_b, A and the two products with z are in the element type like hbegp_sample_posterior_*; the
 * sums of squares for rho, every EI, the minima and the averages are fp64 in a fixed order without atomics, so nei is double.
 * Only Sigma_bb is factored, the candidates never: identical candidates are as fine as distinct ones.  HBEGP_NOT_PD is decided
 * by Sigma_bb alone, with *info = 1 + the first column of the failing 16-column panel as hbegp_sample_posterior_* reports it; then
 * no other output is written.  The library never raises the jitter by itself.
 * nei[mc] (required for mc > 0); best (may be NULL): the LAST index of the maximum of nei, as hbegp_knowledge_gradient_* (-1 for
 * mc = 0); fmin_draws[S] (may be NULL): fmin_s; rho[mc] (may be NULL); info (may be NULL).  mc = 0 fills fmin_draws only.
 * HBEGP_EINVAL (before any device call; a refused call writes nothing) for a NULL model, m < 1, mb < 1, mb > m, S < 1, a NULL z, a
 * NULL nei with mc > 0, a jitter that is negative or not finite, a model of the other element type or a non-finite coordinate.
 * Serialised per model like predict; the same call gives the same bits.  The work matrices (about 2.5 m_p^2 elements, m_p =
 * round128(mb) + mc rounded up to 128) are borrowed for the call; work that does not fit in device memory is HBEGP_ENOMEM. */
int hbegp_noisy_ei_f64(hbegp_model* model, const double* Xs, int m, int mb, const double* z, int S, double jitter, double* nei,
                       int* best, double* fmin_draws, double* rho, int* info);
int hbegp_noisy_ei_f32(hbegp_model* model, const float* Xs, int m, int mb, const float* z, int S, double jitter, double* nei,
                       int* best, double* fmin_draws, double* rho, int* info);

/* Expected hypervolume improvement (EHVI) of TWO objectives, both minimised, each modelled by its own model; the two posteriors
 * are taken as independent.  Everything is in each model's normalised y space.  models[n_obj]: objective 0 then objective 1
 * (n_obj must be 2); they share d, the element type and the device and may differ in n and nu.  At a row of Xs[m*d] objective k has
 * the posterior N(mu_k, sigma_k^2) of hbegp_predict_* (the variance clamped at 0, without the noise).  ref[2] is the reference point
 * r = (r1, r2), front[P*2] the caller's points (a_i, b_i) in any order -- both always double, like bounds.  The library reduces the
 * front on the host to its non-dominated points strictly inside the box (a_i < r1, b_i < r2), sorted by a ascending (b descends), with
 * a_0 = -inf, a_{P+1} = r1, b_0 = r2: dominated points, duplicates and points outside the box change nothing, bit for bit.  With
 *   G_k(t) = E[(t - Y_k)^+] = sigma_k h((t - mu_k) / sigma_k),  h(z) = z Phi(z) + phi(z),  G_k(-inf) = 0,
 *   ehvi = sum_{i=0..P} [G_1(a_{i+1}) - G_1(a_i)] G_2(b_i) >= 0
 * is the expected area, inside the box, that the point would add to what the front dominates; P = 0 gives G_1(r1) G_2(r2).
 * dG/dmu = -Phi(z) and dG/dsigma = phi(z) give the partials from the same sum; grad[m*d] (may be NULL: then no gradient launch is
 * issued) follows through hbegp_predict_grad_*'s dmean and dvar with dsigma = dvar / (2 sigma).  sigma_k = 0: G_k(t) = (t - mu_k)^+
 * and dsigma_k counts as 0, as in hbegp_maximize_ei_*.  h is evaluated without cancellation (phi(a) - a Phi(-a) for z = -a <= 0,
 * z + h(-z) above).  All arithmetic and sums are fp64 for both element types, in a fixed order without atomics: ehvi is double, and a
 * row's bits depend neither on m, nor on its position, nor on whether a gradient was asked for.
 * ehvi[m] (required for m > 0); best (may be NULL): the LAST index of the maximum of ehvi, as hbegp_knowledge_gradient_* (a NaN never
 * wins; -1 for m = 0); mean[m*2], var[m*2] (each may be NULL): row j holds objective 0 then objective 1, bit for bit what
 * hbegp_predict_* returns on its batched path (m > 16), or hbegp_predict_grad_* with a gradient.  A NaN coordinate gives NaN in
 * that row of ehvi and grad only.  m = 0 is a no-op.
 * HBEGP_EINVAL (before any device call) for n_obj != 2, a NULL model, the same model twice, models of different d, element type or
 * device, a model of the other element type, m < 0, P < 0, a NULL Xs or ehvi with m > 0, a NULL ref, a NULL front with P > 0, or a
 * non-finite front or ref value.  Both models are locked for the call, in a fixed order: calls that name them in either order never
 * wait for each other.  Each model's predict runs on its own stream; thresholds and outputs are borrowed for the call; work that
 * does not fit in device memory is HBEGP_ENOMEM. */
int hbegp_ehvi_f64(hbegp_model* const* models, int n_obj, const double* Xs, int m, const double* front, int P, const double* ref,
                   double* ehvi, double* grad, int* best, double* mean, double* var);
int hbegp_ehvi_f32(hbegp_model* const* models, int n_obj, const float* Xs, int m, const double* front, int P, const double* ref,
                   double* ehvi, float* grad, int* best, float* mean, float* var);
/* S bounded L-BFGS runs maximising hbegp_ehvi_* over the box [lo, hi] in lockstep, with the contract of hbegp_maximize_ei_*
 * (lbfgs_step.hpp with the fit's constants): every round is one batched gradient predict per model over the runs still going and
 * the EHVI kernel with its gradient.  starts[S*d] inside the box; x_out[S*d], ehvi_out[S]: each run's best evaluated point (never
 * worse than its start; an f32 run evaluates and returns f32 points of the box) -- hbegp_ehvi_* at x_out reproduces ehvi_out bit
 * for bit; nevals_out[S] (may be NULL) <= maxeval.  A NaN prediction is a failed evaluation.  HBEGP_EINVAL for everything
 * hbegp_ehvi_* refuses about models, front and ref, and for S < 1, a NULL starts / lo / hi / x_out / ehvi_out, maxeval < 1,
 * lo > hi or a start outside the box. */
int hbegp_maximize_ehvi_f64(hbegp_model* const* models, int n_obj, const double* starts, int S, const double* lo, const double* hi,
                            const double* front, int P, const double* ref, int maxeval, double* x_out, double* ehvi_out,
                            int* nevals_out);
int hbegp_maximize_ehvi_f32(hbegp_model* const* models, int n_obj, const float* starts, int S, const double* lo, const double* hi,
                            const double* front, int P, const double* ref, int maxeval, float* x_out, double* ehvi_out,
                            int* nevals_out);

/* Expected hypervolume improvement of n_obj = 2, 3 or 4 objectives, all minimised, each modelled by its own model; the posteriors
 * are taken as independent.  Everything hbegp_ehvi_* says about the models (models[n_obj], objective 0 first; they share d, the
 * element type and the device and may differ in n and nu), the normalised y spaces, the posterior N(mu_k, sigma_k^2) at a row,
 * "sigma = 0", h's evaluation, fp64 arithmetic in a fixed order without atomics, NaN rows, best, m = 0, the locking order, the
 * per-model streams and borrowed device memory holds here with "two" read as n_obj.  ref[n_obj] is the reference point r,
 * front[P*n_obj] the caller's points in any order (row i holds its n_obj coordinates), both always double.  The library reduces the
 * front on the host to its distinct non-dominated points strictly inside the box (every coordinate below r_k) -- the result depends
 * on that SET only: the order of the points, duplicates, dominated points and points outside the box change no bit -- and splits
 * the part of (-inf, r) that no front point weakly dominates into disjoint boxes [l_j, u_j), each l_jk -inf or a k-th coordinate
 * of the front, each u_jk such a coordinate or r_k (a sweep over the objectives in their order: hbegp_debug_ehvi_boxes).  With
 * G_k(t) = E[(t - Y_k)^+] = sigma_k h((t - mu_k) / sigma_k) and G_k(-inf) = 0,
 *   ehvi = sum_j prod_k [G_k(u_jk) - G_k(l_jk)] >= 0
 * is the expected volume, inside the box, that the point would add to what the front dominates; P = 0 gives prod_k G_k(r_k).  The
 * partials follow from dG/dmu = -Phi(z), dG/dsigma = phi(z) in the same sum, grad[m*d] (may be NULL: no gradient launch) through
 * hbegp_predict_grad_*'s dmean and dvar.  n_obj = 2 gives the quantity of hbegp_ehvi_* by another sum: equal within rounding, not
 * bit for bit.  A row's bits depend neither on m, nor on its position, nor on whether a gradient was asked for.
 * ehvi[m] (required for m > 0); best (may be NULL); mean[m*n_obj], var[m*n_obj] (each may be NULL): row j holds objective 0 first,
 * bit for bit hbegp_predict_*'s (batched path) or hbegp_predict_grad_*'s numbers.
 * HBEGP_EINVAL (before any device call) for n_obj outside 2 .. 4, m < 0, P < 0, a NULL ref, a NULL front with P > 0, a non-finite
 * front or ref value, a NULL model, a model named twice, models of different d, element type or device, a model of the other
 * element type, a NULL Xs or ehvi with m > 0.  HBEGP_ENOMEM, also before any device call, for a front whose free region splits
 * into more than HBEGP_EHVI_ND_MAX_BOXES boxes (their number grows like P^(n_obj - 1)), and for work that does not fit in device
 * memory.  The cap keeps the index list of a call, 8 n_obj bytes per box, at 32 MiB at the most. */
#define HBEGP_EHVI_ND_MAX_BOXES 1048576
int hbegp_ehvi_nd_f64(hbegp_model* const* models, int n_obj, const double* Xs, int m, const double* front, int P, const double* ref,
                      double* ehvi, double* grad, int* best, double* mean, double* var);
int hbegp_ehvi_nd_f32(hbegp_model* const* models, int n_obj, const float* Xs, int m, const double* front, int P, const double* ref,
                      double* ehvi, float* grad, int* best, float* mean, float* var);
/* S bounded L-BFGS runs maximising hbegp_ehvi_nd_* over the box [lo, hi] in lockstep, with the contract of hbegp_maximize_ehvi_*:
 * every round is one batched gradient predict per model over the runs still going and the box kernel with its gradient; the
 * front is decomposed once for all rounds.  hbegp_ehvi_nd_* at x_out reproduces ehvi_out bit for bit; nevals_out[S] (may be NULL)
 * <= maxeval.  HBEGP_EINVAL / HBEGP_ENOMEM for everything hbegp_ehvi_nd_* refuses about n_obj, front, ref and models, and
 * HBEGP_EINVAL for S < 1, a NULL starts / lo / hi / x_out / ehvi_out, maxeval < 1, lo > hi or a start outside the box. */
int hbegp_maximize_ehvi_nd_f64(hbegp_model* const* models, int n_obj, const double* starts, int S, const double* lo, const double* hi,
                               const double* front, int P, const double* ref, int maxeval, double* x_out, double* ehvi_out,
                               int* nevals_out);
int hbegp_maximize_ehvi_nd_f32(hbegp_model* const* models, int n_obj, const float* starts, int S, const double* lo, const double* hi,
                               const double* front, int P, const double* ref, int maxeval, float* x_out, double* ehvi_out,
                               int* nevals_out);

/* Constrained expected improvement (cEI; Gardner et al. 2014, Gelbart et al. 2014): the expected improvement of a minimised objective
 * times the probability that C constraints g_k(x) <= t_k hold, each quantity modelled by its own model; the 1 + C posteriors are
 * taken as independent.  Everything is in each model's own normalised y space.  Model 0 is `objective`, models 1 .. C are
 * constraints[0 .. n_con) with limits[k - 1] = t_k (0 <= n_con <= HBEGP_CEI_MAX_CONSTRAINTS); they share d, the element type and the
 * device and may differ in n and nu.  limits and fmin_normalized are always double.  At a row of Xs[m*d] model k has the posterior
 * N(mu_k, sigma_k^2) of hbegp_predict_* (the variance clamped at 0, without the noise), sigma_k = sqrt(var_k); "sigma = 0" means
 * !(sigma > 2.220446049250313e-16), as in hbegp_ehvi_*.  With h(z) = z Phi(z) + phi(z), z_0 = (fmin - mu_0) / sigma_0 and
 * z_k = (t_k - mu_k) / sigma_k:
 *   ei  = sigma_0 h(z_0)              -- hbegp_ehvi_*'s G_0(fmin), evaluated the same way: phi(a) - a Phi(-a) for z = -a <= 0,
 *                                        z + h(-z) above, the tail terms exactly 0 beyond |z| = 38
 *   F_k = Phi(z_k)                    -- from the same evaluation; exactly 0 (or 1) beyond |z| = 38
 *   pof = F_1 F_2 .. F_C              -- multiplied in ascending k; 1.0 for n_con = 0
 *   cei = ei * pof >= 0.
 * ei is expected_improvement (acquisition.rs:141-171) up to rounding; it is NOT bit for bit the host formula inside
 * hbegp_maximize_ei_*.  sigma_0 = 0: ei = (fmin - mu_0)^+.  sigma_k = 0: F_k = [t_k > mu_k].
 * fmin_normalized = +inf means "no feasible point is known": ei counts as 1 and its partials as 0, so cei = pof and the call is a
 * search for feasibility.  -inf and NaN are refused, and so is n_con = 0 with fmin = +inf (nothing would be computed).
 * grad[m*d] (may be NULL: then no gradient launch is issued) is formed WITHOUT dividing by F_k:
 *   d cei / d(.)_0 = pof * d ei / d(.)_0,           d ei / d mu_0 = -Phi(z_0),        d ei / d sigma_0 = phi(z_0)
 *   d cei / d(.)_k = ei * W_k * d F_k / d(.)_k,     d F_k / d mu_k = -phi(z_k) / sigma_k,  d F_k / d sigma_k = -z_k phi(z_k) / sigma_k
 * with W_k = prod_{j != k} F_j from a prefix (ascending) and a suffix (descending) product in a fixed order, so a factor that is
 * exactly 0 leaves the gradient finite.  sigma = 0: the partial w.r.t. that sigma counts as 0, and so do both partials of F_k.
 *   grad[j][i] = sum_{k=0..C} (d cei / d mu_k * dmean_k[j][i] + d cei / d sigma_k * dvar_k[j][i] / (2 sigma_k)),  ascending k,
 * dmean and dvar being hbegp_predict_grad_*'s.  All arithmetic is fp64 for both element types, in a fixed order without atomics:
 * cei, ei and pof are double, and a row's bits depend only on its own posteriors, fmin and limits -- not on m, on the row's
 * position, or on whether a gradient was asked for.  A product that falls below the normal range (about 1e-308)
 * loses its digits to gradual underflow and ends as exactly 0, with a zero gradient: where that matters -- a maximiser started where
 * every start has pof = 0 does not move -- use the log-space form hbegp_log_constrained_ei_* below.
 * cei[m] (required for m > 0); best (may be NULL): the LAST index of the maximum of cei (a NaN never wins; -1 for m = 0); ei[m],
 * pof[m] (each may be NULL); mean[m*(1+C)], var[m*(1+C)] (each may be NULL): row j holds the objective then the constraints, bit
 * for bit what hbegp_predict_* returns on its batched path (m > 16), or hbegp_predict_grad_* with a gradient.  A NaN coordinate
 * gives NaN in that row of cei, ei, pof and grad only.  m = 0 is a no-op.
 * HBEGP_EINVAL (before any device call; a refused call writes nothing) for a NULL objective, n_con < 0 or
 * > HBEGP_CEI_MAX_CONSTRAINTS, a NULL constraints or limits with n_con > 0, a NULL entry in constraints, any model named twice (the
 * objective included), models of different d, element type or device, a model of the other element type, a non-finite limit, a
 * fmin that is NaN or -inf, n_con = 0 with fmin = +inf, m < 0, or a NULL Xs or cei with m > 0.  All 1 + C models are locked for the
 * call, in a fixed order: calls that name them in any order never wait for each other.  Each model's predict runs on its own
 * stream; the outputs are borrowed for the call; work that does not fit in device memory is HBEGP_ENOMEM. */
#define HBEGP_CEI_MAX_CONSTRAINTS 8
int hbegp_constrained_ei_f64(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const double* Xs, int m,
                             double fmin_normalized, const double* limits, double* cei, double* grad, int* best, double* ei,
                             double* pof, double* mean, double* var);
int hbegp_constrained_ei_f32(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const float* Xs, int m,
                             double fmin_normalized, const double* limits, double* cei, float* grad, int* best, double* ei,
                             double* pof, float* mean, float* var);
/* S bounded L-BFGS runs maximising hbegp_constrained_ei_* over the box [lo, hi] in lockstep, with the contract of
 * hbegp_maximize_ehvi_*: every round is one batched gradient predict per model over the runs still going and the cEI kernel with its
 * gradient.  starts[S*d] inside the box; x_out[S*d], cei_out[S]: each run's best evaluated point (never worse than its start; an f32
 * run evaluates and returns f32 points of the box) -- hbegp_constrained_ei_* at x_out reproduces cei_out bit for bit; nevals_out[S]
 * (may be NULL) <= maxeval.  A value or a gradient component that is not finite is a failed evaluation.  HBEGP_EINVAL for
 * everything hbegp_constrained_ei_* refuses about the models, fmin and limits, and for S < 1, a NULL starts / lo / hi / x_out /
 * cei_out, maxeval < 1, lo > hi or a start outside the box. */
int hbegp_maximize_constrained_ei_f64(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const double* starts, int S,
                                      const double* lo, const double* hi, double fmin_normalized, const double* limits, int maxeval,
                                      double* x_out, double* cei_out, int* nevals_out);
int hbegp_maximize_constrained_ei_f32(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const float* starts, int S,
                                      const double* lo, const double* hi, double fmin_normalized, const double* limits, int maxeval,
                                      float* x_out, double* cei_out, int* nevals_out);

/* Constrained expected improvement in log space (log EI: Ament et al. 2023): the logarithm of hbegp_constrained_ei_*'s cei, formed
 * so that the value and the gradient stay finite and informative where cei itself underflows to 0.  The models, the normalised
 * spaces, fmin_normalized, limits, HBEGP_CEI_MAX_CONSTRAINTS, "sigma = 0", the refusals, the locking order and the per-model streams
 * are exactly those of hbegp_constrained_ei_*.  With z_0 = (fmin - mu_0) / sigma_0, z_k = (t_k - mu_k) / sigma_k and
 * h(z) = z Phi(z) + phi(z):
 *   lei  = log sigma_0 + log h(z_0)      -- 0 with zero partials for fmin = +inf
 *   lF_k = log Phi(z_k)
 *   lpof = lF_1 + .. + lF_C              -- added in ascending k; 0.0 for n_con = 0
 *   lcei = lei + lpof.
 * The log of a product is a sum, so every partial of lcei is the partial of one term and none divides plain-space quantities that
 * can underflow:
 *   d lei / d mu_0 = -r(z_0) / sigma_0,   d lei / d sigma_0 = q(z_0) / sigma_0,              r = Phi / h,  q = phi / h
 *   d lF_k / d mu_k = -lambda(z_k) / sigma_k,   d lF_k / d sigma_k = -z_k lambda(z_k) / sigma_k,   lambda = phi / Phi
 *   grad[j][i] = sum_{k=0..C} (d lcei / d mu_k * dmean_k[j][i] + d lcei / d sigma_k * dvar_k[j][i] / (2 sigma_k)),  ascending k.
 * Evaluation, fp64 for both element types: for z > -1 the direct forms (h = phi(a) - a Phi(-a) for z = -a <= 0, z + h(-z) above;
 * log Phi = log1p(-Phi(-z)) for z > 0); for z = -a <= -1 through the Mills ratio u = sqrt(pi/2) erfcx(a / sqrt 2) = Phi(-a) / phi(a)
 * and b = 1 - a u = h / phi:  log h = -a^2/2 - log sqrt(2 pi) + log b,  log Phi = -a^2/2 - log sqrt(2 pi) + log u,  r = u / b,
 * q = 1 / b,  lambda = 1 / u;  from a = 25 on, a u and b come from ten terms of their asymptotic series in 1 / a^2 (below, 1 - a u
 * loses about a^2 eps to cancellation: r and q are good to about 2e-13 just below 25, to a few eps elsewhere).  z is clamped to
 * +-1.7e308.  Every value is finite for |z| <= 1e150 (about -z^2/2 on the far side); beyond, a^2 overflows and the term is -inf, or
 * stays finite for z > 0 -- never NaN.  The partials grow like |z| / sigma and z^2 / sigma and are finite while those are.
 * sigma_0 = 0: lei = log((fmin - mu_0)^+), -inf for fmin <= mu_0; d / d mu_0 = -1 / (fmin - mu_0) where that is positive, else 0;
 * d / d sigma_0 = 0.  sigma_k = 0: lF_k = 0 if t_k > mu_k, else -inf; both partials 0.  A -inf term makes lcei = -inf; the
 * gradient row is still the sum of the partials above.  A row's bits depend only on its own posteriors, fmin and limits -- not on
 * m, on the row's position, or on whether a gradient was asked for.
 * lcei[m] (required for m > 0); best (may be NULL): the LAST index of the maximum of lcei (a NaN never wins, -inf wins only where
 * no row is finite; -1 for m = 0); lei[m], lpof[m], grad[m*d], mean[m*(1+C)], var[m*(1+C)] (each may be NULL) as in
 * hbegp_constrained_ei_*: mean and var are the same bits.  A NaN coordinate gives NaN in that row of lcei, lei, lpof and grad
 * only.  n_con = 0 is log EI.  HBEGP_EINVAL and HBEGP_ENOMEM as for hbegp_constrained_ei_*. */
int hbegp_log_constrained_ei_f64(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const double* Xs, int m,
                                 double fmin_normalized, const double* limits, double* lcei, double* grad, int* best, double* lei,
                                 double* lpof, double* mean, double* var);
int hbegp_log_constrained_ei_f32(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const float* Xs, int m,
                                 double fmin_normalized, const double* limits, double* lcei, float* grad, int* best, double* lei,
                                 double* lpof, float* mean, float* var);
/* hbegp_maximize_constrained_ei_*'s S lockstep L-BFGS runs on lcei instead of cei, with the same contract: x_out[S*d], lcei_out[S]
 * each run's best evaluated point (never worse than its start) -- hbegp_log_constrained_ei_* at x_out reproduces lcei_out bit for
 * bit; nevals_out[S] (may be NULL) <= maxeval.  A value or a gradient component that is not finite is a failed evaluation, so a
 * row at -inf is one.  With n_con = 0 it maximises log EI.  Refusals as for hbegp_maximize_constrained_ei_*. */
int hbegp_maximize_log_constrained_ei_f64(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const double* starts,
                                          int S, const double* lo, const double* hi, double fmin_normalized, const double* limits,
                                          int maxeval, double* x_out, double* lcei_out, int* nevals_out);
int hbegp_maximize_log_constrained_ei_f32(hbegp_model* objective, hbegp_model* const* constraints, int n_con, const float* starts,
                                          int S, const double* lo, const double* hi, double fmin_normalized, const double* limits,
                                          int maxeval, float* x_out, double* lcei_out, int* nevals_out);

/* Max-value entropy search (MES: Wang & Jegelka, ICML 2017) under ONE model, for a minimised function: the information a noise-free
 * observation at a candidate is expected to give about the VALUE of the global minimum, from S samples y*_s of that value (the
 * f_best of hbegp_paths_minimize_*, or the row minima of hbegp_sample_posterior_* over a grid), in the model's normalised y space.
 * The posterior N(mu, sigma^2) is the latent one of hbegp_predict_* (variance without s2, clamped at 0).  ystar[S] is always
 * double, 1 <= S <= HBEGP_MES_MAX_SAMPLES.  With gamma_s = (mu - y*_s) / sigma clamped to +-1.7e308 and lambda = phi / Phi:
 *   t(g)  = g lambda(g) / 2 - log Phi(g)                     t'(g) = -(lambda / 2) (1 + g^2 + g lambda)
 *   mes   = (1/S) sum_s t(gamma_s)  >= 0                     -- lane l of a wave adds s = l, l + 64, .. in ascending s, the 64
 *                                                               partial sums go through a fixed butterfly, then the 1/S
 *   d mes / d mu = (1/S) sum t'(gamma_s) / sigma,    d mes / d sigma = -(1/S) sum gamma_s t'(gamma_s) / sigma
 *   grad[j][i] = d mes / d mu * dmean[j][i] + d mes / d sigma * dvar[j][i] / (2 sigma),
 * dmean and dvar being hbegp_predict_grad_*'s.  "sigma = 0" means !(sigma > 2.220446049250313e-16): mes = 0 and every partial is 0
 * (a point the model is certain about carries no information).  Evaluation, fp64 for both element types, with lcei's branch points:
 * for g > -1 the direct forms (Phi(-|g|) = erfc(|g| / sqrt 2) / 2, log Phi by log up to 0 and log1p(-Phi(-g)) above; g lambda and
 * t' count as 0 where phi has underflowed).  For g = -a <= -1 both terms of t grow like a^2 / 2 and cancel to O(log a); with
 * au = a sqrt(pi/2) erfcx(a / sqrt 2) and b = 1 - au:  w = a^2 b / au,  t = -w / 2 + log sqrt(2 pi) + (log a - log au),
 * t' = -(a / au) (1 - w) / 2.  From a = 25 on, au, b / x and (au - b / x) / x (x = 1 / a^2) come from ten-term asymptotic series,
 * w = (b / x) / au and 1 - w = x ((au - b / x) / x) / au; a^2 is never formed.  Against 60 digits the value is good to 5e-14
 * max(1, |t|) and t' to 1e-10 relative (worst just below a = 25, where 1 - w cancels about a^4 eps); for g > 8 the value is below
 * 1e-14 with a relative error of up to 0.5 %.  There are no atomics: a row's bits depend only on its own (mu, sigma^2, dmean, dvar)
 * and on ystar in the order given -- not on m, on the row's position, or on whether a gradient was asked for.
 * mes[m] (required for m > 0); grad[m*d] (may be NULL: no gradient launch); best (may be NULL): the LAST index of the maximum of mes
 * (a NaN never wins; -1 for m = 0); mean[m], var[m] (each may be NULL): bit for bit what hbegp_predict_* returns on its batched
 * path (m > 16), or hbegp_predict_grad_* with a gradient.  A NaN coordinate gives NaN in that row of mes and grad only.  m = 0 is
 * a no-op with best = -1.  Calls are serialised per model, like predict.
 * HBEGP_EINVAL, before any device call and without writing anything: a NULL model, a model of the other element type, m < 0, a NULL
 * Xs or mes with m > 0, S < 1 or S > HBEGP_MES_MAX_SAMPLES, a NULL ystar or a ystar that is not finite.  HBEGP_ENOMEM: m beyond
 * the device's memory. */
#define HBEGP_MES_MAX_SAMPLES 1024 /* = HBEGP_PATHS_MAX_PATHS */
int hbegp_mes_f64(hbegp_model* model, const double* Xs, int m, const double* ystar, int S, double* mes, double* grad, int* best,
                  double* mean, double* var);
int hbegp_mes_f32(hbegp_model* model, const float* Xs, int m, const double* ystar, int S, double* mes, float* grad, int* best,
                  float* mean, float* var);
/* R bounded L-BFGS runs maximising hbegp_mes_* over the box lo <= x <= hi, in lockstep: every round is one hbegp_mes_* with a
 * gradient at the points of the unfinished runs.  starts[R*d] inside the box; x_out[R*d], mes_out[R]: each run's best evaluated
 * point, never worse than its start -- hbegp_mes_* at x_out reproduces mes_out bit for bit; nevals_out[R] (may be NULL) <= maxeval.
 * A value or a gradient component that is not finite is a failed evaluation.  Refused with HBEGP_EINVAL before any device call:
 * everything hbegp_mes_* refuses about the model, ystar and S, and everything hbegp_maximize_ei_* refuses about R (its S), the
 * box, the starts, maxeval and the outputs. */
int hbegp_maximize_mes_f64(hbegp_model* model, const double* starts, int R, const double* lo, const double* hi, const double* ystar,
                           int S, int maxeval, double* x_out, double* mes_out, int* nevals_out);
int hbegp_maximize_mes_f32(hbegp_model* model, const float* starts, int R, const double* lo, const double* hi, const double* ystar,
                           int S, int maxeval, float* x_out, double* mes_out, int* nevals_out);

/* The confidence bound of ONE model, cb = mu + kappa sigma, in the model's normalised y space: the reference's
 * predict_confidence_bound (kappa > 0: the pessimistic value suggest_optimum minimises) and, with kappa < 0, GP-LCB (Srinivas et
 * al., ICML 2010).  The posterior N(mu, sigma^2) is the latent one of hbegp_predict_* (variance without s2, clamped at 0).
 *   cb[j]      = mu + kappa sigma                                 sigma = sqrt(var), stored as double
 *   grad[j][i] = dmean[j][i] + kappa (dvar[j][i] / (2 sigma))     rounded to the element type once
 * dmean and dvar being hbegp_predict_grad_*'s.  Every operation is one correctly rounded fp64 operation for both element types
 * (no fused multiply-add), so the two lines above, evaluated in double on the returned posteriors, give the same bits.
 * "sigma = 0" means !(sigma > 2.220446049250313e-16): cb = mu and grad = dmean, the sigma term is dropped and never divided.
 * kappa = 0 drops it too: cb is mean widened to double and grad holds dmean's bits.  There are no atomics: a row's bits depend only on
 * its own (mu, sigma^2, dmean, dvar) and kappa -- not on m, on the row's position, or on whether a gradient was asked for.
 * cb[m] (required for m > 0); grad[m*d] (may be NULL: no gradient launch); best (may be NULL): the FIRST index of the minimum of cb
 * (a NaN never wins; -1 for m = 0 and where every row is NaN) -- first, because the reference replaces its suggestion only on a
 * strictly lower bound; mean[m], var[m] (each may be NULL): bit for bit what hbegp_predict_* returns on its batched path (m > 16),
 * or hbegp_predict_grad_* with a gradient.  A NaN coordinate gives NaN in that row of cb and grad only.  m = 0 is a no-op with
 * best = -1.  Calls are serialised per model, like predict.
 * HBEGP_EINVAL, before any device call and without writing anything: a kappa that is not finite (either sign and 0 are valid), a
 * NULL model, a model of the other element type, m < 0, a NULL Xs or cb with m > 0.  HBEGP_ENOMEM: m beyond the device's memory. */
int hbegp_confidence_bound_f64(hbegp_model* model, const double* Xs, int m, double kappa, double* cb, double* grad, int* best,
                               double* mean, double* var);
int hbegp_confidence_bound_f32(hbegp_model* model, const float* Xs, int m, double kappa, double* cb, float* grad, int* best, float* mean,
                               float* var);
/* S bounded L-BFGS runs MINIMISING hbegp_confidence_bound_* over the box lo <= x <= hi, in lockstep: every round is one
 * hbegp_confidence_bound_* with a gradient at the points of the unfinished runs (the device alternative to the reference's 150
 * single-point BOBYQA evaluations in suggest_optimum).  starts[S*d] inside the box; x_out[S*d], cb_out[S]: each run's best
 * evaluated point, never worse than its start -- hbegp_confidence_bound_* at x_out reproduces cb_out bit for bit; nevals_out[S]
 * (may be NULL) <= maxeval.  A value or a gradient component that is not finite is a failed evaluation.  A start with a NaN
 * coordinate is admitted and fails its own run alone: that run returns its start, cb_out = +inf and one evaluation, the others
 * what they return without it.  Refused with HBEGP_EINVAL before any device call: everything hbegp_confidence_bound_* refuses
 * about the model and kappa, and everything hbegp_maximize_ei_* refuses about S, the box, starts outside it, maxeval and the
 * outputs. */
int hbegp_minimize_confidence_bound_f64(hbegp_model* model, const double* starts, int S, const double* lo, const double* hi, double kappa,
                                        int maxeval, double* x_out, double* cb_out, int* nevals_out);
int hbegp_minimize_confidence_bound_f32(hbegp_model* model, const float* starts, int S, const double* lo, const double* hi, double kappa,
                                        int maxeval, float* x_out, double* cb_out, int* nevals_out);

/* Sensitivity of the posterior mean mu (hbegp_predict_*'s mean, normalised y space) to each feature, from the CALLER's sample
 * matrices in the feature coordinates the model was fitted on (the RNG stays on the caller side).  Both calls evaluate the mean at
 * base rows with ONE coordinate substituted,
 *   mu(a | k <- s) = sum_j c phi(r_j) alpha_j,   r_j^2 = sum_{l != k} ((a_l - x_jl) / ell_l)^2 + ((s - x_jk) / ell_k)^2,
 * in one fused pass: no query matrix and no K* are formed.  r^2 is accumulated in the element type from non-negative terms only (a
 * substituted point that coincides with a training row has r^2 == 0 exactly); the Matern map, the sums over j and every reduction
 * are fp64 in a fixed order without atomics.  Every value depends only on its own row (and k, and the substituted value): the same
 * bits alone or in a batch, whatever the library's internal slabs of rows.
 *
 * hbegp_sobol_*: variance-based (Sobol) indices by pick-freeze sampling.  A[N*d], B[N*d]: two independent sample matrices.  With
 * f_A[i] = mu(A_i), f_B[i] = mu(B_i), f_AB[k][i] = mu(A_i | k <- B_ik), rounded to the element type (the optional outputs f_a[N],
 * f_b[N], f_ab[d*N] with f_ab[k*N + i]; may be NULL):
 *   f0 = mean of the 2N values f_A and f_B,   V = their mean squared deviation from f0,
 *   first[k] = (1/N) sum_i (f_B[i] - f0) (f_AB[k][i] - f_A[i]) / V      (Saltelli et al. 2010),
 *   total[k] = (1/(2N)) sum_i (f_A[i] - f_AB[k][i])^2 / V               (Jansen 1999);   V == 0 gives first = total = 0.
 * first[d], total[d] (required), *f0, *variance (may be NULL) are double.
 *
 * hbegp_main_effects_*: main-effect (partial dependence) curves (Friedman 2001).  A[N*d]: the sample; grid[d*G]: G values per
 * feature (grid[k*G + g]);  effect[k*G + g] = (1/N) sum_i mu(A_i | k <- grid[k][g])  (required, double), the rows added in
 * ascending i; f_a[N] (may be NULL): mu(A_i).  N = 1 gives one row's conditional curve.
 *
 * HBEGP_EINVAL (before any device call; a refused call writes nothing) for a NULL model, A, B, first or total (sobol), a NULL grid
 * or effect (main effects), N < 2 (sobol), N < 1 (main effects), G < 1, or a model of the other element type.  The rows are not
 * screened: a NaN coordinate makes that row's values NaN (and with them the sums the row enters), nothing else, and nothing is left
 * behind for a later call.  Serialised per model like predict.  The workspace is the chunk partial sums of one slab of rows, at
 * most 128 MiB (one row's worth where a single row needs more) plus the samples and the per-row values; work that does not fit in
 * device memory is HBEGP_ENOMEM.  HBEGP_SENS_SLAB_ROWS (environment, read per call) forces the slab size: tests only. */
int hbegp_sobol_f64(hbegp_model* model, const double* A, const double* B, int N, double* first, double* total, double* f0,
                    double* variance, double* f_a, double* f_b, double* f_ab);
int hbegp_sobol_f32(hbegp_model* model, const float* A, const float* B, int N, double* first, double* total, double* f0,
                    double* variance, float* f_a, float* f_b, float* f_ab);
int hbegp_main_effects_f64(hbegp_model* model, const double* A, int N, const double* grid, int G, double* effect, double* f_a);
int hbegp_main_effects_f32(hbegp_model* model, const float* A, int N, const float* grid, int G, double* effect, float* f_a);

/* Batch expected improvement by Monte Carlo (q-EI) in the normalised y space like hbegp_predict_*, for B batches of q points:
 * Xb[B*q*d] (batch b = rows b*q .. b*q + q - 1, feature space), z[S*q] the CALLER's standard normals (draw s = row s), shared by
 * every batch (common random numbers; the RNG stays on the caller side).  Per batch b:
 *   mu_a = the batched predict mean;  Sigma = K**(X_b, X_b) + (1e-5 + jitter) I - Q_b^T Q_b, the matrix hbegp_predict_cov returns
 *   for those q points, to rounding (here formed by fp64 dots);  L = chol(Sigma), lower, factored in fp64 for both element types;
 *   per draw s: f_s = mu + L z_s,  j_s = argmin_a f_s,a (ties to the lowest index, as hbegp_sample_posterior),
 *   I_s = max(0, fmin - f_s,j_s);   qei[b] = (1/S) sum_s I_s, summed in fp64 in ascending s.
 * grad[B*q*d] (may be NULL): the exact gradient of that sample average for the given z (defined almost everywhere: ties and
 * I_s = 0 are measure-zero kinks), reverse mode in fp64:
 *   mubar_a = -(1/S) #{s : I_s > 0, j_s = a},   Lbar_ac = -(1/S) sum_{s : I_s > 0, j_s = a} z_s,c  (c <= a),
 *   X = L^-T Phi(L^T Lbar) L^-1 (Phi: lower triangle, halved diagonal; Murray 2016),  Sigmabar = (X + X^T) / 2,
 *   dqEI/dx_a,k = mubar_a dmu_a/dx_a,k + 2 sum_c Sigmabar_ac (dk(x_a, x_c)/dx_a,k - w_a,k . q_c),
 *   w_a,k = L_K^-1 dk*_a / dx_a,k (hbegp_predict_grad's bounded form), q_c = L_K^-1 k*_c; dk with hbegp_predict_grad's psi and its
 *   convention at r = 0, so the c = a term is -w_a,a . q_a; no derivative of the jitter.  For q = 1 this is
 *   (1/S) sum_{I_s > 0} (-dmean - z_s dvar / (2 sigma)) with hbegp_predict_grad's dmean / dvar.
 * info[B] (may be NULL): 0, or 1 + the first column whose pivot failed in that batch's factor; such a batch gets qei NaN and a zero
 * gradient, the others stay valid, and the call returns HBEGP_NOT_PD after writing every output.  No automatic jitter increase.
 * 1 <= q <= 64, S >= 1, B >= 0 (B = 0 is a no-op).  HBEGP_EINVAL (before any device call) for a NULL model, q out of range, B < 0,
 * S < 1, a NULL z, a non-finite fmin, a jitter < 0 or not finite, a non-finite coordinate or a model of the other element type.
 * Work that does not fit in device memory (Kstar / Q, and with a gradient G and W: d B q n_p elements each) is HBEGP_ENOMEM.
 * Fixed-order sums, no atomics: the same call gives the same bits, and a batch's outputs do not depend on the other batches of the
 * call.  Serialised per model like predict: threads may call it on one model at once. */
int hbegp_qei_f64(hbegp_model* model, const double* Xb, int B, int q, const double* z, int S, double fmin_normalized, double jitter,
                  double* qei, double* grad, int* info);
int hbegp_qei_f32(hbegp_model* model, const float* Xb, int B, int q, const float* z, int S, double fmin_normalized, double jitter,
                  double* qei, float* grad, int* info);

/* Maximise q-EI over batches: R bounded L-BFGS ascents (the fit optimiser's method and constants, lbfgs_step.hpp with a host state
 * sized per run), each over the q*d coordinates of one batch, [lo, hi] (d entries) applied to every point; run r starts at
 * starts[r*q*d ..] (inside the box).  The runs advance in lockstep: one hbegp_qei call per round over the runs still going, with
 * the same z every round (a deterministic sample-average objective).  A batch whose factor fails is a failed evaluation (objective
 * +inf); f32 points are rounded into the box.  x_out[R*q*d]: the best batch each run evaluated, qei_out[R] its qEI (never below
 * the qEI at the start; bit for bit hbegp_qei at x_out; a run whose every evaluation failed, its start included, keeps the start
 * with qei_out = -inf), nevals_out[R] (may be NULL) the evaluations used (<= maxeval).
 * HBEGP_EINVAL for R < 1, maxeval < 1, lo > hi, a start outside the box, or any hbegp_qei check. */
int hbegp_maximize_qei_f64(hbegp_model* model, const double* starts, int R, int q, const double* lo, const double* hi, const double* z,
                           int S, double fmin_normalized, double jitter, int maxeval, double* x_out, double* qei_out, int* nevals_out);
int hbegp_maximize_qei_f32(hbegp_model* model, const float* starts, int R, int q, const double* lo, const double* hi, const float* z,
                           int S, double fmin_normalized, double jitter, int maxeval, float* x_out, double* qei_out, int* nevals_out);

/* Leave-one-out cross-validation of the model on its own training data, in closed form (Rasmussen & Williams 5.4.2), in the
 * model's normalised y space.  With K = c Matern(X, X) + s2 I, M = K^-1, m_i = M_ii:
 *   mean[i] = y_i - alpha_i / m_i    the prediction of y_i from the other n - 1 rows at the model's theta
 *   var[i]  = 1 / m_i                the predictive variance of the OBSERVATION y_i: it includes the noise s2 (the latent
 *                                    function's is var[i] - s2).  hbegp_predict_* predicts the latent function (c + 1e-5 - ..):
 *                                    deleting row i, extending at the same theta and predicting at x_i gives mean[i] and
 *                                    var[i] - s2 + 1e-5
 *   lpd[i]  = 1/2 ln m_i - alpha_i^2 / (2 m_i) - 1/2 ln 2 pi     the log predictive density of y_i;    *loo = sum_i lpd[i]
 * m_i is the column sum of squares of L^-1, sum_{a >= i} (L^-1)_ai^2 -- positive terms only, summed in fp64 in a fixed order for
 * both element types; the diagonal of the stored K^-1 loses digits in proportion to cond(K) (DESIGN.md sections 10, 15).
 * grad[p]: d loo / d theta at the model's theta, order [ln s2, ln c, ln ell_k], as hbegp_problem_eval_loo returns it
 * (R&W eq. 5.13 reduced to one symmetric n^3 product for all p parameters: DESIGN.md section 15).
 * mean, var, lpd [n] have the model's element type; loo and grad are fp64.  Every output may be NULL, but not all of them.
 * Two work matrices of n_p^2 elements (n_p = n rounded up to 128) are borrowed from the block pool only when grad is asked for;
 * work that does not fit in device memory is HBEGP_ENOMEM.  HBEGP_EINVAL (before any device call) when every output is NULL, for a
 * NULL model or a model of the other element type.  A value that is not finite (NaN data) is HBEGP_NOT_PD with *loo = -inf and
 * grad = 0.  Serialised per model like predict: threads may call it on one model at once; the same call gives the same bits. */
int hbegp_model_loo_f64(hbegp_model* model, double* mean, double* var, double* lpd, double* loo, double* grad);
int hbegp_model_loo_f32(hbegp_model* model, float* mean, float* var, float* lpd, double* loo, double* grad);

/* Leave-group-out cross-validation of the model on its own training data, in closed form, in the model's
 * normalised y space: every group of rows is predicted from all rows outside it.  Where rows are replicates, near-duplicates or
 * measured together, leave-one-out predicts a row from its twins and reports a confidence the model does not have.
 * group[n] (NULL: every row is its own group, which is leave-one-out): one label per training row, any int values; the labels are
 * mapped to dense ids 0 .. G - 1 in order of first appearance.  A group holds at most HBEGP_LGO_MAX_GROUP rows (HBEGP_EINVAL with a
 * message that names the label and its size otherwise).  With K = c Matern + diag(s2 + v_i), M = K^-1 and a group's row set I (s rows):
 *   Sigma_g = (M_II)^-1            the covariance of the OBSERVATIONS y_I given all other rows (it includes the noise, as
 *                                  hbegp_model_loo's var does);  var[i] = its diagonal entry of row i
 *   r_g     = Sigma_g alpha_I,     mean[i] = y_i - r_g[i]
 *   lpd[g]  = -1/2 alpha_I^T r_g + 1/2 ln|M_II| - s/2 ln 2 pi     indexed by dense id;   *lgo = sum_g lpd[g];   *n_groups = G
 * M_II is the Gram matrix of the group's columns of L^-1, summed in fp64 in a fixed order for both element types, never a block of
 * the stored K^-1; a row's mean and var depend on its group's row set alone, not on labels or on the other groups.
 * grad[p]: d lgo / d theta, order [ln s2, ln c, ln ell_k]: leave-one-out's one symmetric n^3 product with a block-diagonal weight.
 * mean, var [n] and lpd [at most n] have the model's element type; lgo and grad are fp64.  Every output may be NULL, but not all
 * of them.  Memory, HBEGP_EINVAL and threading as hbegp_model_loo_*.  A group whose M_II or B_g = 1/2 (r_g r_g^T + Sigma_g) has a
 * pivot that is not positive, or a value that is not finite (NaN data), is HBEGP_NOT_PD with *lgo = -inf and grad = 0. */
#define HBEGP_LGO_MAX_GROUP 64
int hbegp_model_lgo_f64(hbegp_model* model, const int* group, double* mean, double* var, double* lpd, int* n_groups, double* lgo,
                        double* grad);
int hbegp_model_lgo_f32(hbegp_model* model, const int* group, float* mean, float* var, float* lpd, int* n_groups, double* lgo,
                        double* grad);

int hbegp_model_info(const hbegp_model* model, int* n, int* d, int* is_f32, double* nu, double* lml);
/* theta[p] (log space, clamped), alpha[n], kinv[n*n] full symmetric; any pointer may be NULL. */
int hbegp_model_get_f64(hbegp_model* model, double* theta, double* alpha, double* kinv);
int hbegp_model_get_f32(hbegp_model* model, double* theta, float* alpha, float* kinv);
/* Reference counting for `Clone`/`Drop` of the Rust wrapper (gpr.rs:53; models are kept for the whole run,
 * minimize.rs:331).  Device memory is freed on the last release. */
void hbegp_model_retain(hbegp_model* model);
void hbegp_model_release(hbegp_model* model);

/* ---- host-side optimiser, exposed for its own tests (mirrors minimize_by_gradient, gradmin.rs:35-60) --------- */
typedef double (*hbegp_objective_fn)(const double* x, double* grad, void* user);
/* Bounded L-BFGS minimisation; x is updated in place; returns the best objective value found. */
double hbegp_minimize_by_gradient(hbegp_objective_fn f, void* user, double* x, const double* lo, const double* hi,
                                  int n, int maxeval);

/* ---- test hook: raw copy of a slot's work matrix after the last evaluation (np x np row-major, np = n rounded up to 128;
 * which = 1: W1 (Schur complements / U), 2: W2 (X = L^-1), 3: W3 (the factor L; right-looking task queue and f32
 * refinement only), 4: the K^-1 buffer the last evaluation wrote (lower tiles, not mirrored).  out holds np*np elements of
 * the problem's type. */
int hbegp_problem_debug_get_f64(hbegp_problem* prob, int dev, int slot, int which, double* out);
int hbegp_problem_debug_get_f32(hbegp_problem* prob, int dev, int slot, int which, float* out);

/* ---- test hook: the kernel parameters every posterior query of the model evaluates with (its device copy of noise,
 * amplitude, ell_1..ell_d), copied into out[d + 2].  For a device-driven fit these are the numbers the captured evaluation ran
 * with, which can differ from exp(theta) of the reported theta in the last bit.  HBEGP_EINVAL for a NULL model or out. */
int hbegp_model_debug_params(hbegp_model* model, double* out);

/* ---- test hook (host only, no GPU): build the task queue of the device-scheduled factorisation for `nblocks`
 * 128-blocks (bk = contraction elements per stage: 16 for f64, 32 for f32; nodes up to small_h blocks wide use 64x64
 * tiles; nwg > 0: order the queue by a list schedule simulated for nwg workgroups; fine bit 0: per-row-block dependencies,
 * bit 1: must be 0 (a plan variant removed in round 5), bit 2: the tiles of K^-1 = X^T X follow in the same queue,
 * bit 3: the right-looking plan instead of the recursion, bit 4: its row-progressive inverse and K^-1) and
 * check it: queue order topological (=> deadlock-free for any number of resident workgroups), every wait for a full
 * count, no unordered access to a tile.  crit_us / sim_us: critical path and simulated makespan under the host's task
 * time estimates.  Returns HBEGP_OK or HBEGP_EINVAL with the reason in err. */
int hbegp_debug_dag_plan(int nblocks, int bk, int small_h, int nwg, int fine, int* ntasks, int* ncounters, int* nleaf,
                         double* gflop, double* crit_us, double* sim_us, char* err, int errlen);

/* ---- test hook (host only, no GPU): the host's bounded L-BFGS state machine (csrc/lbfgs_step.hpp) fed with a RECORDED sequence
 * of evaluations -- f[i] (objective, +inf for a failed evaluation) and g[i*n ..] (its gradient) are what evaluation i returned;
 * requested[i*n ..] receives the point the state machine asks for as evaluation i (requested[0] = the clipped start point),
 * n_requested how many points it asked for (<= count).  lo / hi: the box in the optimiser's coordinates.  memory <= 0: the
 * default.  The GPU tests replay the trace of a run of the persistent fit kernel (a wave-wide transcription of the same method,
 * gradmin.rs:35-60) through it and compare every point. */
int hbegp_debug_lbfgs_replay(int n, const double* x0, const double* lo, const double* hi, int maxeval, int memory, int fixed_work,
                             int count, const double* f, const double* g, double* requested, int* n_requested);

/* ---- test hook (host only, no GPU): the same replay, with the decision query a two-phase evaluation asks before it pays for a
 * gradient (csrc/lbfgs_step.hpp: lbfgs_is_trial / lbfgs_trial_accepted).  Per evaluation i: trial[i] = it is a line-search trial,
 * accepted[i] = the query's answer for f[i] before the state machine sees it, took[i] = lbfgs_advance then took its accepted
 * branch (read the gradient).  accepted == took at every evaluation is what the fit relies on. */
int hbegp_debug_lbfgs_decisions(int n, const double* x0, const double* lo, const double* hi, int maxeval, int memory, int fixed_work,
                                int count, const double* f, const double* g, double* requested, int* trial, int* accepted, int* took,
                                int* n_requested);

/* ---- test hook (host only, no GPU): the queues of a task-queue evaluation.  which = 0: the full plan (K^-1 tiles included),
 * 1: the plan without them (first phase of a lazily evaluated trial), 2: the full plan's K^-1 tasks alone, in its order (second
 * phase).  nblocks .. fine as in hbegp_debug_dag_plan (bit 2 is implied by `which`; bit 5: the K^-1 sums of the top-left quadrant
 * are not split in two, as in a fit with several slots), big128 as HBEGP_DAG_BIG128.  tasks (may be NULL)
 * receives 6 ints per task -- kind, flags, row0, col0, kbeg, kend -- for the first cap tasks in queue order.  The queue is checked
 * as in hbegp_debug_dag_plan. */
int hbegp_debug_dag_queues(int nblocks, int bk, int small_h, int nwg, int fine, int big128, int which, int* ntasks, int* tasks, int cap,
                           char* err, int errlen);

/* ---- test hook (host only, no GPU): a queue as hbegp_debug_dag_queues builds it, ordered for order_wg workers (0: nwg, the
 * launch's own count; -1: for no count, strictly by bottom level among the tasks whose predecessors are in the queue), and its
 * in-order replay on `workers` workgroups (0: none) under the planner's task times: each workgroup claims the next index when
 * free, the task starts when its counters are complete.  tasks (may be NULL) receives 18 ints per task -- kind, flags, row0, col0,
 * kbeg, kend, nwait, 4 counters waited for, their 4 values, 3 counters bumped (65535: unused).  out (may be NULL) receives 6
 * doubles: the replay's makespan (us), its waiting and busy time (CU x us), the planner's sim_us and crit_us, and the planner cost
 * of the 128x128 tasks with beta = 1.  hbegp_debug_dag_order_wg: the library's default order_wg (0: the launch's own count) for
 * queue 0 / 1 / 2 (fused, phase 1, K^-1 alone) of an even (share 0), lead (1) or lag (2) launch of nwg workgroups, where the
 * problem's even launch has even_wg. */
int hbegp_debug_dag_replay(int nblocks, int bk, int small_h, int nwg, int order_wg, int fine, int big128, int which, int workers,
                           int* ntasks, int* tasks, int cap, double* out, char* err, int errlen);
int hbegp_debug_dag_order_wg(int queue, int share, int nwg, int even_wg, int nblocks, int n_slots);

/* ---- test hook (host only, no GPU): the rule by which a 128x128 task-queue tile skips structurally zero operand halves
 * (HBEGP_DAG_ZERO_SKIP; csrc/engine.hpp: dag_zero_halves), for a task's flags, row0, col0, kbeg, kend and the stage depth bk.
 * out receives 8 ints: the leading stages in which A's rows row0.., A's rows row0 + 64.., B's columns col0.., B's columns
 * col0 + 64.. lie wholly above the diagonal of the inverse factor, then the trailing stages in the same order.  An operand that
 * does not live in the inverse factor's matrix gets zeros. */
int hbegp_debug_dag_zero_halves(int flags, int row0, int col0, int kbeg, int kend, int bk, int* out);

/* ---- test hooks (host only, no GPU): the share policy of a fit's slots (csrc/slot_share.hpp).  Per slot of one
 * problem on one device: running[i] != 0 while the slot is inside an optimiser run, done[i] the evaluations that run has completed,
 * maxeval[i] its cap.  share[i] receives 0 (even), 1 (lead) or 2 (lag).  hysteresis < 0: the library's default.  lead_wg / lag_wg
 * (may be NULL): the default workgroup counts of a lead / lag launch where an even launch has even_wg workgroups on cus compute
 * units.  hbegp_debug_fits_in_flight: hbegp_fit_* / hbegp_fit_loo_* calls in flight on a device id, counted from the call on. */
int hbegp_debug_slot_shares(int n_slots, const int* running, const int* done, const int* maxeval, int hysteresis, int* share, int even_wg,
                            int cus, int* lead_wg, int* lag_wg);
int hbegp_debug_fits_in_flight(int device_id);

/* ---- test hook (tests/test_gpu_pool_hygiene.py): how many blocks of the device pool, and how many bytes, have been filled on
 * hand-out under HBEGP_POOL_POISON (1: the word 0x40490FDB, finite in both element types; 2: 0x7FF80000, a quiet NaN in both)
 * since the process started.  Either pointer may be NULL.  Needs no GPU. */
int hbegp_debug_pool_poisoned(long long* blocks, long long* bytes);
/* ---- timing hook (tools/posterior_cov_bench.py): phase_ms[4] (may be NULL) receives the device time of the phases of the
 * calling thread's last timed hbegp_sample_posterior_* call -- Q (Kstar, mean, Q = Kstar L^-T), Sigma, its factor, the draws
 * (upload of z, Z L^T, epilogue) -- in milliseconds; then enable != 0 makes this thread's later sampling calls timed (events
 * around the phases on the model stream). */
int hbegp_debug_posterior_phases(int enable, double* phase_ms);
/* ---- timing hook (tools/batch_select_bench.py): phase_ms[2] (may be NULL) receives the device time of the phases of the
 * calling thread's last timed hbegp_select_batch_* call -- Sigma (upload, K*, mean, Q, kmat, Q Q^T, mirror), the selection
 * kernel -- in milliseconds; then enable != 0 makes this thread's later selection calls timed. */
int hbegp_debug_batch_select_phases(int enable, double* phase_ms);
/* ---- timing hook (tools/kg_bench.py): phase_ms[2] (may be NULL) receives the device time of the phases of the calling thread's
 * last timed hbegp_knowledge_gradient_* call -- Sigma (upload, K*, mean, Q, kmat, Q Q^T, mirror), kg (the per-candidate kernel and
 * the epilogue) -- in milliseconds; then enable != 0 makes this thread's later knowledge-gradient calls timed. */
int hbegp_debug_kg_phases(int enable, double* phase_ms);
/* ---- timing hook (tools/nei_bench.py): phase_ms[4] (may be NULL) receives the device time of the phases of the calling thread's
 * last timed hbegp_noisy_ei_* call -- Sigma (upload, K*, mean, Q, kmat, Q Q^T, the padding), the baseline's factor, the panel and
 * draw products (with the upload of z), the reductions -- in milliseconds; then enable != 0 makes this thread's later noisy-EI
 * calls timed. */
int hbegp_debug_nei_phases(int enable, double* phase_ms);
/* ---- timing hook (tools/ehvi_bench.py): phase_ms[3] (may be NULL) receives the device time of the phases of the calling thread's
 * last timed hbegp_ehvi_* call -- objective 0's predict and objective 1's (each with its upload, on its own stream: they overlap),
 * the EHVI kernel with the arg-max -- in milliseconds; then enable != 0 makes this thread's later EHVI calls timed. */
int hbegp_debug_ehvi_phases(int enable, double* phase_ms);
/* ---- timing hook (tools/ehvi_nd_bench.py): phase_ms[5] (may be NULL) receives the device time of the phases of the calling
 * thread's last timed hbegp_ehvi_nd_* call -- objective 0's predict .. objective n_obj - 1's (each with its upload, on its own
 * stream: they overlap), then the box kernel with the arg-max; the entries behind these n_obj + 1 are 0 -- in milliseconds; then
 * enable != 0 makes this thread's later hbegp_ehvi_nd_* calls timed. */
int hbegp_debug_ehvi_nd_phases(int enable, double* phase_ms);
/* ---- the box decomposition of hbegp_ehvi_nd_*, on the host alone (no device is touched; for the tests of the decomposition).
 * front[P*n_obj], ref[n_obj] and their refusals as there.  thr_count[n_obj] receives the number of thresholds per objective:
 * -inf, the distinct coordinates of the reduced front ascending, r_k; *n_boxes the number of boxes.  With thr_cap = box_cap = 0
 * nothing else is written.  Otherwise thr[thr_cap] receives the thresholds, objective 0's first, and boxes[box_cap * 2 * n_obj]
 * per box and objective (l, u) as indices into that objective's thresholds (0 = -inf), in the order the kernel sums them;
 * HBEGP_EINVAL when a cap is below its count.  HBEGP_ENOMEM past HBEGP_EHVI_ND_MAX_BOXES boxes. */
int hbegp_debug_ehvi_boxes(const double* front, int P, int n_obj, const double* ref, int* thr_count, double* thr, int thr_cap,
                           int* n_boxes, int* boxes, int box_cap);
/* ---- timing hook (tools/cei_bench.py): phase_ms[2] (may be NULL) receives the device time of the phases of the calling thread's
 * last timed hbegp_constrained_ei_* call -- the 1 + C predicts (from the objective's upload to the join of the streams: they
 * overlap), the cEI kernel with the arg-max -- in milliseconds; then enable != 0 makes this thread's later cEI calls timed. */
int hbegp_debug_cei_phases(int enable, double* phase_ms);
/* ---- timing hook (tools/lcei_bench.py): phase_ms[2] (may be NULL) receives the device time of the phases of the calling thread's
 * last timed hbegp_log_constrained_ei_* call -- the 1 + C predicts as above, the log-space kernel with the arg-max -- in
 * milliseconds; then enable != 0 makes this thread's later log-cEI calls timed.  A record of its own: cEI's is not touched. */
int hbegp_debug_lcei_phases(int enable, double* phase_ms);
/* ---- timing hook (tools/mes_bench.py): phase_ms[2] (may be NULL) receives the device time of the phases of the calling thread's
 * last timed hbegp_mes_* call -- the predict (the uploads of the candidates and of ystar, the batched predict's launches and, with
 * a gradient, the gradient's), the MES kernel with the arg-max -- in milliseconds; then enable != 0 makes this thread's later MES
 * calls timed (the rounds of hbegp_maximize_mes_* too: the record holds the last one). */
int hbegp_debug_mes_phases(int enable, double* phase_ms);
/* ---- timing hook (tools/cb_bench.py): phase_ms[2] (may be NULL) receives the device time of the phases of the calling thread's
 * last timed hbegp_confidence_bound_* call -- the predict (the upload of the candidates, the batched predict's launches and, with a
 * gradient, the gradient's), the confidence-bound kernel with the arg-min -- in milliseconds; then enable != 0 makes this thread's
 * later calls timed (the rounds of hbegp_minimize_confidence_bound_* too: the record holds the last one). */
int hbegp_debug_cb_phases(int enable, double* phase_ms);
/* ---- timing hook (tools/sens_bench.py): phase_ms[4] (may be NULL) receives the device time of the phases of the calling thread's
 * last timed hbegp_sobol_* / hbegp_main_effects_* call -- the upload (with the grid's scaling), the substituted means, the chunk and
 * row sums (both summed over the slabs), the final reduction with the downloads -- in milliseconds; then enable != 0 makes this
 * thread's later sensitivity calls timed. */
int hbegp_debug_sens_phases(int enable, double* phase_ms);
/* ---- timing hook (tools/qei_bench.py): phase_ms[2] (may be NULL) receives the device time of the phases of the calling thread's
 * last timed hbegp_qei_* call -- the shared launches (upload of the points, Kstar, mean, Q; with a gradient dmean, G, W; upload of
 * z), the qEI kernel -- in milliseconds; then enable != 0 makes this thread's later qEI calls timed. */
int hbegp_debug_qei_phases(int enable, double* phase_ms);

/* ---- timing hook (tools/loo_bench.py): phase_ms[4] (may be NULL) receives the device time of the phases of the calling thread's
 * last timed leave-one-out call with a gradient (hbegp_model_loo_*, hbegp_problem_eval_loo) -- the diagonal pass, u and Y, the
 * SYRK C = Y Y^T, the weighted trace -- in milliseconds; then enable != 0 makes this thread's later calls timed. */
int hbegp_debug_loo_phases(int enable, double* phase_ms);

/* ---- timing hook (tools/lgo_bench.py): as hbegp_debug_loo_phases for the leave-group-out calls with a gradient (hbegp_model_lgo_*,
 * hbegp_problem_eval_lgo): phase_ms[4] = the group pass, u and Y, the SYRK C = Y Y^T, the weighted trace. */
int hbegp_debug_lgo_phases(int enable, double* phase_ms);

/* ---- posterior sample paths: draws of the posterior that are FUNCTIONS (pathwise conditioning, Matheron's rule, on a
 * random-Fourier-feature prior draw).  In the model's normalised y space,
 *   f_s(x) = phi(x) . w_s + k(x, X) . v_s,    v_s = K^-1 (y - Phi(X) w_s - sqrt(sigma^2) eps_s),   K = k(X, X) + sigma^2 I
 *   phi_j(x) = sqrt(2 c / F) cos(om_j . x + b_j),   om_jk = omega0_jk / ell_k
 * All randomness is the caller's: omega0[F*d] drawn from the kernel's spectral density at unit length scale (nu = inf: standard
 * normals; Matern nu: a standard normal vector divided by sqrt(chi2_{2 nu} / (2 nu)) per feature), phase[F] uniform in
 * [0, 2 pi), w[S*F] standard normals, eps[S*n] standard normals or NULL (no noise draw: eps = 0; bit-identical to zeros).
 * hbegp_paths_create_* computes v on the device through L^-1 (two triangular tile products over all S right-hand sides,
 * never the stored K^-1) and keeps V, w and the scaled frequencies there.  The handle retains the model (the model may be
 * released first) and lives on the model's device.
 * Limits: 1 <= F <= HBEGP_PATHS_MAX_FEATURES, 1 <= S <= HBEGP_PATHS_MAX_PATHS; larger values are HBEGP_EINVAL, never
 * truncated.  The handle holds 8 (S F + F d + F) bytes and S_p n_p elements; the preparation borrows at most max(128 MiB, 8 n S bytes) of
 * partial sums and two more S_p n_p operands from the block pool (S_p, n_p: rounded up to 128), and gives them back.
 *
 * hbegp_paths_eval_*: f[S*m] (path-major) and, unless df is NULL, df[S*m*d] = d f_s / d x at
 *   per_path = 0: the same m points Xs[m*d] for every path;   per_path = 1: path s at its own m points Xs[(s*m + i)*d ..].
 * The phase, sin / cos, the kernel's slope psi and every sum are fp64 for both element types; r^2 is formed as in hbegp_predict_*.
 * A training point at r = 0 contributes 0 to the gradient (as in hbegp_predict_grad_*).  A NaN in a query row gives NaN in that
 * row's outputs only.  Sums run in a fixed order without atomics, and a (path, point) pair's sums do not depend on the rest of
 * the call: the same pair gives the same bits alone, in a batch of any m, with shared or per-path points, from any thread.
 * m = 0 is a no-op.  Points are evaluated in blocks, so m is bounded only by the caller's arrays.
 *
 * hbegp_paths_minimize_*: S*R bounded L-BFGS descents (the fit optimiser's method and constants), R per path from
 * starts[(s*R + r)*d ..] inside [lo, hi], in lockstep: one per-path evaluation per round over the runs still going.  Each path
 * returns the best point any of its R runs evaluated: x_best[S*d], f_best[S] (the value hbegp_paths_eval_* gives there, bit for
 * bit), n_evals[S] (may be NULL; summed over the path's runs).  f32 points are rounded into the box.  d <= 66 (the optimiser's
 * state).  maxeval >= 1 is per run. */
#define HBEGP_PATHS_MAX_FEATURES 16384
#define HBEGP_PATHS_MAX_PATHS 1024
typedef struct hbegp_paths hbegp_paths;
int hbegp_paths_create_f64(hbegp_model* model, const double* omega0, const double* phase, const double* w, const double* eps, int F, int S,
                           hbegp_paths** paths);
int hbegp_paths_create_f32(hbegp_model* model, const float* omega0, const float* phase, const float* w, const float* eps, int F, int S,
                           hbegp_paths** paths);
int hbegp_paths_eval_f64(hbegp_paths* paths, const double* Xs, int m, int per_path, double* f, double* df);
int hbegp_paths_eval_f32(hbegp_paths* paths, const float* Xs, int m, int per_path, float* f, float* df);
int hbegp_paths_minimize_f64(hbegp_paths* paths, const double* starts, int R, const double* lo, const double* hi, int maxeval,
                             double* x_best, double* f_best, int* n_evals);
int hbegp_paths_minimize_f32(hbegp_paths* paths, const float* starts, int R, const double* lo, const double* hi, int maxeval,
                             float* x_best, double* f_best, int* n_evals);
/* n, d of the model, F, S, element type; any pointer may be NULL */
int hbegp_paths_info(const hbegp_paths* paths, int* n, int* d, int* n_features, int* n_paths, int* is_f32);
void hbegp_paths_release(hbegp_paths* paths);
/* ---- timing hook (tools/paths_bench.py): phase_ms[3] (may be NULL) receives the device time of the phases of the calling
 * thread's last timed hbegp_paths_create_* call -- uploads and the frequency scaling, the feature projection, the two triangular
 * products -- in milliseconds; then enable != 0 makes this thread's later create calls timed. */
int hbegp_debug_paths_phases(int enable, double* phase_ms);
/* ---- test hooks (host only, no GPU): the size-dependent splits of the sample paths, from the functions the engine itself calls.
 * hbegp_debug_paths_eval_blocks: *mb = the points per block of hbegp_paths_eval_* with m points on a handle of S paths and F
 * features over a model of n rows and d features -- min(m, 262144 / S, 256 MiB / (8 (ceil(n/512) + ceil(F/512)) S (d + 1))), at
 * least 1; a call with m > mb runs ceil(m / mb) blocks, and a lockstep round of the minimiser is such a call with per-path points.
 * hbegp_debug_paths_project_chunks: the projection of hbegp_paths_create_* walks F features in *nch chunks of *fch (a multiple of
 * 32; the last chunk may be shorter), *cap = min(64, 128 MiB / (8 S n)), at least 1, being the most chunks its partial sums allow.
 * Any output pointer of the second may be NULL.  HBEGP_EINVAL for sizes the entry points refuse (n, d < 1, m < 0, F or S outside
 * their limits). */
int hbegp_debug_paths_eval_blocks(int n, int d, int n_features, int n_paths, int m, int* mb);
int hbegp_debug_paths_project_chunks(int n_features, int n, int n_paths, int* cap, int* nch, int* fch);

#ifdef __cplusplus
}
#endif
#endif /* HBEGP_H */
