//! `EstimatorGpu` / `SurrogateModelGpu`: hbetune's GP surrogate on an MI355X through libhbegp.so.
//!
//! Drop-in for `EstimatorGPR` / `SurrogateModelGPR` (src/core/gpr.rs:54-63, 215-338): implements the same two traits,
//! `Estimator<A>` and `SurrogateModel<A>` (src/core/surrogate_model.rs:6-65), so `Minimizer::minimize` and everything
//! above it stay untouched.  Everything below `FittedKernel::new/extend` (src/gpr/fit.rs:18-68) and `predict`
//! (src/gpr/predict.rs:7-52) runs in hand-written HIP kernels; what stays here is the O(n) host work the reference
//! keeps in its adapter: y-normalisation, the amplitude heuristic, defaults and prior reuse, expected improvement,
//! summary statistics.
//!
//! STATUS: written out in full, NEVER COMPILED -- the repository that ships it has no Rust toolchain in its build
//! image (cargo / rustc absent).  It targets the reference at the commit surveyed (ndarray 0.13, statrs 0.12,
//! edition 2018).  Behaviour is pinned by the Python mirror of the same adapter (hbetune_rs_amd/estimator.py), which is
//! tested against the reference's own suites (tests/test_gpu_estimator.py restates tests/gpr_tests.rs).
//!
//! Installation in the hbetune crate:
//!   1. copy this file to `src/core/gpr_gpu.rs`, integration/build.rs to `build.rs`;
//!   2. `src/core/mod.rs`:  `#[cfg(feature = "gpu")] pub mod gpr_gpu;`
//!      `src/lib.rs`:       `#[cfg(feature = "gpu")] pub use crate::core::gpr_gpu::{EstimatorGpu, SurrogateModelGpu};`
//!   3. `src/bin/hbetune/main.rs:240-244`: select `command_run::<A, EstimatorGpu>` behind a `--gpu` flag
//!      (the function is already generic over the estimator: minimize.rs:231-241).
//! The one addition to the trait surface that pays on a GPU is `predict_confidence_bound_a` (batched confidence bound for
//! `find_best_individual_by_confidence_bound`, minimize.rs:680-714); it is provided as an inherent method.

use std::ffi::CStr;
use std::os::raw::{c_char, c_double, c_float, c_int};

use ndarray::prelude::*;

use crate::core::acquisition::expected_improvement;
use crate::core::surrogate_model::SummaryStatistics;
use crate::core::ynormalize::{Projection, YNormalize};
use crate::util::{BoundedValue, BoundsError};
use crate::{Estimator, Scalar, Space, SurrogateModel, RNG};

// ------------------------------------------------------------------------------------------------------------------
// FFI: 1:1 with include/hbegp.h (ABI 0.2.0)
// ------------------------------------------------------------------------------------------------------------------
#[repr(C)]
pub struct HbegpCtx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct HbegpModel {
    _private: [u8; 0],
}
#[repr(C)]
pub struct HbegpProblem {
    _private: [u8; 0],
}

/// `hbegp_fit_options` (include/hbegp.h)
#[repr(C)]
pub struct HbegpFitOptions {
    /// `size_of::<HbegpFitOptions>()`: the library copies min(struct_size, its own size), so the struct may grow at its end
    pub struct_size: usize,
    pub maxeval: c_int,
    pub fixed_work: c_int,
    pub lbfgs_memory: c_int,
    pub trace_cap: c_int,
    pub trace_theta: *mut c_double,
    pub trace_lml: *mut c_double,
    pub trace_grad: *mut c_double,
    pub trace_run: *mut c_int,
    pub trace_count: *mut c_int,
    pub n_evals: *mut c_int,
    pub n_not_pd: *mut c_int,
}

pub const HBEGP_OK: c_int = 0;
pub const HBEGP_NOT_PD: c_int = 1;
pub const HBEGP_ALL_FAILED: c_int = 2;

extern "C" {
    fn hbegp_version() -> c_int;
    fn hbegp_device_count() -> c_int;
    fn hbegp_ctx_create(n_devices: c_int, device_ids: *const c_int, out: *mut *mut HbegpCtx) -> c_int;
    fn hbegp_ctx_destroy(ctx: *mut HbegpCtx);
    fn hbegp_last_error() -> *const c_char;

    fn hbegp_fit_f64(
        ctx: *mut HbegpCtx, x: *const c_double, y: *const c_double, n: c_int, d: c_int, nu: c_double,
        theta0: *const c_double, lo: *const c_double, hi: *const c_double, starts: *const c_double, n_restarts: c_int,
        opt: *const HbegpFitOptions, theta_best: *mut c_double, lml_best: *mut c_double, model: *mut *mut HbegpModel,
    ) -> c_int;
    fn hbegp_fit_f32(
        ctx: *mut HbegpCtx, x: *const c_float, y: *const c_float, n: c_int, d: c_int, nu: c_double,
        theta0: *const c_double, lo: *const c_double, hi: *const c_double, starts: *const c_double, n_restarts: c_int,
        opt: *const HbegpFitOptions, theta_best: *mut c_double, lml_best: *mut c_double, model: *mut *mut HbegpModel,
    ) -> c_int;
    fn hbegp_extend_f64(
        ctx: *mut HbegpCtx, x: *const c_double, y: *const c_double, n: c_int, d: c_int, nu: c_double,
        theta: *const c_double, lo: *const c_double, hi: *const c_double, model: *mut *mut HbegpModel,
    ) -> c_int;
    fn hbegp_extend_f32(
        ctx: *mut HbegpCtx, x: *const c_float, y: *const c_float, n: c_int, d: c_int, nu: c_double,
        theta: *const c_double, lo: *const c_double, hi: *const c_double, model: *mut *mut HbegpModel,
    ) -> c_int;
    fn hbegp_extend_from_f64(
        ctx: *mut HbegpCtx, prior: *mut HbegpModel, x: *const c_double, y: *const c_double, n: c_int,
        model: *mut *mut HbegpModel, incremental: *mut c_int,
    ) -> c_int;
    fn hbegp_extend_from_f32(
        ctx: *mut HbegpCtx, prior: *mut HbegpModel, x: *const c_float, y: *const c_float, n: c_int,
        model: *mut *mut HbegpModel, incremental: *mut c_int,
    ) -> c_int;
    fn hbegp_predict_f64(
        model: *mut HbegpModel, xs: *const c_double, m: c_int, mean: *mut c_double, var: *mut c_double, n_warn: *mut c_int,
    ) -> c_int;
    fn hbegp_predict_f32(
        model: *mut HbegpModel, xs: *const c_float, m: c_int, mean: *mut c_float, var: *mut c_float, n_warn: *mut c_int,
    ) -> c_int;
    fn hbegp_predict_grad_f64(
        model: *mut HbegpModel, xs: *const c_double, m: c_int, mean: *mut c_double, var: *mut c_double, dmean: *mut c_double,
        dvar: *mut c_double, n_warn: *mut c_int,
    ) -> c_int;
    fn hbegp_predict_grad_f32(
        model: *mut HbegpModel, xs: *const c_float, m: c_int, mean: *mut c_float, var: *mut c_float, dmean: *mut c_float,
        dvar: *mut c_float, n_warn: *mut c_int,
    ) -> c_int;
    fn hbegp_maximize_ei_f64(
        model: *mut HbegpModel, starts: *const c_double, s: c_int, lo: *const c_double, hi: *const c_double,
        fmin_normalized: c_double, maxeval: c_int, x_out: *mut c_double, ei_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    fn hbegp_maximize_ei_f32(
        model: *mut HbegpModel, starts: *const c_float, s: c_int, lo: *const c_double, hi: *const c_double,
        fmin_normalized: c_double, maxeval: c_int, x_out: *mut c_float, ei_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    fn hbegp_predict_cov_f64(
        model: *mut HbegpModel, xs: *const c_double, m: c_int, jitter: c_double, mean: *mut c_double, cov: *mut c_double,
    ) -> c_int;
    fn hbegp_predict_cov_f32(
        model: *mut HbegpModel, xs: *const c_float, m: c_int, jitter: c_double, mean: *mut c_float, cov: *mut c_float,
    ) -> c_int;
    fn hbegp_sample_posterior_f64(
        model: *mut HbegpModel, xs: *const c_double, m: c_int, z: *const c_double, s: c_int, jitter: c_double,
        samples: *mut c_double, argmin: *mut c_int, info: *mut c_int,
    ) -> c_int;
    fn hbegp_sample_posterior_f32(
        model: *mut HbegpModel, xs: *const c_float, m: c_int, z: *const c_float, s: c_int, jitter: c_double,
        samples: *mut c_float, argmin: *mut c_int, info: *mut c_int,
    ) -> c_int;
    fn hbegp_select_batch_f64(
        model: *mut HbegpModel, xs: *const c_double, m: c_int, k: c_int, fmin_normalized: c_double, lie: *const c_double,
        idx: *mut c_int, ei: *mut c_double, mean_out: *mut c_double, var_out: *mut c_double,
    ) -> c_int;
    fn hbegp_select_batch_f32(
        model: *mut HbegpModel, xs: *const c_float, m: c_int, k: c_int, fmin_normalized: c_double, lie: *const c_double,
        idx: *mut c_int, ei: *mut c_double, mean_out: *mut c_float, var_out: *mut c_float,
    ) -> c_int;
    fn hbegp_knowledge_gradient_f64(
        model: *mut HbegpModel, xs: *const c_double, m: c_int, mc: c_int, kg: *mut c_double, best: *mut c_int, imin: *mut c_int,
        mean_out: *mut c_double, var_out: *mut c_double,
    ) -> c_int;
    fn hbegp_knowledge_gradient_f32(
        model: *mut HbegpModel, xs: *const c_float, m: c_int, mc: c_int, kg: *mut c_double, best: *mut c_int, imin: *mut c_int,
        mean_out: *mut c_float, var_out: *mut c_float,
    ) -> c_int;
    fn hbegp_ehvi_f64(
        models: *const *mut HbegpModel, n_obj: c_int, xs: *const c_double, m: c_int, front: *const c_double, p: c_int,
        reference: *const c_double, ehvi: *mut c_double, grad: *mut c_double, best: *mut c_int, mean: *mut c_double, var: *mut c_double,
    ) -> c_int;
    fn hbegp_ehvi_f32(
        models: *const *mut HbegpModel, n_obj: c_int, xs: *const c_float, m: c_int, front: *const c_double, p: c_int,
        reference: *const c_double, ehvi: *mut c_double, grad: *mut c_float, best: *mut c_int, mean: *mut c_float, var: *mut c_float,
    ) -> c_int;
    fn hbegp_ehvi_nd_f64(
        models: *const *mut HbegpModel, n_obj: c_int, xs: *const c_double, m: c_int, front: *const c_double, p: c_int,
        reference: *const c_double, ehvi: *mut c_double, grad: *mut c_double, best: *mut c_int, mean: *mut c_double, var: *mut c_double,
    ) -> c_int;
    fn hbegp_ehvi_nd_f32(
        models: *const *mut HbegpModel, n_obj: c_int, xs: *const c_float, m: c_int, front: *const c_double, p: c_int,
        reference: *const c_double, ehvi: *mut c_double, grad: *mut c_float, best: *mut c_int, mean: *mut c_float, var: *mut c_float,
    ) -> c_int;
    fn hbegp_constrained_ei_f64(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, xs: *const c_double, m: c_int,
        fmin_normalized: c_double, limits: *const c_double, cei: *mut c_double, grad: *mut c_double, best: *mut c_int,
        ei: *mut c_double, pof: *mut c_double, mean: *mut c_double, var: *mut c_double,
    ) -> c_int;
    fn hbegp_maximize_constrained_ei_f64(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, starts: *const c_double, s: c_int,
        lo: *const c_double, hi: *const c_double, fmin_normalized: c_double, limits: *const c_double, maxeval: c_int,
        x_out: *mut c_double, cei_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    fn hbegp_constrained_ei_f32(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, xs: *const c_float, m: c_int,
        fmin_normalized: c_double, limits: *const c_double, cei: *mut c_double, grad: *mut c_float, best: *mut c_int,
        ei: *mut c_double, pof: *mut c_double, mean: *mut c_float, var: *mut c_float,
    ) -> c_int;
    fn hbegp_maximize_constrained_ei_f32(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, starts: *const c_float, s: c_int,
        lo: *const c_double, hi: *const c_double, fmin_normalized: c_double, limits: *const c_double, maxeval: c_int,
        x_out: *mut c_float, cei_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    #[allow(dead_code)]
    fn hbegp_debug_cei_phases(enable: c_int, phase_ms: *mut c_double) -> c_int;
    fn hbegp_log_constrained_ei_f64(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, xs: *const c_double, m: c_int,
        fmin_normalized: c_double, limits: *const c_double, lcei: *mut c_double, grad: *mut c_double, best: *mut c_int,
        lei: *mut c_double, lpof: *mut c_double, mean: *mut c_double, var: *mut c_double,
    ) -> c_int;
    fn hbegp_maximize_log_constrained_ei_f64(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, starts: *const c_double, s: c_int,
        lo: *const c_double, hi: *const c_double, fmin_normalized: c_double, limits: *const c_double, maxeval: c_int,
        x_out: *mut c_double, lcei_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    fn hbegp_log_constrained_ei_f32(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, xs: *const c_float, m: c_int,
        fmin_normalized: c_double, limits: *const c_double, lcei: *mut c_double, grad: *mut c_float, best: *mut c_int,
        lei: *mut c_double, lpof: *mut c_double, mean: *mut c_float, var: *mut c_float,
    ) -> c_int;
    fn hbegp_maximize_log_constrained_ei_f32(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, starts: *const c_float, s: c_int,
        lo: *const c_double, hi: *const c_double, fmin_normalized: c_double, limits: *const c_double, maxeval: c_int,
        x_out: *mut c_float, lcei_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    #[allow(dead_code)]
    fn hbegp_debug_lcei_phases(enable: c_int, phase_ms: *mut c_double) -> c_int;
    fn hbegp_mes_f64(
        model: *mut HbegpModel, xs: *const c_double, m: c_int, ystar: *const c_double, s: c_int, mes: *mut c_double, grad: *mut c_double,
        best: *mut c_int, mean: *mut c_double, var: *mut c_double,
    ) -> c_int;
    fn hbegp_maximize_mes_f64(
        model: *mut HbegpModel, starts: *const c_double, r: c_int, lo: *const c_double, hi: *const c_double, ystar: *const c_double,
        s: c_int, maxeval: c_int, x_out: *mut c_double, mes_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    fn hbegp_mes_f32(
        model: *mut HbegpModel, xs: *const c_float, m: c_int, ystar: *const c_double, s: c_int, mes: *mut c_double, grad: *mut c_float,
        best: *mut c_int, mean: *mut c_float, var: *mut c_float,
    ) -> c_int;
    fn hbegp_maximize_mes_f32(
        model: *mut HbegpModel, starts: *const c_float, r: c_int, lo: *const c_double, hi: *const c_double, ystar: *const c_double,
        s: c_int, maxeval: c_int, x_out: *mut c_float, mes_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    #[allow(dead_code)]
    fn hbegp_debug_mes_phases(enable: c_int, phase_ms: *mut c_double) -> c_int;
    fn hbegp_minimize_confidence_bound_f64(
        model: *mut HbegpModel, starts: *const c_double, s: c_int, lo: *const c_double, hi: *const c_double, kappa: c_double,
        maxeval: c_int, x_out: *mut c_double, cb_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    fn hbegp_minimize_confidence_bound_f32(
        model: *mut HbegpModel, starts: *const c_float, s: c_int, lo: *const c_double, hi: *const c_double, kappa: c_double,
        maxeval: c_int, x_out: *mut c_float, cb_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    fn hbegp_noisy_ei_f64(
        model: *mut HbegpModel, xs: *const c_double, m: c_int, mb: c_int, z: *const c_double, s: c_int, jitter: c_double,
        nei: *mut c_double, best: *mut c_int, fmin_draws: *mut c_double, rho: *mut c_double, info: *mut c_int,
    ) -> c_int;
    fn hbegp_noisy_ei_f32(
        model: *mut HbegpModel, xs: *const c_float, m: c_int, mb: c_int, z: *const c_float, s: c_int, jitter: c_double,
        nei: *mut c_double, best: *mut c_int, fmin_draws: *mut c_double, rho: *mut c_double, info: *mut c_int,
    ) -> c_int;
    fn hbegp_sobol_f64(
        model: *mut HbegpModel, a: *const c_double, b: *const c_double, n: c_int, first: *mut c_double, total: *mut c_double,
        f0: *mut c_double, variance: *mut c_double, f_a: *mut c_double, f_b: *mut c_double, f_ab: *mut c_double,
    ) -> c_int;
    fn hbegp_sobol_f32(
        model: *mut HbegpModel, a: *const c_float, b: *const c_float, n: c_int, first: *mut c_double, total: *mut c_double,
        f0: *mut c_double, variance: *mut c_double, f_a: *mut c_float, f_b: *mut c_float, f_ab: *mut c_float,
    ) -> c_int;
    fn hbegp_main_effects_f64(
        model: *mut HbegpModel, a: *const c_double, n: c_int, grid: *const c_double, g: c_int, effect: *mut c_double,
        f_a: *mut c_double,
    ) -> c_int;
    fn hbegp_main_effects_f32(
        model: *mut HbegpModel, a: *const c_float, n: c_int, grid: *const c_float, g: c_int, effect: *mut c_double,
        f_a: *mut c_float,
    ) -> c_int;
    fn hbegp_qei_f64(
        model: *mut HbegpModel, xb: *const c_double, b: c_int, q: c_int, z: *const c_double, s: c_int, fmin_normalized: c_double,
        jitter: c_double, qei: *mut c_double, grad: *mut c_double, info: *mut c_int,
    ) -> c_int;
    fn hbegp_qei_f32(
        model: *mut HbegpModel, xb: *const c_float, b: c_int, q: c_int, z: *const c_float, s: c_int, fmin_normalized: c_double,
        jitter: c_double, qei: *mut c_double, grad: *mut c_float, info: *mut c_int,
    ) -> c_int;
    fn hbegp_maximize_qei_f64(
        model: *mut HbegpModel, starts: *const c_double, r: c_int, q: c_int, lo: *const c_double, hi: *const c_double,
        z: *const c_double, s: c_int, fmin_normalized: c_double, jitter: c_double, maxeval: c_int, x_out: *mut c_double,
        qei_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    fn hbegp_maximize_qei_f32(
        model: *mut HbegpModel, starts: *const c_float, r: c_int, q: c_int, lo: *const c_double, hi: *const c_double,
        z: *const c_float, s: c_int, fmin_normalized: c_double, jitter: c_double, maxeval: c_int, x_out: *mut c_float,
        qei_out: *mut c_double, nevals_out: *mut c_int,
    ) -> c_int;
    fn hbegp_model_info(
        model: *const HbegpModel, n: *mut c_int, d: *mut c_int, is_f32: *mut c_int, nu: *mut c_double, lml: *mut c_double,
    ) -> c_int;
    fn hbegp_model_get_f64(model: *mut HbegpModel, theta: *mut c_double, alpha: *mut c_double, kinv: *mut c_double) -> c_int;
    fn hbegp_model_get_f32(model: *mut HbegpModel, theta: *mut c_double, alpha: *mut c_float, kinv: *mut c_float) -> c_int;
    fn hbegp_model_retain(model: *mut HbegpModel);
    fn hbegp_model_release(model: *mut HbegpModel);
    // input warping (include/hbegp.h; declared to keep the block in step with the header, the binding does not wrap them yet):
    // ab = [a_1..a_d, b_1..b_d]; every output of hbegp_warp_apply may be null
    pub fn hbegp_warp_apply(
        ab: *const c_double, d: c_int, x: *const c_double, m: c_int, u: *mut c_double, du_dlna: *mut c_double, du_dlnb: *mut c_double,
        du_dx: *mut c_double,
    ) -> c_int;
    pub fn hbegp_warp_invert(ab: *const c_double, d: c_int, u: *const c_double, m: c_int, x: *mut c_double) -> c_int;
    pub fn hbegp_problem_eval_xgrad(
        prob: *mut HbegpProblem, dev: c_int, slot: c_int, theta: *const c_double, lo: *const c_double, hi: *const c_double,
        lml: *mut c_double, grad: *mut c_double, gx: *mut c_double,
    ) -> c_int;
    pub fn hbegp_problem_eval_warped(
        prob: *mut HbegpProblem, dev: c_int, slot: c_int, theta: *const c_double, lo: *const c_double, hi: *const c_double,
        ab: *const c_double, lml: *mut c_double, grad: *mut c_double,
    ) -> c_int;
    pub fn hbegp_fit_warped_f64(
        ctx: *mut HbegpCtx, x: *const c_double, y: *const c_double, rv: *const c_double, n: c_int, d: c_int, nu: c_double,
        theta0: *const c_double, lo: *const c_double, hi: *const c_double, ab0: *const c_double, ab_lo: *const c_double,
        ab_hi: *const c_double, starts: *const c_double, n_restarts: c_int, opt: *const HbegpFitOptions, theta_best: *mut c_double,
        ab_best: *mut c_double, lml_best: *mut c_double, model: *mut *mut HbegpModel,
    ) -> c_int;
    pub fn hbegp_fit_warped_f32(
        ctx: *mut HbegpCtx, x: *const c_float, y: *const c_float, rv: *const c_double, n: c_int, d: c_int, nu: c_double,
        theta0: *const c_double, lo: *const c_double, hi: *const c_double, ab0: *const c_double, ab_lo: *const c_double,
        ab_hi: *const c_double, starts: *const c_double, n_restarts: c_int, opt: *const HbegpFitOptions, theta_best: *mut c_double,
        ab_best: *mut c_double, lml_best: *mut c_double, model: *mut *mut HbegpModel,
    ) -> c_int;
    pub fn hbegp_model_warp(model: *const HbegpModel, ab: *mut c_double) -> c_int;
}

fn last_error() -> String {
    unsafe {
        let p = hbegp_last_error();
        if p.is_null() {
            String::new()
        } else {
            CStr::from_ptr(p).to_string_lossy().into_owned()
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// A = f64 | f32 dispatch (src/gpr/scalar.rs:3-30; `--use-32`, src/bin/hbetune/main.rs:240-244)
// ------------------------------------------------------------------------------------------------------------------
mod sealed {
    pub trait Sealed {}
    impl Sealed for f64 {}
    impl Sealed for f32 {}
}

/// The two element types libhbegp carries.  Sealed: the library has exactly these two instantiations.
pub trait GpuScalar: Scalar + sealed::Sealed {
    /// `hbegp_fit_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_fit(
        ctx: *mut HbegpCtx, x: *const Self, y: *const Self, n: c_int, d: c_int, nu: f64, theta0: *const f64,
        lo: *const f64, hi: *const f64, starts: *const f64, n_restarts: c_int, opt: *const HbegpFitOptions,
        theta_best: *mut f64, lml_best: *mut f64, model: *mut *mut HbegpModel,
    ) -> c_int;
    /// `hbegp_extend_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_extend(
        ctx: *mut HbegpCtx, x: *const Self, y: *const Self, n: c_int, d: c_int, nu: f64, theta: *const f64,
        lo: *const f64, hi: *const f64, model: *mut *mut HbegpModel,
    ) -> c_int;
    /// `hbegp_extend_from_*`
    unsafe fn ffi_extend_from(
        ctx: *mut HbegpCtx, prior: *mut HbegpModel, x: *const Self, y: *const Self, n: c_int,
        model: *mut *mut HbegpModel, incremental: *mut c_int,
    ) -> c_int;
    /// `hbegp_predict_*`
    unsafe fn ffi_predict(
        model: *mut HbegpModel, xs: *const Self, m: c_int, mean: *mut Self, var: *mut Self, n_warn: *mut c_int,
    ) -> c_int;
    /// `hbegp_predict_grad_*`
    unsafe fn ffi_predict_grad(
        model: *mut HbegpModel, xs: *const Self, m: c_int, mean: *mut Self, var: *mut Self, dmean: *mut Self, dvar: *mut Self,
        n_warn: *mut c_int,
    ) -> c_int;
    /// `hbegp_maximize_ei_*`
    unsafe fn ffi_maximize_ei(
        model: *mut HbegpModel, starts: *const Self, s: c_int, lo: *const f64, hi: *const f64, fmin_normalized: f64,
        maxeval: c_int, x_out: *mut Self, ei_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int;
    /// `hbegp_predict_cov_*`
    unsafe fn ffi_predict_cov(
        model: *mut HbegpModel, xs: *const Self, m: c_int, jitter: f64, mean: *mut Self, cov: *mut Self,
    ) -> c_int;
    /// `hbegp_sample_posterior_*`
    unsafe fn ffi_sample_posterior(
        model: *mut HbegpModel, xs: *const Self, m: c_int, z: *const Self, s: c_int, jitter: f64, samples: *mut Self,
        argmin: *mut c_int, info: *mut c_int,
    ) -> c_int;
    /// `hbegp_select_batch_*`
    unsafe fn ffi_select_batch(
        model: *mut HbegpModel, xs: *const Self, m: c_int, k: c_int, fmin_normalized: f64, lie: *const f64, idx: *mut c_int,
        ei: *mut f64, mean_out: *mut Self, var_out: *mut Self,
    ) -> c_int;
    /// `hbegp_knowledge_gradient_*`
    unsafe fn ffi_knowledge_gradient(
        model: *mut HbegpModel, xs: *const Self, m: c_int, mc: c_int, kg: *mut f64, best: *mut c_int, imin: *mut c_int,
        mean_out: *mut Self, var_out: *mut Self,
    ) -> c_int;
    /// `hbegp_ehvi_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_ehvi(
        models: *const *mut HbegpModel, n_obj: c_int, xs: *const Self, m: c_int, front: *const f64, p: c_int, reference: *const f64,
        ehvi: *mut f64, grad: *mut Self, best: *mut c_int, mean: *mut Self, var: *mut Self,
    ) -> c_int;
    /// `hbegp_ehvi_nd_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_ehvi_nd(
        models: *const *mut HbegpModel, n_obj: c_int, xs: *const Self, m: c_int, front: *const f64, p: c_int, reference: *const f64,
        ehvi: *mut f64, grad: *mut Self, best: *mut c_int, mean: *mut Self, var: *mut Self,
    ) -> c_int;
    /// `hbegp_constrained_ei_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, xs: *const Self, m: c_int, fmin_normalized: f64,
        limits: *const f64, cei: *mut f64, grad: *mut Self, best: *mut c_int, ei: *mut f64, pof: *mut f64, mean: *mut Self,
        var: *mut Self,
    ) -> c_int;
    /// `hbegp_maximize_constrained_ei_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_maximize_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, starts: *const Self, s: c_int, lo: *const f64,
        hi: *const f64, fmin_normalized: f64, limits: *const f64, maxeval: c_int, x_out: *mut Self, cei_out: *mut f64,
        nevals_out: *mut c_int,
    ) -> c_int;
    /// `hbegp_log_constrained_ei_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_log_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, xs: *const Self, m: c_int, fmin_normalized: f64,
        limits: *const f64, cei: *mut f64, grad: *mut Self, best: *mut c_int, ei: *mut f64, pof: *mut f64, mean: *mut Self,
        var: *mut Self,
    ) -> c_int;
    /// `hbegp_maximize_log_constrained_ei_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_maximize_log_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, starts: *const Self, s: c_int, lo: *const f64,
        hi: *const f64, fmin_normalized: f64, limits: *const f64, maxeval: c_int, x_out: *mut Self, cei_out: *mut f64,
        nevals_out: *mut c_int,
    ) -> c_int;
    /// `hbegp_mes_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_mes(
        model: *mut HbegpModel, xs: *const Self, m: c_int, ystar: *const f64, s: c_int, mes: *mut f64, grad: *mut Self,
        best: *mut c_int, mean: *mut Self, var: *mut Self,
    ) -> c_int;
    /// `hbegp_maximize_mes_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_maximize_mes(
        model: *mut HbegpModel, starts: *const Self, r: c_int, lo: *const f64, hi: *const f64, ystar: *const f64, s: c_int,
        maxeval: c_int, x_out: *mut Self, mes_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int;
    /// `hbegp_minimize_confidence_bound_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_minimize_confidence_bound(
        model: *mut HbegpModel, starts: *const Self, s: c_int, lo: *const f64, hi: *const f64, kappa: f64, maxeval: c_int,
        x_out: *mut Self, cb_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int;
    /// `hbegp_noisy_ei_*`
    #[allow(clippy::too_many_arguments)]
    unsafe fn ffi_noisy_ei(
        model: *mut HbegpModel, xs: *const Self, m: c_int, mb: c_int, z: *const Self, s: c_int, jitter: f64, nei: *mut f64,
        best: *mut c_int, fmin_draws: *mut f64, rho: *mut f64, info: *mut c_int,
    ) -> c_int;
    /// `hbegp_qei_*`
    unsafe fn ffi_qei(
        model: *mut HbegpModel, xb: *const Self, b: c_int, q: c_int, z: *const Self, s: c_int, fmin_normalized: f64, jitter: f64,
        qei: *mut f64, grad: *mut Self, info: *mut c_int,
    ) -> c_int;
    /// `hbegp_maximize_qei_*`
    unsafe fn ffi_maximize_qei(
        model: *mut HbegpModel, starts: *const Self, r: c_int, q: c_int, lo: *const f64, hi: *const f64, z: *const Self, s: c_int,
        fmin_normalized: f64, jitter: f64, maxeval: c_int, x_out: *mut Self, qei_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int;
}

impl GpuScalar for f64 {
    unsafe fn ffi_fit(
        ctx: *mut HbegpCtx, x: *const f64, y: *const f64, n: c_int, d: c_int, nu: f64, theta0: *const f64,
        lo: *const f64, hi: *const f64, starts: *const f64, n_restarts: c_int, opt: *const HbegpFitOptions,
        theta_best: *mut f64, lml_best: *mut f64, model: *mut *mut HbegpModel,
    ) -> c_int {
        hbegp_fit_f64(ctx, x, y, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, lml_best, model)
    }
    unsafe fn ffi_extend(
        ctx: *mut HbegpCtx, x: *const f64, y: *const f64, n: c_int, d: c_int, nu: f64, theta: *const f64,
        lo: *const f64, hi: *const f64, model: *mut *mut HbegpModel,
    ) -> c_int {
        hbegp_extend_f64(ctx, x, y, n, d, nu, theta, lo, hi, model)
    }
    unsafe fn ffi_extend_from(
        ctx: *mut HbegpCtx, prior: *mut HbegpModel, x: *const f64, y: *const f64, n: c_int,
        model: *mut *mut HbegpModel, incremental: *mut c_int,
    ) -> c_int {
        hbegp_extend_from_f64(ctx, prior, x, y, n, model, incremental)
    }
    unsafe fn ffi_predict(
        model: *mut HbegpModel, xs: *const f64, m: c_int, mean: *mut f64, var: *mut f64, n_warn: *mut c_int,
    ) -> c_int {
        hbegp_predict_f64(model, xs, m, mean, var, n_warn)
    }
    unsafe fn ffi_predict_grad(
        model: *mut HbegpModel, xs: *const f64, m: c_int, mean: *mut f64, var: *mut f64, dmean: *mut f64, dvar: *mut f64,
        n_warn: *mut c_int,
    ) -> c_int {
        hbegp_predict_grad_f64(model, xs, m, mean, var, dmean, dvar, n_warn)
    }
    unsafe fn ffi_maximize_ei(
        model: *mut HbegpModel, starts: *const f64, s: c_int, lo: *const f64, hi: *const f64, fmin_normalized: f64,
        maxeval: c_int, x_out: *mut f64, ei_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_maximize_ei_f64(model, starts, s, lo, hi, fmin_normalized, maxeval, x_out, ei_out, nevals_out)
    }
    unsafe fn ffi_predict_cov(
        model: *mut HbegpModel, xs: *const f64, m: c_int, jitter: f64, mean: *mut f64, cov: *mut f64,
    ) -> c_int {
        hbegp_predict_cov_f64(model, xs, m, jitter, mean, cov)
    }
    unsafe fn ffi_sample_posterior(
        model: *mut HbegpModel, xs: *const f64, m: c_int, z: *const f64, s: c_int, jitter: f64, samples: *mut f64,
        argmin: *mut c_int, info: *mut c_int,
    ) -> c_int {
        hbegp_sample_posterior_f64(model, xs, m, z, s, jitter, samples, argmin, info)
    }
    unsafe fn ffi_select_batch(
        model: *mut HbegpModel, xs: *const f64, m: c_int, k: c_int, fmin_normalized: f64, lie: *const f64, idx: *mut c_int,
        ei: *mut f64, mean_out: *mut f64, var_out: *mut f64,
    ) -> c_int {
        hbegp_select_batch_f64(model, xs, m, k, fmin_normalized, lie, idx, ei, mean_out, var_out)
    }
    unsafe fn ffi_knowledge_gradient(
        model: *mut HbegpModel, xs: *const f64, m: c_int, mc: c_int, kg: *mut f64, best: *mut c_int, imin: *mut c_int,
        mean_out: *mut f64, var_out: *mut f64,
    ) -> c_int {
        hbegp_knowledge_gradient_f64(model, xs, m, mc, kg, best, imin, mean_out, var_out)
    }
    unsafe fn ffi_ehvi(
        models: *const *mut HbegpModel, n_obj: c_int, xs: *const f64, m: c_int, front: *const f64, p: c_int, reference: *const f64,
        ehvi: *mut f64, grad: *mut f64, best: *mut c_int, mean: *mut f64, var: *mut f64,
    ) -> c_int {
        hbegp_ehvi_f64(models, n_obj, xs, m, front, p, reference, ehvi, grad, best, mean, var)
    }
    unsafe fn ffi_ehvi_nd(
        models: *const *mut HbegpModel, n_obj: c_int, xs: *const f64, m: c_int, front: *const f64, p: c_int, reference: *const f64,
        ehvi: *mut f64, grad: *mut f64, best: *mut c_int, mean: *mut f64, var: *mut f64,
    ) -> c_int {
        hbegp_ehvi_nd_f64(models, n_obj, xs, m, front, p, reference, ehvi, grad, best, mean, var)
    }
    unsafe fn ffi_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, xs: *const f64, m: c_int, fmin_normalized: f64,
        limits: *const f64, cei: *mut f64, grad: *mut f64, best: *mut c_int, ei: *mut f64, pof: *mut f64, mean: *mut f64,
        var: *mut f64,
    ) -> c_int {
        hbegp_constrained_ei_f64(objective, constraints, n_con, xs, m, fmin_normalized, limits, cei, grad, best, ei, pof, mean, var)
    }
    unsafe fn ffi_maximize_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, starts: *const f64, s: c_int, lo: *const f64,
        hi: *const f64, fmin_normalized: f64, limits: *const f64, maxeval: c_int, x_out: *mut f64, cei_out: *mut f64,
        nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_maximize_constrained_ei_f64(objective, constraints, n_con, starts, s, lo, hi, fmin_normalized, limits, maxeval, x_out,
                                          cei_out, nevals_out)
    }
    unsafe fn ffi_log_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, xs: *const f64, m: c_int, fmin_normalized: f64,
        limits: *const f64, cei: *mut f64, grad: *mut f64, best: *mut c_int, ei: *mut f64, pof: *mut f64, mean: *mut f64,
        var: *mut f64,
    ) -> c_int {
        hbegp_log_constrained_ei_f64(objective, constraints, n_con, xs, m, fmin_normalized, limits, cei, grad, best, ei, pof, mean, var)
    }
    unsafe fn ffi_maximize_log_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, starts: *const f64, s: c_int, lo: *const f64,
        hi: *const f64, fmin_normalized: f64, limits: *const f64, maxeval: c_int, x_out: *mut f64, cei_out: *mut f64,
        nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_maximize_log_constrained_ei_f64(objective, constraints, n_con, starts, s, lo, hi, fmin_normalized, limits, maxeval,
                                              x_out, cei_out, nevals_out)
    }
    unsafe fn ffi_mes(
        model: *mut HbegpModel, xs: *const f64, m: c_int, ystar: *const f64, s: c_int, mes: *mut f64, grad: *mut f64,
        best: *mut c_int, mean: *mut f64, var: *mut f64,
    ) -> c_int {
        hbegp_mes_f64(model, xs, m, ystar, s, mes, grad, best, mean, var)
    }
    unsafe fn ffi_maximize_mes(
        model: *mut HbegpModel, starts: *const f64, r: c_int, lo: *const f64, hi: *const f64, ystar: *const f64, s: c_int,
        maxeval: c_int, x_out: *mut f64, mes_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_maximize_mes_f64(model, starts, r, lo, hi, ystar, s, maxeval, x_out, mes_out, nevals_out)
    }
    unsafe fn ffi_minimize_confidence_bound(
        model: *mut HbegpModel, starts: *const f64, s: c_int, lo: *const f64, hi: *const f64, kappa: f64, maxeval: c_int,
        x_out: *mut f64, cb_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_minimize_confidence_bound_f64(model, starts, s, lo, hi, kappa, maxeval, x_out, cb_out, nevals_out)
    }
    unsafe fn ffi_noisy_ei(
        model: *mut HbegpModel, xs: *const f64, m: c_int, mb: c_int, z: *const f64, s: c_int, jitter: f64, nei: *mut f64,
        best: *mut c_int, fmin_draws: *mut f64, rho: *mut f64, info: *mut c_int,
    ) -> c_int {
        hbegp_noisy_ei_f64(model, xs, m, mb, z, s, jitter, nei, best, fmin_draws, rho, info)
    }
    unsafe fn ffi_qei(
        model: *mut HbegpModel, xb: *const f64, b: c_int, q: c_int, z: *const f64, s: c_int, fmin_normalized: f64, jitter: f64,
        qei: *mut f64, grad: *mut f64, info: *mut c_int,
    ) -> c_int {
        hbegp_qei_f64(model, xb, b, q, z, s, fmin_normalized, jitter, qei, grad, info)
    }
    unsafe fn ffi_maximize_qei(
        model: *mut HbegpModel, starts: *const f64, r: c_int, q: c_int, lo: *const f64, hi: *const f64, z: *const f64, s: c_int,
        fmin_normalized: f64, jitter: f64, maxeval: c_int, x_out: *mut f64, qei_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_maximize_qei_f64(model, starts, r, q, lo, hi, z, s, fmin_normalized, jitter, maxeval, x_out, qei_out, nevals_out)
    }
}

impl GpuScalar for f32 {
    unsafe fn ffi_fit(
        ctx: *mut HbegpCtx, x: *const f32, y: *const f32, n: c_int, d: c_int, nu: f64, theta0: *const f64,
        lo: *const f64, hi: *const f64, starts: *const f64, n_restarts: c_int, opt: *const HbegpFitOptions,
        theta_best: *mut f64, lml_best: *mut f64, model: *mut *mut HbegpModel,
    ) -> c_int {
        hbegp_fit_f32(ctx, x, y, n, d, nu, theta0, lo, hi, starts, n_restarts, opt, theta_best, lml_best, model)
    }
    unsafe fn ffi_extend(
        ctx: *mut HbegpCtx, x: *const f32, y: *const f32, n: c_int, d: c_int, nu: f64, theta: *const f64,
        lo: *const f64, hi: *const f64, model: *mut *mut HbegpModel,
    ) -> c_int {
        hbegp_extend_f32(ctx, x, y, n, d, nu, theta, lo, hi, model)
    }
    unsafe fn ffi_extend_from(
        ctx: *mut HbegpCtx, prior: *mut HbegpModel, x: *const f32, y: *const f32, n: c_int,
        model: *mut *mut HbegpModel, incremental: *mut c_int,
    ) -> c_int {
        hbegp_extend_from_f32(ctx, prior, x, y, n, model, incremental)
    }
    unsafe fn ffi_predict(
        model: *mut HbegpModel, xs: *const f32, m: c_int, mean: *mut f32, var: *mut f32, n_warn: *mut c_int,
    ) -> c_int {
        hbegp_predict_f32(model, xs, m, mean, var, n_warn)
    }
    unsafe fn ffi_predict_grad(
        model: *mut HbegpModel, xs: *const f32, m: c_int, mean: *mut f32, var: *mut f32, dmean: *mut f32, dvar: *mut f32,
        n_warn: *mut c_int,
    ) -> c_int {
        hbegp_predict_grad_f32(model, xs, m, mean, var, dmean, dvar, n_warn)
    }
    unsafe fn ffi_maximize_ei(
        model: *mut HbegpModel, starts: *const f32, s: c_int, lo: *const f64, hi: *const f64, fmin_normalized: f64,
        maxeval: c_int, x_out: *mut f32, ei_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_maximize_ei_f32(model, starts, s, lo, hi, fmin_normalized, maxeval, x_out, ei_out, nevals_out)
    }
    unsafe fn ffi_predict_cov(
        model: *mut HbegpModel, xs: *const f32, m: c_int, jitter: f64, mean: *mut f32, cov: *mut f32,
    ) -> c_int {
        hbegp_predict_cov_f32(model, xs, m, jitter, mean, cov)
    }
    unsafe fn ffi_sample_posterior(
        model: *mut HbegpModel, xs: *const f32, m: c_int, z: *const f32, s: c_int, jitter: f64, samples: *mut f32,
        argmin: *mut c_int, info: *mut c_int,
    ) -> c_int {
        hbegp_sample_posterior_f32(model, xs, m, z, s, jitter, samples, argmin, info)
    }
    unsafe fn ffi_select_batch(
        model: *mut HbegpModel, xs: *const f32, m: c_int, k: c_int, fmin_normalized: f64, lie: *const f64, idx: *mut c_int,
        ei: *mut f64, mean_out: *mut f32, var_out: *mut f32,
    ) -> c_int {
        hbegp_select_batch_f32(model, xs, m, k, fmin_normalized, lie, idx, ei, mean_out, var_out)
    }
    unsafe fn ffi_knowledge_gradient(
        model: *mut HbegpModel, xs: *const f32, m: c_int, mc: c_int, kg: *mut f64, best: *mut c_int, imin: *mut c_int,
        mean_out: *mut f32, var_out: *mut f32,
    ) -> c_int {
        hbegp_knowledge_gradient_f32(model, xs, m, mc, kg, best, imin, mean_out, var_out)
    }
    unsafe fn ffi_ehvi(
        models: *const *mut HbegpModel, n_obj: c_int, xs: *const f32, m: c_int, front: *const f64, p: c_int, reference: *const f64,
        ehvi: *mut f64, grad: *mut f32, best: *mut c_int, mean: *mut f32, var: *mut f32,
    ) -> c_int {
        hbegp_ehvi_f32(models, n_obj, xs, m, front, p, reference, ehvi, grad, best, mean, var)
    }
    unsafe fn ffi_ehvi_nd(
        models: *const *mut HbegpModel, n_obj: c_int, xs: *const f32, m: c_int, front: *const f64, p: c_int, reference: *const f64,
        ehvi: *mut f64, grad: *mut f32, best: *mut c_int, mean: *mut f32, var: *mut f32,
    ) -> c_int {
        hbegp_ehvi_nd_f32(models, n_obj, xs, m, front, p, reference, ehvi, grad, best, mean, var)
    }
    unsafe fn ffi_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, xs: *const f32, m: c_int, fmin_normalized: f64,
        limits: *const f64, cei: *mut f64, grad: *mut f32, best: *mut c_int, ei: *mut f64, pof: *mut f64, mean: *mut f32,
        var: *mut f32,
    ) -> c_int {
        hbegp_constrained_ei_f32(objective, constraints, n_con, xs, m, fmin_normalized, limits, cei, grad, best, ei, pof, mean, var)
    }
    unsafe fn ffi_maximize_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, starts: *const f32, s: c_int, lo: *const f64,
        hi: *const f64, fmin_normalized: f64, limits: *const f64, maxeval: c_int, x_out: *mut f32, cei_out: *mut f64,
        nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_maximize_constrained_ei_f32(objective, constraints, n_con, starts, s, lo, hi, fmin_normalized, limits, maxeval, x_out,
                                          cei_out, nevals_out)
    }
    unsafe fn ffi_log_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, xs: *const f32, m: c_int, fmin_normalized: f64,
        limits: *const f64, cei: *mut f64, grad: *mut f32, best: *mut c_int, ei: *mut f64, pof: *mut f64, mean: *mut f32,
        var: *mut f32,
    ) -> c_int {
        hbegp_log_constrained_ei_f32(objective, constraints, n_con, xs, m, fmin_normalized, limits, cei, grad, best, ei, pof, mean, var)
    }
    unsafe fn ffi_maximize_log_constrained_ei(
        objective: *mut HbegpModel, constraints: *const *mut HbegpModel, n_con: c_int, starts: *const f32, s: c_int, lo: *const f64,
        hi: *const f64, fmin_normalized: f64, limits: *const f64, maxeval: c_int, x_out: *mut f32, cei_out: *mut f64,
        nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_maximize_log_constrained_ei_f32(objective, constraints, n_con, starts, s, lo, hi, fmin_normalized, limits, maxeval,
                                              x_out, cei_out, nevals_out)
    }
    unsafe fn ffi_mes(
        model: *mut HbegpModel, xs: *const f32, m: c_int, ystar: *const f64, s: c_int, mes: *mut f64, grad: *mut f32,
        best: *mut c_int, mean: *mut f32, var: *mut f32,
    ) -> c_int {
        hbegp_mes_f32(model, xs, m, ystar, s, mes, grad, best, mean, var)
    }
    unsafe fn ffi_maximize_mes(
        model: *mut HbegpModel, starts: *const f32, r: c_int, lo: *const f64, hi: *const f64, ystar: *const f64, s: c_int,
        maxeval: c_int, x_out: *mut f32, mes_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_maximize_mes_f32(model, starts, r, lo, hi, ystar, s, maxeval, x_out, mes_out, nevals_out)
    }
    unsafe fn ffi_minimize_confidence_bound(
        model: *mut HbegpModel, starts: *const f32, s: c_int, lo: *const f64, hi: *const f64, kappa: f64, maxeval: c_int,
        x_out: *mut f32, cb_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_minimize_confidence_bound_f32(model, starts, s, lo, hi, kappa, maxeval, x_out, cb_out, nevals_out)
    }
    unsafe fn ffi_noisy_ei(
        model: *mut HbegpModel, xs: *const f32, m: c_int, mb: c_int, z: *const f32, s: c_int, jitter: f64, nei: *mut f64,
        best: *mut c_int, fmin_draws: *mut f64, rho: *mut f64, info: *mut c_int,
    ) -> c_int {
        hbegp_noisy_ei_f32(model, xs, m, mb, z, s, jitter, nei, best, fmin_draws, rho, info)
    }
    unsafe fn ffi_qei(
        model: *mut HbegpModel, xb: *const f32, b: c_int, q: c_int, z: *const f32, s: c_int, fmin_normalized: f64, jitter: f64,
        qei: *mut f64, grad: *mut f32, info: *mut c_int,
    ) -> c_int {
        hbegp_qei_f32(model, xb, b, q, z, s, fmin_normalized, jitter, qei, grad, info)
    }
    unsafe fn ffi_maximize_qei(
        model: *mut HbegpModel, starts: *const f32, r: c_int, q: c_int, lo: *const f64, hi: *const f64, z: *const f32, s: c_int,
        fmin_normalized: f64, jitter: f64, maxeval: c_int, x_out: *mut f32, qei_out: *mut f64, nevals_out: *mut c_int,
    ) -> c_int {
        hbegp_maximize_qei_f32(model, starts, r, q, lo, hi, z, s, fmin_normalized, jitter, maxeval, x_out, qei_out, nevals_out)
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Context: devices, shared by every model of a run.  Reference-counted so that estimator and models can be cloned/moved.
// ------------------------------------------------------------------------------------------------------------------
struct Context {
    raw: *mut HbegpCtx,
}
impl Drop for Context {
    fn drop(&mut self) {
        unsafe { hbegp_ctx_destroy(self.raw) }
    }
}
impl Context {
    /// All visible gfx950 devices: the optimiser runs of a fit are sharded run r -> device r mod G (gradmin.rs:19-31 is
    /// the axis; no collective).  `HBEGP_DEVICES=k` limits the count.
    fn open() -> Result<std::rc::Rc<Context>, Error> {
        let abi = unsafe { hbegp_version() };
        if abi < 200 {
            return Err(Error::Backend(format!("libhbegp ABI {} is older than this binding (200: hbegp_fit_options.struct_size)", abi)));
        }
        let mut count = unsafe { hbegp_device_count() };
        if let Some(limit) = std::env::var("HBEGP_DEVICES").ok().and_then(|s| s.parse::<c_int>().ok()) {
            count = count.min(limit.max(1));
        }
        if count < 1 {
            return Err(Error::Backend("no gfx950 device visible: libhbegp has no CPU fallback".to_owned()));
        }
        let mut raw = std::ptr::null_mut();
        let rc = unsafe { hbegp_ctx_create(count, std::ptr::null(), &mut raw) };
        if rc != HBEGP_OK {
            return Err(Error::Backend(last_error()));
        }
        Ok(std::rc::Rc::new(Context { raw }))
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Model
// ------------------------------------------------------------------------------------------------------------------
/// Mirror of `SurrogateModelGPR<A>` (gpr.rs:54-63).  X, alpha, K^-1 live on the device behind `handle`; the host keeps
/// what `get_kernel_or_default` hands to the next fit (kernel parameters AND their bounds, gpr.rs:407-409).
pub struct SurrogateModelGpu<A: Scalar> {
    handle: *mut HbegpModel,
    ctx: std::rc::Rc<Context>,
    /// `[ln s2, ln c, ln ell_1..]`, clamped into the bounds (fit.rs:155-164)
    theta: Vec<f64>,
    /// linear-space bounds in theta order: noise, amplitude, length scales
    lo: Vec<f64>,
    hi: Vec<f64>,
    matern_nu: f64,
    y_norm: YNormalize<A>,
    lml: f64,
}

impl<A: Scalar> std::fmt::Debug for SurrogateModelGpu<A> {
    fn fmt(&self, f: &mut std::fmt::Formatter) -> std::fmt::Result {
        f.debug_struct("SurrogateModelGpu")
            .field("noise", &self.theta[0].exp())
            .field("amplitude", &self.theta[1].exp())
            .field("length_scale", &self.theta[2..].iter().map(|t| t.exp()).collect::<Vec<_>>())
            .field("matern_nu", &self.matern_nu)
            .field("lml", &self.lml)
            .field("y_norm", &self.y_norm)
            .finish()
    }
}

/// Models are kept for the whole run (`all_models`, minimize.rs:331) and `SurrogateModelGPR` is `Clone` (gpr.rs:53):
/// the device copy is shared and reference-counted by the library, freed on the last drop.
impl<A: Scalar> Clone for SurrogateModelGpu<A> {
    fn clone(&self) -> Self {
        unsafe { hbegp_model_retain(self.handle) };
        SurrogateModelGpu {
            handle: self.handle,
            ctx: self.ctx.clone(),
            theta: self.theta.clone(),
            lo: self.lo.clone(),
            hi: self.hi.clone(),
            matern_nu: self.matern_nu,
            y_norm: self.y_norm.clone(),
            lml: self.lml,
        }
    }
}

impl<A: Scalar> Drop for SurrogateModelGpu<A> {
    fn drop(&mut self) {
        unsafe { hbegp_model_release(self.handle) }
    }
}

impl<A: GpuScalar> SurrogateModelGpu<A> {
    /// log marginal likelihood of the captured evaluation (`FittedKernel::lml`, fit.rs:11)
    pub fn lml(&self) -> f64 {
        self.lml
    }

    pub fn noise(&self) -> BoundedValue<f64> {
        BoundedValue::new(self.theta[0].exp(), self.lo[0], self.hi[0]).expect("fitted noise lies in its bounds")
    }

    pub fn amplitude(&self) -> BoundedValue<f64> {
        BoundedValue::new(self.theta[1].exp(), self.lo[1], self.hi[1]).expect("fitted amplitude lies in its bounds")
    }

    /// alpha (n) and the full symmetric K^-1 (n x n) copied back from the device -- `FittedKernel::{alpha, k_inv}`
    /// (fit.rs:6-12); only needed by code that wants the CPU `predict` beside the device one.
    pub fn arrays(&self) -> (Array1<A>, Array2<A>)
    where
        A: HostCopy,
    {
        let (mut n, mut d) = (0 as c_int, 0 as c_int);
        let rc = unsafe {
            hbegp_model_info(self.handle, &mut n, &mut d, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())
        };
        assert!(rc == HBEGP_OK, "hbegp_model_info: {}", last_error());
        let n = n as usize;
        let mut alpha = Array1::<A>::zeros(n);
        let mut kinv = Array2::<A>::zeros((n, n));
        let rc = unsafe { A::ffi_model_get(self.handle, alpha.as_mut_ptr(), kinv.as_mut_ptr()) };
        assert!(rc == HBEGP_OK, "hbegp_model_get: {}", last_error());
        (alpha, kinv)
    }

    /// `predict()` (predict.rs:7-52) on the device: normalised mean and, if wanted, variance
    /// (`c + 1e-5 - k*^T K^-1 k*`, negatives clamped to 0).  Prints the reference's warning when variances fell below
    /// `-sqrt(1e-5)` before clamping (predict.rs:39-48).
    fn predict_normalized(&self, x: ArrayView2<A>, want_variance: bool) -> (Array1<A>, Option<Array1<A>>) {
        let m = x.nrows();
        let x = x.as_standard_layout(); // row-major m x d, as `project_into_features_array` produces (space.rs:141-159)
        let mut mean = Array1::<A>::zeros(m);
        let mut var = if want_variance { Some(Array1::<A>::zeros(m)) } else { None };
        if m == 0 {
            return (mean, var);
        }
        let mut n_warn: c_int = 0;
        let var_ptr = var.as_mut().map(|v| v.as_mut_ptr()).unwrap_or(std::ptr::null_mut());
        let rc = unsafe { A::ffi_predict(self.handle, x.as_ptr(), m as c_int, mean.as_mut_ptr(), var_ptr, &mut n_warn) };
        if rc != HBEGP_OK {
            panic!("hbegp_predict failed: {}", last_error());
        }
        if n_warn > 0 {
            eprintln!("Variances below 0 were predicted and will be corrected ({} values)", n_warn);
        }
        (mean, var)
    }

    /// `predict_normalized` plus the gradients w.r.t. the features (`hbegp_predict_grad_*`): mean, variance, d mean / dx
    /// and d variance / dx ([m, d]), all in the normalised y space.  Opt-in: nothing the estimator suggests uses it.
    pub fn predict_normalized_with_gradient(&self, x: ArrayView2<A>) -> (Array1<A>, Array1<A>, Array2<A>, Array2<A>) {
        let (m, d) = x.dim();
        let x = x.as_standard_layout();
        let mut mean = Array1::<A>::zeros(m);
        let mut var = Array1::<A>::zeros(m);
        let mut dmean = Array2::<A>::zeros((m, d));
        let mut dvar = Array2::<A>::zeros((m, d));
        if m == 0 {
            return (mean, var, dmean, dvar);
        }
        let mut n_warn: c_int = 0;
        let rc = unsafe {
            A::ffi_predict_grad(self.handle, x.as_ptr(), m as c_int, mean.as_mut_ptr(), var.as_mut_ptr(), dmean.as_mut_ptr(),
                                dvar.as_mut_ptr(), &mut n_warn)
        };
        if rc != HBEGP_OK {
            panic!("hbegp_predict_grad failed: {}", last_error());
        }
        (mean, var, dmean, dvar)
    }

    /// Bounded L-BFGS ascents of EI in the normalised y space from every row of `starts` inside [lo, hi]
    /// (`hbegp_maximize_ei_*`, all runs in lockstep on the device model): each run's best point, its EI and its evaluations.
    pub fn maximize_ei(&self, starts: ArrayView2<A>, lo: &[f64], hi: &[f64], fmin_normalized: f64, maxeval: usize)
        -> (Array2<A>, Vec<f64>, Vec<c_int>) {
        let (s, d) = starts.dim();
        assert!(lo.len() == d && hi.len() == d, "bounds must have one entry per feature");
        let starts = starts.as_standard_layout();
        let mut x = Array2::<A>::zeros((s, d));
        let mut ei = vec![0.0f64; s];
        let mut nevals: Vec<c_int> = vec![0; s];
        let rc = unsafe {
            A::ffi_maximize_ei(self.handle, starts.as_ptr(), s as c_int, lo.as_ptr(), hi.as_ptr(), fmin_normalized,
                               maxeval as c_int, x.as_mut_ptr(), ei.as_mut_ptr(), nevals.as_mut_ptr())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_maximize_ei failed: {}", last_error());
        }
        (x, ei, nevals)
    }

    /// Joint posterior at the rows of `x` (`hbegp_predict_cov_*`): mean [m] and covariance [m, m] in the normalised y space,
    /// cov = K** + (1e-5 + jitter) I - K*^T K^-1 K* (unclamped, exactly symmetric).  Opt-in, like the gradients.
    pub fn predict_normalized_cov(&self, x: ArrayView2<A>, jitter: f64) -> (Array1<A>, Array2<A>) {
        let (m, _d) = x.dim();
        let x = x.as_standard_layout();
        let mut mean = Array1::<A>::zeros(m);
        let mut cov = Array2::<A>::zeros((m, m));
        if m == 0 {
            return (mean, cov);
        }
        let rc = unsafe { A::ffi_predict_cov(self.handle, x.as_ptr(), m as c_int, jitter, mean.as_mut_ptr(), cov.as_mut_ptr()) };
        if rc != HBEGP_OK {
            panic!("hbegp_predict_cov failed: {}", last_error());
        }
        (mean, cov)
    }

    /// Joint draws mean + L z_s (`hbegp_sample_posterior_*`, L = cholesky(cov) of `predict_normalized_cov`) from the caller's
    /// standard normals `z` [S, m] (the RNG stays with the caller): the draws [S, m] in the normalised y space and each draw's
    /// argmin (ties to the lowest index: batch Thompson sampling for a minimiser).  Err(info) when cov is not positive definite
    /// in A (info = 1 + the failing pivot's panel column): the caller may retry with a larger jitter.
    pub fn sample_normalized(&self, x: ArrayView2<A>, z: ArrayView2<A>, jitter: f64) -> Result<(Array2<A>, Vec<usize>), c_int> {
        let (m, _d) = x.dim();
        let (s, mz) = z.dim();
        assert!(mz == m && s >= 1, "z must be [S, m] with S >= 1");
        let x = x.as_standard_layout();
        let z = z.as_standard_layout();
        let mut samples = Array2::<A>::zeros((s, m));
        let mut argmin: Vec<c_int> = vec![0; s];
        if m == 0 {
            return Ok((samples, Vec::new()));
        }
        let mut info: c_int = 0;
        let rc = unsafe {
            A::ffi_sample_posterior(self.handle, x.as_ptr(), m as c_int, z.as_ptr(), s as c_int, jitter, samples.as_mut_ptr(),
                                    argmin.as_mut_ptr(), &mut info)
        };
        if rc == HBEGP_NOT_PD {
            return Err(info);
        }
        if rc != HBEGP_OK {
            panic!("hbegp_sample_posterior failed: {}", last_error());
        }
        Ok((samples, argmin.into_iter().map(|i| i as usize).collect()))
    }

    /// Greedy batch selection by EI with fantasised observations (`hbegp_select_batch_*`): k distinct rows of `x`, each the
    /// largest EI (ties to the last index, as `max_by`) after the model was conditioned on a fantasy at every earlier pick --
    /// its mean (kriging believer, `lie = None`) or `lie` (constant liar).  `fmin_normalized` and `lie` are in the normalised
    /// y space.  Returns (indices [k], EI of each pick [k]).  k = 1 is `find_best_candidate_by_ei`.  Opt-in.
    pub fn select_batch_normalized(&self, x: ArrayView2<A>, k: usize, fmin_normalized: f64, lie: Option<f64>) -> (Vec<usize>, Vec<f64>) {
        let (m, _d) = x.dim();
        assert!(k <= m, "k must be <= the number of candidates");
        if k == 0 {
            return (Vec::new(), Vec::new());
        }
        let x = x.as_standard_layout();
        let mut idx: Vec<c_int> = vec![0; k];
        let mut ei = vec![0.0f64; k];
        let lie_ptr = lie.as_ref().map_or(std::ptr::null(), |l| l as *const f64);
        let rc = unsafe {
            A::ffi_select_batch(self.handle, x.as_ptr(), m as c_int, k as c_int, fmin_normalized, lie_ptr, idx.as_mut_ptr(),
                                ei.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_select_batch failed: {}", last_error());
        }
        (idx.into_iter().map(|i| i as usize).collect(), ei)
    }

    /// Knowledge gradient over a candidate set (`hbegp_knowledge_gradient_*`; Frazier, Powell, Dayanik 2009): for each of the first
    /// `n_candidates` rows of `x` the expected drop of the minimum of the posterior mean over ALL rows of `x` after one more noisy
    /// observation there, in closed form, in the normalised y space -- no fmin, no random numbers.  Returns (kg [n_candidates],
    /// best = the last index of its maximum as `max_by` (None without candidates), imin = the lowest index of the minimum of the
    /// posterior mean: the row a tuner of a noisy objective should recommend instead of its best observation).  Opt-in.
    pub fn knowledge_gradient_normalized(&self, x: ArrayView2<A>, n_candidates: usize) -> (Vec<f64>, Option<usize>, Option<usize>) {
        let (m, _d) = x.dim();
        assert!(n_candidates <= m, "n_candidates must be <= the number of rows");
        let x = x.as_standard_layout();
        let mut kg = vec![0.0f64; n_candidates];
        let (mut best, mut imin): (c_int, c_int) = (-1, -1);
        let kg_ptr = if n_candidates > 0 { kg.as_mut_ptr() } else { std::ptr::null_mut() };
        let rc = unsafe {
            A::ffi_knowledge_gradient(self.handle, x.as_ptr(), m as c_int, n_candidates as c_int, kg_ptr, &mut best, &mut imin,
                                      std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_knowledge_gradient failed: {}", last_error());
        }
        (kg, usize::try_from(best).ok(), usize::try_from(imin).ok())
    }

    /// Expected hypervolume improvement of TWO minimised objectives (`hbegp_ehvi_*`): `self` models objective 0, `other` objective 1
    /// (same features, element type and device; their posteriors are taken as independent).  `front` [P, 2] holds the points reached
    /// so far in any order and `reference` the reference point, both in the two models' NORMALISED y spaces (project each column
    /// with that model's `YNormalize`: the projections are monotone, so dominance is preserved; the area is measured in normalised
    /// units).  Closed form, no fmin, no random numbers.  Returns (ehvi [m], best = the last index of its maximum as `max_by`, None
    /// without rows).  Opt-in.
    pub fn ehvi_normalized(&self, other: &Self, x: ArrayView2<A>, front: ArrayView2<f64>, reference: [f64; 2]) -> (Vec<f64>, Option<usize>) {
        let (m, _d) = x.dim();
        let (p, two) = front.dim();
        assert!(p == 0 || two == 2, "front must be [P, 2]");
        let x = x.as_standard_layout();
        let front = front.as_standard_layout();
        let models = [self.handle, other.handle];
        let mut ehvi = vec![0.0f64; m];
        let mut best: c_int = -1;
        let ehvi_ptr = if m > 0 { ehvi.as_mut_ptr() } else { std::ptr::null_mut() };
        let front_ptr = if p > 0 { front.as_ptr() } else { std::ptr::null() };
        let rc = unsafe {
            A::ffi_ehvi(models.as_ptr(), 2, x.as_ptr(), m as c_int, front_ptr, p as c_int, reference.as_ptr(), ehvi_ptr,
                        std::ptr::null_mut(), &mut best, std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_ehvi failed: {}", last_error());
        }
        (ehvi, usize::try_from(best).ok())
    }

    /// Expected hypervolume improvement of two to four minimised objectives (`hbegp_ehvi_nd_*`): `self` models objective 0, `others`
    /// the objectives 1 .. (one to three models of the same features, element type and device; the posteriors are taken as
    /// independent).  `front` [P, n_obj] and `reference` [n_obj] are in the models' NORMALISED y spaces, as in `ehvi_normalized`; the
    /// volume is measured in normalised units.  The library splits the free region into boxes on the host and refuses a front that
    /// needs more than `HBEGP_EHVI_ND_MAX_BOXES` of them.  Returns (ehvi [m], best = the last index of its maximum, None without
    /// rows).  Opt-in.
    pub fn ehvi_nd_normalized(&self, others: &[&Self], x: ArrayView2<A>, front: ArrayView2<f64>, reference: &[f64]) -> (Vec<f64>, Option<usize>) {
        let n_obj = 1 + others.len();
        assert!((2..=4).contains(&n_obj), "EHVI over boxes takes two, three or four models");
        assert!(reference.len() == n_obj, "reference must hold one value per objective");
        let (m, _d) = x.dim();
        let (p, cols) = front.dim();
        assert!(p == 0 || cols == n_obj, "front must be [P, n_obj]");
        let x = x.as_standard_layout();
        let front = front.as_standard_layout();
        let mut models = vec![self.handle];
        models.extend(others.iter().map(|o| o.handle));
        let mut ehvi = vec![0.0f64; m];
        let mut best: c_int = -1;
        let ehvi_ptr = if m > 0 { ehvi.as_mut_ptr() } else { std::ptr::null_mut() };
        let front_ptr = if p > 0 { front.as_ptr() } else { std::ptr::null() };
        let rc = unsafe {
            A::ffi_ehvi_nd(models.as_ptr(), n_obj as c_int, x.as_ptr(), m as c_int, front_ptr, p as c_int, reference.as_ptr(), ehvi_ptr,
                           std::ptr::null_mut(), &mut best, std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_ehvi_nd failed: {}", last_error());
        }
        (ehvi, usize::try_from(best).ok())
    }

    /// Constrained expected improvement (`hbegp_constrained_ei_*`; Gardner et al. 2014, Gelbart et al. 2014): the EI of `self` (the
    /// minimised objective) below `fmin_normalized` times the probability that every `constraints[k]` stays at or below `limits[k]`
    /// (same features, element type and device; at most 8 constraints; the posteriors are taken as independent).  Everything is in
    /// each model's own NORMALISED y space: project fmin with the objective's `YNormalize` and each limit with its constraint's.
    /// `fmin_normalized = f64::INFINITY` means that no feasible point is known: EI counts as 1 and the result is the probability of
    /// feasibility.  Returns (cei [m], best = the last index of its maximum as `max_by`, None without rows).  Opt-in.
    pub fn constrained_ei_normalized(&self, constraints: &[&Self], x: ArrayView2<A>, fmin_normalized: f64, limits: &[f64])
        -> (Vec<f64>, Option<usize>) {
        assert_eq!(constraints.len(), limits.len(), "one limit per constraint");
        let (m, _d) = x.dim();
        let x = x.as_standard_layout();
        let handles: Vec<*mut HbegpModel> = constraints.iter().map(|c| c.handle).collect();
        let mut cei = vec![0.0f64; m];
        let mut best: c_int = -1;
        let cei_ptr = if m > 0 { cei.as_mut_ptr() } else { std::ptr::null_mut() };
        let rc = unsafe {
            A::ffi_constrained_ei(self.handle, handles.as_ptr(), handles.len() as c_int, x.as_ptr(), m as c_int, fmin_normalized,
                                  limits.as_ptr(), cei_ptr, std::ptr::null_mut(), &mut best, std::ptr::null_mut(), std::ptr::null_mut(),
                                  std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_constrained_ei failed: {}", last_error());
        }
        (cei, usize::try_from(best).ok())
    }

    /// Bounded L-BFGS ascents of `constrained_ei_normalized` from every row of `starts` inside [lo, hi], all runs in lockstep
    /// (`hbegp_maximize_constrained_ei_*`).  Returns (x [S, d] row-major, cei [S], evaluations [S]): each run's best evaluated point,
    /// never worse than its start.  Opt-in.
    #[allow(clippy::too_many_arguments)]
    pub fn maximize_constrained_ei(&self, constraints: &[&Self], starts: ArrayView2<A>, lo: &[f64], hi: &[f64], fmin_normalized: f64,
                                   limits: &[f64], maxeval: usize) -> (Vec<A>, Vec<f64>, Vec<c_int>) {
        assert_eq!(constraints.len(), limits.len(), "one limit per constraint");
        let (s, d) = starts.dim();
        assert!(lo.len() == d && hi.len() == d, "one bound pair per feature");
        let starts = starts.as_standard_layout();
        let handles: Vec<*mut HbegpModel> = constraints.iter().map(|c| c.handle).collect();
        let mut x_out = vec![A::zero(); s * d];
        let mut cei = vec![0.0f64; s];
        let mut nevals = vec![0 as c_int; s];
        let rc = unsafe {
            A::ffi_maximize_constrained_ei(self.handle, handles.as_ptr(), handles.len() as c_int, starts.as_ptr(), s as c_int, lo.as_ptr(),
                                           hi.as_ptr(), fmin_normalized, limits.as_ptr(), maxeval as c_int, x_out.as_mut_ptr(),
                                           cei.as_mut_ptr(), nevals.as_mut_ptr())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_maximize_constrained_ei failed: {}", last_error());
        }
        (x_out, cei, nevals)
    }

    /// `constrained_ei_normalized` in log space (`hbegp_log_constrained_ei_*`; log EI, Ament et al. 2023): lcei = log EI + sum_k log
    /// P[constraint k holds] from stable forms, finite -- with a usable ranking and gradient -- where `constrained_ei_normalized`
    /// underflows to exactly 0 (every |z| beyond 38); -inf only for a sigma = 0 on the wrong side of its threshold.  Arguments as
    /// `constrained_ei_normalized`; without constraints it is log EI.  Returns (lcei [m], best = the last index of its maximum,
    /// None without rows).  Opt-in.
    pub fn log_constrained_ei_normalized(&self, constraints: &[&Self], x: ArrayView2<A>, fmin_normalized: f64, limits: &[f64])
        -> (Vec<f64>, Option<usize>) {
        assert_eq!(constraints.len(), limits.len(), "one limit per constraint");
        let (m, _d) = x.dim();
        let x = x.as_standard_layout();
        let handles: Vec<*mut HbegpModel> = constraints.iter().map(|c| c.handle).collect();
        let mut lcei = vec![0.0f64; m];
        let mut best: c_int = -1;
        let lcei_ptr = if m > 0 { lcei.as_mut_ptr() } else { std::ptr::null_mut() };
        let rc = unsafe {
            A::ffi_log_constrained_ei(self.handle, handles.as_ptr(), handles.len() as c_int, x.as_ptr(), m as c_int, fmin_normalized,
                                      limits.as_ptr(), lcei_ptr, std::ptr::null_mut(), &mut best, std::ptr::null_mut(),
                                      std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_log_constrained_ei failed: {}", last_error());
        }
        (lcei, usize::try_from(best).ok())
    }

    /// `maximize_constrained_ei` on `log_constrained_ei_normalized` (`hbegp_maximize_log_constrained_ei_*`): the runs move where
    /// every start has a constrained EI of exactly 0.  Returns (x [S, d] row-major, lcei [S], evaluations [S]); a row at -inf is a
    /// failed evaluation.  Opt-in.
    #[allow(clippy::too_many_arguments)]
    pub fn maximize_log_constrained_ei(&self, constraints: &[&Self], starts: ArrayView2<A>, lo: &[f64], hi: &[f64], fmin_normalized: f64,
                                       limits: &[f64], maxeval: usize) -> (Vec<A>, Vec<f64>, Vec<c_int>) {
        assert_eq!(constraints.len(), limits.len(), "one limit per constraint");
        let (s, d) = starts.dim();
        assert!(lo.len() == d && hi.len() == d, "one bound pair per feature");
        let starts = starts.as_standard_layout();
        let handles: Vec<*mut HbegpModel> = constraints.iter().map(|c| c.handle).collect();
        let mut x_out = vec![A::zero(); s * d];
        let mut lcei = vec![0.0f64; s];
        let mut nevals = vec![0 as c_int; s];
        let rc = unsafe {
            A::ffi_maximize_log_constrained_ei(self.handle, handles.as_ptr(), handles.len() as c_int, starts.as_ptr(), s as c_int,
                                               lo.as_ptr(), hi.as_ptr(), fmin_normalized, limits.as_ptr(), maxeval as c_int,
                                               x_out.as_mut_ptr(), lcei.as_mut_ptr(), nevals.as_mut_ptr())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_maximize_log_constrained_ei failed: {}", last_error());
        }
        (x_out, lcei, nevals)
    }

    /// Max-value entropy search (`hbegp_mes_*`; Wang & Jegelka 2017) at the rows of `x`, in the normalised y space of a minimised
    /// function: the information an observation is expected to give about the VALUE of the global minimum, from the sampled minimum
    /// values `ystar` [S] (`PosteriorPaths::minimize`'s f_best, or the row minima of `sample_posterior` over a grid; S <= 1024).
    /// Stable where a candidate's mean lies far below a sample in units of sigma.  Returns (mes [m] >= 0, best = the last index of
    /// its maximum, None without rows).  Opt-in.
    pub fn mes_normalized(&self, x: ArrayView2<A>, ystar: &[f64]) -> (Vec<f64>, Option<usize>) {
        let (m, _d) = x.dim();
        let x = x.as_standard_layout();
        let mut mes = vec![0.0f64; m];
        let mut best: c_int = -1;
        let mes_ptr = if m > 0 { mes.as_mut_ptr() } else { std::ptr::null_mut() };
        let rc = unsafe {
            A::ffi_mes(self.handle, x.as_ptr(), m as c_int, ystar.as_ptr(), ystar.len() as c_int, mes_ptr, std::ptr::null_mut(),
                       &mut best, std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_mes failed: {}", last_error());
        }
        (mes, usize::try_from(best).ok())
    }

    /// Bounded L-BFGS ascents of `mes_normalized` from every row of `starts` inside [lo, hi] (`hbegp_maximize_mes_*`, all runs in
    /// lockstep on the device model).  Returns (x [R, d] row-major, mes [R], evaluations [R]): each run's best point, never worse
    /// than its start.  Opt-in.
    pub fn maximize_mes(&self, starts: ArrayView2<A>, lo: &[f64], hi: &[f64], ystar: &[f64], maxeval: usize)
        -> (Vec<A>, Vec<f64>, Vec<c_int>) {
        let (r, d) = starts.dim();
        assert!(lo.len() == d && hi.len() == d, "one bound pair per feature");
        let starts = starts.as_standard_layout();
        let mut x_out = vec![A::zero(); r * d];
        let mut mes = vec![0.0f64; r];
        let mut nevals = vec![0 as c_int; r];
        let rc = unsafe {
            A::ffi_maximize_mes(self.handle, starts.as_ptr(), r as c_int, lo.as_ptr(), hi.as_ptr(), ystar.as_ptr(),
                                ystar.len() as c_int, maxeval as c_int, x_out.as_mut_ptr(), mes.as_mut_ptr(), nevals.as_mut_ptr())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_maximize_mes failed: {}", last_error());
        }
        (x_out, mes, nevals)
    }

    /// Bounded L-BFGS descents of the confidence bound mean + `confidence_bound` * std, in the NORMALISED y space, from every row
    /// of `starts` inside [lo, hi] (`hbegp_minimize_confidence_bound_*`, all runs in lockstep on the device model, the exact
    /// gradient from the posterior gradients).  Returns (x [S, d] row-major, bound [S] normalised, evaluations [S]): each run's
    /// best point, never worse than its start.  `project_location_from_normalized` is strictly increasing, so the point that
    /// minimises the normalised bound minimises `predict_confidence_bound`; project the returned bound with it.
    /// A maintainer may call this from `suggest_optimum` (minimize.rs:598-610) in place of the BOBYQA loop over 150 single-point
    /// `predict_confidence_bound` calls: start it at `suggestion_features` with the unit box, then snap the result through
    /// `project_from_features` / `project_into_features` once -- the reference does that inside every BOBYQA evaluation, this
    /// minimiser works in the continuous feature box.  Opt-in: nothing calls it by default.
    pub fn minimize_confidence_bound(&self, starts: ArrayView2<A>, lo: &[f64], hi: &[f64], confidence_bound: f64, maxeval: usize)
        -> (Vec<A>, Vec<f64>, Vec<c_int>) {
        let (s, d) = starts.dim();
        assert!(lo.len() == d && hi.len() == d, "one bound pair per feature");
        let starts = starts.as_standard_layout();
        let mut x_out = vec![A::zero(); s * d];
        let mut bound = vec![0.0f64; s];
        let mut nevals = vec![0 as c_int; s];
        let rc = unsafe {
            A::ffi_minimize_confidence_bound(self.handle, starts.as_ptr(), s as c_int, lo.as_ptr(), hi.as_ptr(), confidence_bound,
                                             maxeval as c_int, x_out.as_mut_ptr(), bound.as_mut_ptr(), nevals.as_mut_ptr())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_minimize_confidence_bound failed: {}", last_error());
        }
        (x_out, bound, nevals)
    }

    /// Noisy expected improvement over a candidate set (`hbegp_noisy_ei_*`; Letham, Karrer, Ottoni, Bakshy 2019): EI of every row
    /// of `candidates` averaged over the joint posterior draws of the latent function at `baseline` (normally the training rows)
    /// that the caller's normals `z` [S, mb] select, each draw with its own incumbent and its own conditioned belief about the
    /// candidate, in the normalised y space -- no fmin.  Only the baseline's covariance is factored, so candidates may repeat.
    /// Returns `Ok((nei [mc], best = the last index of its maximum as `max_by`, None without candidates))`, or `Err(info)` when the
    /// baseline's covariance does not factor (info = 1 + the first column of the failing panel; retry with a larger jitter).  Opt-in.
    pub fn noisy_ei_normalized(&self, baseline: ArrayView2<A>, candidates: ArrayView2<A>, z: ArrayView2<A>, jitter: f64)
        -> Result<(Vec<f64>, Option<usize>), c_int> {
        let (mb, d) = baseline.dim();
        let (mc, dc) = candidates.dim();
        let (s, zc) = z.dim();
        assert!(mb > 0 && zc == mb && (mc == 0 || dc == d), "z must be [S, mb] and the candidates must have the baseline's features");
        let mut x = Array2::<A>::zeros((mb + mc, d));
        x.slice_mut(ndarray::s![..mb, ..]).assign(&baseline);
        if mc > 0 {
            x.slice_mut(ndarray::s![mb.., ..]).assign(&candidates);
        }
        let z = z.as_standard_layout();
        let mut nei = vec![0.0f64; mc];
        let (mut best, mut info): (c_int, c_int) = (-1, 0);
        let nei_ptr = if mc > 0 { nei.as_mut_ptr() } else { std::ptr::null_mut() };
        let rc = unsafe {
            A::ffi_noisy_ei(self.handle, x.as_ptr(), (mb + mc) as c_int, mb as c_int, z.as_ptr(), s as c_int, jitter, nei_ptr, &mut best,
                            std::ptr::null_mut(), std::ptr::null_mut(), &mut info)
        };
        if rc == HBEGP_NOT_PD {
            return Err(info);
        }
        if rc != HBEGP_OK {
            panic!("hbegp_noisy_ei failed: {}", last_error());
        }
        Ok((nei, usize::try_from(best).ok()))
    }

    /// Monte Carlo q-EI (`hbegp_qei_*`) of `b` batches of q points, `xb` [b q, d] (batch i = rows i q .. i q + q - 1), with the
    /// caller's normals `z` [S, q] shared by the batches, in the normalised y space.  Returns (qei[b], grad[b q, d], info[b]): a
    /// batch whose Sigma did not factor has qei NaN, a zero gradient and info = 1 + the failed column.  Opt-in.
    pub fn qei_normalized(&self, xb: ArrayView2<A>, b: usize, z: ArrayView2<A>, fmin_normalized: f64, jitter: f64)
        -> (Vec<f64>, Array2<A>, Vec<c_int>) {
        let (rows, d) = xb.dim();
        let (s, q) = z.dim();
        assert!(q > 0 && rows == b * q, "xb must hold b batches of q = z.ncols() points");
        let xb = xb.as_standard_layout();
        let z = z.as_standard_layout();
        let mut qei = vec![0.0f64; b];
        let mut grad = Array2::<A>::zeros((rows, d));
        let mut info: Vec<c_int> = vec![0; b];
        let rc = unsafe {
            A::ffi_qei(self.handle, xb.as_ptr(), b as c_int, q as c_int, z.as_ptr(), s as c_int, fmin_normalized, jitter,
                       qei.as_mut_ptr(), grad.as_mut_ptr(), info.as_mut_ptr())
        };
        if rc != HBEGP_OK && rc != HBEGP_NOT_PD {
            panic!("hbegp_qei failed: {}", last_error());
        }
        (qei, grad, info)
    }

    /// `hbegp_maximize_qei_*`: `r` bounded L-BFGS ascents of q-EI over whole batches from `starts` [r q, d] inside [lo, hi], with the
    /// same normals `z` [S, q] every round.  Returns (x[r q, d], qei[r], nevals[r]): each run's best batch.  Opt-in.
    pub fn maximize_qei_normalized(&self, starts: ArrayView2<A>, r: usize, lo: &[f64], hi: &[f64], z: ArrayView2<A>,
                                   fmin_normalized: f64, jitter: f64, maxeval: usize) -> (Array2<A>, Vec<f64>, Vec<c_int>) {
        let (rows, d) = starts.dim();
        let (s, q) = z.dim();
        assert!(q > 0 && rows == r * q && lo.len() == d && hi.len() == d, "starts must hold r batches of q = z.ncols() points");
        let starts = starts.as_standard_layout();
        let z = z.as_standard_layout();
        let mut x = Array2::<A>::zeros((rows, d));
        let mut qei = vec![0.0f64; r];
        let mut nevals: Vec<c_int> = vec![0; r];
        let rc = unsafe {
            A::ffi_maximize_qei(self.handle, starts.as_ptr(), r as c_int, q as c_int, lo.as_ptr(), hi.as_ptr(), z.as_ptr(), s as c_int,
                                fmin_normalized, jitter, maxeval as c_int, x.as_mut_ptr(), qei.as_mut_ptr(), nevals.as_mut_ptr())
        };
        if rc != HBEGP_OK {
            panic!("hbegp_maximize_qei failed: {}", last_error());
        }
        (x, qei, nevals)
    }

    /// Batched `predict_confidence_bound` (gpr.rs:94-112 for every row): one device call instead of one per individual
    /// in `find_best_individual_by_confidence_bound` (minimize.rs:680-714).
    pub fn predict_confidence_bound_a(&self, x: Array2<A>, cb: A) -> Array1<A> {
        let (mnorm, vnorm) = self.predict_normalized(x.view(), true);
        let stdnorm = vnorm.expect("variance was requested").mapv(|v| v.sqrt());
        // Confidence bounds are quantiles of the distribution, thus treating them as fixed locations is correct.
        self.y_norm.project_location_from_normalized(mnorm + stdnorm * cb)
    }
}

/// `hbegp_model_get_*` per element type (kept apart from `GpuScalar` so that the hot trait stays minimal).
pub trait HostCopy: GpuScalar {
    unsafe fn ffi_model_get(model: *mut HbegpModel, alpha: *mut Self, kinv: *mut Self) -> c_int;
}
impl HostCopy for f64 {
    unsafe fn ffi_model_get(model: *mut HbegpModel, alpha: *mut f64, kinv: *mut f64) -> c_int {
        hbegp_model_get_f64(model, std::ptr::null_mut(), alpha, kinv)
    }
}
impl HostCopy for f32 {
    unsafe fn ffi_model_get(model: *mut HbegpModel, alpha: *mut f32, kinv: *mut f32) -> c_int {
        hbegp_model_get_f32(model, std::ptr::null_mut(), alpha, kinv)
    }
}

impl<A: GpuScalar> SurrogateModel<A> for SurrogateModelGpu<A> {
    /// gpr.rs:72-79
    fn length_scales(&self) -> Vec<f64> {
        self.theta[2..].iter().map(|t| t.exp()).collect()
    }

    /// gpr.rs:81-92
    fn predict_mean_a(&self, x: Array2<A>) -> Array1<A> {
        let (y, _) = self.predict_normalized(x.view(), false);
        self.y_norm.project_location_from_normalized(y)
    }

    /// gpr.rs:94-112
    fn predict_confidence_bound(&self, x: Array1<A>, cb: A) -> A {
        let ys = self.predict_confidence_bound_a(x.insert_axis(Axis(0)), cb);
        *ys.first().unwrap()
    }

    /// Summary of the predictive distribution at one point -- the behaviour of gpr.rs:114-177, written independently of its text:
    /// mean / std / cv through `YNormalize`'s projections; the quartiles are the normal quantiles of N(m, s) in normalised units
    /// (all three equal m when s vanishes), projected back as locations.  Panics where the reference panics.
    fn predict_statistics(&self, x: Array1<A>) -> SummaryStatistics<A> {
        let (m, v) = self.predict_normalized(x.view().insert_axis(Axis(0)), true);
        let v = v.expect("variance was requested");
        assert!(m.len() == 1 && v.len() == 1, "should contain one element");
        let m0: f64 = m[0].into();
        let s0: f64 = v[0].sqrt().into();
        let quantiles_norm: [f64; 3] = if abs_diff_eq!(s0, 0.0) {
            [m0; 3]
        } else {
            use statrs::distribution::InverseCDF;
            let dist = statrs::distribution::Normal::new(m0, s0).unwrap_or_else(|err| {
                panic!("could not create normal distribution with mean {} std {}: {}", m0, s0, err)
            });
            [dist.inverse_cdf(0.25), dist.inverse_cdf(0.5), dist.inverse_cdf(0.75)]
        };
        let yn = &self.y_norm;
        let mean = yn.project_mean_from_normalized(m.clone(), v.view())[0];
        let std = yn.project_std_from_normalized(m.view(), v.clone())[0];
        let cv = yn.project_cv_from_normalized(m.view(), v)[0];
        let q = yn.project_location_from_normalized(quantiles_norm.iter().map(|&q| A::from_f(q)).collect::<Array1<A>>());
        SummaryStatistics::new_mean_std_cv_quartiles(mean, std, cv, [q[0], q[1], q[2]])
    }

    /// Mean and expected improvement for a batch (behaviour of gpr.rs:179-212) -- the entry the acquisition should use, one call
    /// per generation (hbetune_rs_amd/estimator.py::acquire_by_mutation re-expresses acquisition.rs:86-116, 177-202 over it):
    /// the incumbent goes into normalised units, EI is taken there per candidate on (mean, std), the mean comes back as a location.
    fn predict_mean_ei_a(&self, x: Array2<A>, fmin: A) -> (Array1<A>, Array1<A>) {
        let (mean_n, var_n) = self.predict_normalized(x.view(), true);
        let var_n = var_n.expect("variance was requested");
        let fmin_n: f64 = self.y_norm.project_into_normalized(array![fmin])[0].into();
        let ei: Array1<A> = mean_n
            .iter()
            .zip(var_n.iter())
            .map(|(&m, &v)| A::from_f(expected_improvement(m.into(), v.sqrt().into(), fmin_n)))
            .collect();
        (self.y_norm.project_location_from_normalized(mean_n), ei)
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Estimator
// ------------------------------------------------------------------------------------------------------------------
/// Mirror of `EstimatorGPR` (gpr.rs:339-400) + the device context.
#[derive(Clone)]
pub struct EstimatorGpu {
    noise_bounds: (f64, f64),
    length_scale_bounds: Vec<(f64, f64)>,
    n_restarts_optimizer: usize,
    matern_nu: f64,
    amplitude_bounds: Option<(f64, f64)>,
    y_projection: Projection,
    known_optimum: Option<f64>,
    /// evaluations per optimiser run: the reference's NLopt cap (gradmin.rs:54)
    maxeval: usize,
    ctx: std::rc::Rc<Context>,
}

impl std::fmt::Debug for EstimatorGpu {
    fn fmt(&self, f: &mut std::fmt::Formatter) -> std::fmt::Result {
        f.debug_struct("EstimatorGpu")
            .field("noise_bounds", &self.noise_bounds)
            .field("length_scale_bounds", &self.length_scale_bounds)
            .field("n_restarts_optimizer", &self.n_restarts_optimizer)
            .field("matern_nu", &self.matern_nu)
            .field("amplitude_bounds", &self.amplitude_bounds)
            .field("y_projection", &self.y_projection)
            .field("known_optimum", &self.known_optimum)
            .finish()
    }
}

/// builders: gpr.rs:351-400
impl EstimatorGpu {
    pub fn noise_bounds(self, lo: f64, hi: f64) -> Self {
        EstimatorGpu { noise_bounds: (lo, hi), ..self }
    }

    pub fn length_scale_bounds(self, bounds: Vec<(f64, f64)>) -> Self {
        EstimatorGpu { length_scale_bounds: bounds, ..self }
    }

    pub fn n_restarts_optimizer(self, n: usize) -> Self {
        EstimatorGpu { n_restarts_optimizer: n, ..self }
    }

    /// 0.5, 1.5 or 2.5 (matern_kernel.rs:65-80; other values are `unimplemented!` there and rejected by the library);
    /// `f64::INFINITY` selects the library's squared-exponential kernel (an extension: no CPU counterpart in hbetune)
    pub fn matern_nu(self, nu: f64) -> Self {
        EstimatorGpu { matern_nu: nu, ..self }
    }

    pub fn amplitude_bounds(self, bounds: Option<(f64, f64)>) -> Self {
        EstimatorGpu { amplitude_bounds: bounds, ..self }
    }

    pub fn y_projection(self, y_projection: Projection) -> Self {
        EstimatorGpu { y_projection, ..self }
    }

    pub fn known_optimum(self, known_optimum: f64) -> Self {
        EstimatorGpu { known_optimum: Some(known_optimum), ..self }
    }
}

/// gpr.rs:429-450, verbatim semantics (the function is private to gpr.rs, hence restated)
fn estimate_amplitude<A: Scalar>(y: ArrayView1<A>, bounds: Option<(f64, f64)>) -> BoundedValue<f64> {
    use ndarray_stats::Quantile1dExt as _;
    use noisy_float::types::N64;
    let (lo, hi) = bounds.unwrap_or_else(|| {
        let hi = y.mapv(|x| x.powi(2)).sum().into();
        let lo = y
            .mapv(|x| N64::from_f64(x.into()))
            .quantile_mut(N64::from_f64(0.1), &ndarray_stats::interpolate::Lower)
            .unwrap()
            .raw()
            .powi(2)
            * y.len() as f64;
        assert!(lo >= 0.0);
        let lo = if lo > 2e-5 { lo } else { 2e-5 };
        (lo / 2.0, hi * 2.0)
    });
    let start = f64::exp((lo.ln() + hi.ln()) / 2.0);
    BoundedValue::new(start, lo, hi).unwrap()
}

/// `get_kernel_or_default` (gpr.rs:402-427) in the library's terms: start point `[ln s2, ln c, ln ell..]` and
/// linear-space bounds in the same order (fit.rs:140-144).  A prior hands over its whole kernel: parameters, bounds, nu.
struct KernelSpec {
    theta0: Vec<f64>,
    lo: Vec<f64>,
    hi: Vec<f64>,
    nu: f64,
}

fn get_kernel_or_default<A: Scalar>(
    prior: Option<&SurrogateModelGpu<A>>,
    amplitude: BoundedValue<f64>,
    config: &EstimatorGpu,
) -> Result<KernelSpec, Error> {
    if let Some(prior) = prior {
        return Ok(KernelSpec {
            theta0: prior.theta.clone(),
            lo: prior.lo.clone(),
            hi: prior.hi.clone(),
            nu: prior.matern_nu,
        });
    }

    let noise = BoundedValue::new(1.0, config.noise_bounds.0, config.noise_bounds.1).map_err(Error::NoiseBounds)?;

    let length_scale: Vec<BoundedValue<f64>> = config
        .length_scale_bounds
        .iter()
        .map(|&(lo, hi)| BoundedValue::new(((lo.ln() + hi.ln()) / 2.).exp(), lo, hi))
        .collect::<Result<_, _>>()
        .map_err(Error::LengthScaleBounds)?;

    let mut theta0 = vec![noise.value().ln(), amplitude.value().ln()];
    let mut lo = vec![noise.min(), amplitude.min()];
    let mut hi = vec![noise.max(), amplitude.max()];
    for ls in &length_scale {
        theta0.push(ls.value().ln());
        lo.push(ls.min());
        hi.push(ls.max());
    }
    Ok(KernelSpec { theta0, lo, hi, nu: config.matern_nu })
}

impl<A: GpuScalar> Estimator<A> for EstimatorGpu {
    type Model = SurrogateModelGpu<A>;
    type Error = Error;

    /// gpr.rs:219-236 + the device context.  Panics without a usable GPU: `Estimator::new` cannot return an error
    /// (surrogate_model.rs:11) and there is no CPU fallback in the library -- use `EstimatorGPR` for that.
    fn new(space: &Space) -> Self {
        let ctx = match Context::open() {
            Ok(ctx) => ctx,
            Err(err) => panic!("EstimatorGpu: {}", err),
        };
        EstimatorGpu {
            noise_bounds: (1e-5, 1e5),
            length_scale_bounds: std::iter::repeat((1e-3, 1e3)).take(space.len()).collect(),
            n_restarts_optimizer: 2,
            matern_nu: 5. / 2.,
            amplitude_bounds: None,
            y_projection: Projection::Linear,
            known_optimum: None,
            maxeval: 150,
            ctx,
        }
    }

    /// gpr.rs:238-291
    fn estimate(
        &self,
        x: Array2<A>,
        y: Array1<A>,
        prior: Option<&Self::Model>,
        rng: &mut RNG,
    ) -> Result<Self::Model, Self::Error> {
        let (n_observations, n_features) = x.dim();
        assert!(
            y.len() == n_observations,
            "expected y values for {} observations: {}",
            n_observations,
            y,
        );

        let (y_train, y_norm) =
            YNormalize::new_project_into_normalized(y, self.y_projection, self.known_optimum.map(A::from_f));

        let amplitude = estimate_amplitude(y_train.view(), self.amplitude_bounds);
        let spec = get_kernel_or_default(prior, amplitude, self)?;
        let p = spec.theta0.len();
        assert!(p == n_features + 2, "kernel has {} parameters for {} features", p, n_features);

        // Start points of the restarts: the SAME draws the reference makes, in the same order -- one uniform value per
        // parameter in its log-bounds (gradmin.rs:21-24), from the forked RNG (gpr.rs:276).  They cross the ABI explicitly,
        // so the caller's random stream is preserved.
        let mut fit_rng = rng.fork_random_state();
        let mut starts: Vec<f64> = Vec::with_capacity(self.n_restarts_optimizer * p);
        for _ in 0..self.n_restarts_optimizer {
            for (lo, hi) in spec.lo.iter().zip(&spec.hi) {
                starts.push(fit_rng.uniform(lo.ln()..=hi.ln()));
            }
        }

        let x_train = x.as_standard_layout();
        let y_train = y_train.as_standard_layout();
        let opt = HbegpFitOptions {
            struct_size: std::mem::size_of::<HbegpFitOptions>(),
            maxeval: self.maxeval as c_int,
            fixed_work: 0,
            lbfgs_memory: 0,
            trace_cap: 0,
            trace_theta: std::ptr::null_mut(),
            trace_lml: std::ptr::null_mut(),
            trace_grad: std::ptr::null_mut(),
            trace_run: std::ptr::null_mut(),
            trace_count: std::ptr::null_mut(),
            n_evals: std::ptr::null_mut(),
            n_not_pd: std::ptr::null_mut(),
        };
        let mut theta = vec![0.0f64; p];
        let mut lml = 0.0f64;
        let mut handle: *mut HbegpModel = std::ptr::null_mut();
        let rc = unsafe {
            A::ffi_fit(
                self.ctx.raw,
                x_train.as_ptr(),
                y_train.as_ptr(),
                n_observations as c_int,
                n_features as c_int,
                spec.nu,
                spec.theta0.as_ptr(),
                spec.lo.as_ptr(),
                spec.hi.as_ptr(),
                if starts.is_empty() { std::ptr::null() } else { starts.as_ptr() },
                self.n_restarts_optimizer as c_int,
                &opt,
                theta.as_mut_ptr(),
                &mut lml,
                &mut handle,
            )
        };
        match rc {
            HBEGP_OK => Ok(SurrogateModelGpu {
                handle,
                ctx: self.ctx.clone(),
                theta,
                lo: spec.lo,
                hi: spec.hi,
                matern_nu: spec.nu,
                y_norm,
                lml,
            }),
            // `capture.replace(None).unwrap()` panics in the reference when no evaluation succeeded (fit.rs:161)
            HBEGP_ALL_FAILED => panic!("called `Option::unwrap()` on a `None` value: every evaluation of the fit failed"),
            _ => Err(Error::Backend(last_error())),
        }
    }

    /// gpr.rs:293-337: no re-fit -- the prior's kernel (parameters, bounds, nu) on the new data.  The caller appends its
    /// validation samples to the rows the prior was built on (minimize.rs:629-644), so the engine reuses the prior's
    /// factorisation for the unchanged leading 128-row blocks (`hbegp_extend_from_*`) and falls back to the full
    /// evaluation by itself when they differ; results are the same to rounding.
    fn extend(
        &self,
        x: Array2<A>,
        y: Array1<A>,
        prior: &Self::Model,
        _rng: &mut RNG,
    ) -> Result<Self::Model, Self::Error> {
        let (n_observations, n_features) = x.dim();
        assert!(
            y.len() == n_observations,
            "expected y values for {} observations: {}",
            n_observations,
            y
        );
        assert!(
            prior.theta.len() == n_features + 2,
            "prior model has {} kernel parameters for {} features",
            prior.theta.len(),
            n_features
        );
        let (y_train, y_norm) =
            YNormalize::new_project_into_normalized(y, self.y_projection, self.known_optimum.map(A::from_f));

        let x_train = x.as_standard_layout();
        let y_train = y_train.as_standard_layout();
        let mut handle: *mut HbegpModel = std::ptr::null_mut();
        let mut incremental: c_int = 0;
        let rc = unsafe {
            A::ffi_extend_from(
                self.ctx.raw,
                prior.handle,
                x_train.as_ptr(),
                y_train.as_ptr(),
                n_observations as c_int,
                &mut handle,
                &mut incremental,
            )
        };
        let rc = if rc == HBEGP_OK || rc == HBEGP_NOT_PD {
            rc
        } else {
            // e.g. the prior lives on another device: the plain full path at the prior's parameters
            unsafe {
                A::ffi_extend(
                    self.ctx.raw,
                    x_train.as_ptr(),
                    y_train.as_ptr(),
                    n_observations as c_int,
                    n_features as c_int,
                    prior.matern_nu,
                    prior.theta.as_ptr(),
                    prior.lo.as_ptr(),
                    prior.hi.as_ptr(),
                    &mut handle,
                )
            }
        };
        match rc {
            HBEGP_OK => {
                let mut lml = 0.0f64;
                let info = unsafe {
                    hbegp_model_info(handle, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), &mut lml)
                };
                assert!(info == HBEGP_OK, "hbegp_model_info: {}", last_error());
                Ok(SurrogateModelGpu {
                    handle,
                    ctx: self.ctx.clone(),
                    theta: prior.theta.clone(),
                    lo: prior.lo.clone(),
                    hi: prior.hi.clone(),
                    matern_nu: prior.matern_nu,
                    y_norm,
                    lml,
                })
            }
            HBEGP_NOT_PD => panic!("Kernel matrix must be invertible."), // fit.rs:55
            _ => Err(Error::Backend(last_error())),
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Error: gpr.rs:453-473 + the backend
// ------------------------------------------------------------------------------------------------------------------
#[derive(Debug)]
pub enum Error {
    NoiseBounds(BoundsError<f64>),
    LengthScaleBounds(BoundsError<f64>),
    /// a HIP / library failure (text of `hbegp_last_error`)
    Backend(String),
}

impl std::fmt::Display for Error {
    fn fmt(&self, f: &mut std::fmt::Formatter) -> std::fmt::Result {
        match *self {
            Error::NoiseBounds(BoundsError { value, min, max }) => write!(
                f,
                "noise level {} violated bounds [{}, {}] during model fitting",
                value, min, max,
            ),
            Error::LengthScaleBounds(BoundsError { value, min, max }) => write!(
                f,
                "length scale {} violated bounds [{}, {}] during model fitting",
                value, min, max,
            ),
            Error::Backend(ref msg) => write!(f, "GPU backend: {}", msg),
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Tests (need an MI355X): the reference's suites are generic over the estimator, so they run unchanged on this type --
// tests/minimize_test.rs:370-397 takes `Model: hbetune::Estimator<A>`; tests/gpr_tests.rs needs `EstimatorGPR` replaced
// by `EstimatorGpu` in its `use` line.  The two below pin what is specific to this binding.
// ------------------------------------------------------------------------------------------------------------------
#[cfg(test)]
mod tests {
    use super::*;

    fn space_1d() -> Space {
        let mut space = Space::new();
        space.add_real_parameter("test", 0.0, 1.0);
        space
    }

    #[test]
    fn clone_and_drop_share_one_device_model() {
        let xs = array![0.1, 0.5, 0.5, 0.9].insert_axis(Axis(1));
        let ys = array![1.0, 1.8, 2.2, 3.0];
        let model = <EstimatorGpu as Estimator<f64>>::new(&space_1d())
            .estimate(xs, ys, None, &mut RNG::new_with_seed(123))
            .unwrap();
        let copy = model.clone();
        let a = model.predict_mean(array![0.3]);
        drop(model);
        let b = copy.predict_mean(array![0.3]); // the device copy outlives the first owner
        assert!(a == b);
        assert_abs_diff_eq!(a, 1.5, epsilon = 0.1); // gpr_tests.rs:105-110
    }

    #[test]
    fn batched_confidence_bound_matches_the_scalar_trait_method() {
        let xs = array![0.3, 0.5, 0.7].insert_axis(Axis(1));
        let ys = array![1.0, 2.0, 1.5];
        let model = <EstimatorGpu as Estimator<f64>>::new(&space_1d())
            .noise_bounds(1e-5, 1e0)
            .length_scale_bounds(vec![(0.1, 1.0)])
            .estimate(xs, ys, None, &mut RNG::new_with_seed(9372))
            .unwrap();
        let grid = Array::linspace(0.0, 1.0, 11).insert_axis(Axis(1));
        let batched = model.predict_confidence_bound_a(grid.clone(), 1.5);
        for (row, want) in grid.outer_iter().zip(batched.iter()) {
            assert_abs_diff_eq!(model.predict_confidence_bound(row.to_owned(), 1.5), *want, epsilon = 1e-12);
        }
    }
}
