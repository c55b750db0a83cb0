// hbegp.hpp — header-only C++ mirror of the reference's src/gpr interface over the C ABI (include/hbegp.h).
//
// Names follow the reference: FittedKernel::new_ / ::extend (src/gpr/fit.rs:18-68; `new` is a C++ keyword),
// FittedKernel::predict (src/gpr/predict.rs:7-52), fields kernel parameters / noise / alpha / k_inv / lml (fit.rs:6-12).
// Errors: usage and runtime errors throw hbegp::Error; the two numerical failures the reference panics on
// (extend on a non-positive-definite matrix fit.rs:55, a fit where every evaluation failed fit.rs:161) throw
// hbegp::NotPositiveDefinite.  Copying a FittedKernel shares the device model (ref-counted, like `Clone` in gpr.rs:53).
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "hbegp.h"

namespace hbegp {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& msg) : std::runtime_error("hbegp error " + std::to_string(c) + ": " + msg), code(c) {}
};
struct NotPositiveDefinite : Error {
  using Error::Error;
};
inline void check(int code) {
  if (code == HBEGP_OK) return;
  if (code == HBEGP_NOT_PD || code == HBEGP_ALL_FAILED) throw NotPositiveDefinite(code, hbegp_last_error());
  throw Error(code, hbegp_last_error());
}

class Context {
 public:
  explicit Context(int n_devices = 1, const int* ids = nullptr) { check(hbegp_ctx_create(n_devices, ids, &h_)); }
  ~Context() { if (h_) hbegp_ctx_destroy(h_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  hbegp_ctx* get() const { return h_; }

 private:
  hbegp_ctx* h_ = nullptr;
};

namespace detail {
template <typename A> struct Abi;
template <> struct Abi<double> {
  static int fit(hbegp_ctx* c, const double* x, const double* y, int n, int d, double nu, const double* t0, const double* lo,
                 const double* hi, const double* st, int r, const hbegp_fit_options* o, double* tb, double* lb, hbegp_model** m) {
    return hbegp_fit_f64(c, x, y, n, d, nu, t0, lo, hi, st, r, o, tb, lb, m);
  }
  static int extend(hbegp_ctx* c, const double* x, const double* y, int n, int d, double nu, const double* t, const double* lo,
                    const double* hi, hbegp_model** m) { return hbegp_extend_f64(c, x, y, n, d, nu, t, lo, hi, m); }
  static int extend_from(hbegp_ctx* c, hbegp_model* p, const double* x, const double* y, int n, hbegp_model** m, int* inc) { return hbegp_extend_from_f64(c, p, x, y, n, m, inc); }
  // the same with known per-row noise variances rv[n] behind y (hbegp.h: row variances)
  static int fit_rv(hbegp_ctx* c, const double* x, const double* y, const double* rv, int n, int d, double nu, const double* t0, const double* lo,
                    const double* hi, const double* st, int r, const hbegp_fit_options* o, double* tb, double* lb, hbegp_model** m) {
    return hbegp_fit_rv_f64(c, x, y, rv, n, d, nu, t0, lo, hi, st, r, o, tb, lb, m);
  }
  static int extend_rv(hbegp_ctx* c, const double* x, const double* y, const double* rv, int n, int d, double nu, const double* t, const double* lo,
                       const double* hi, hbegp_model** m) { return hbegp_extend_rv_f64(c, x, y, rv, n, d, nu, t, lo, hi, m); }
  static int extend_from_rv(hbegp_ctx* c, hbegp_model* p, const double* x, const double* y, const double* rv, int n, hbegp_model** m, int* inc) { return hbegp_extend_from_rv_f64(c, p, x, y, rv, n, m, inc); }
  // the warped fit (hbegp.h: input warping); rv, ab0, ab_lo, ab_hi may be nullptr
  static int fit_warped(hbegp_ctx* c, const double* x, const double* y, const double* rv, int n, int d, double nu, const double* t0,
                        const double* lo, const double* hi, const double* ab0, const double* alo, const double* ahi, const double* st, int r,
                        const hbegp_fit_options* o, double* tb, double* ab, double* lb, hbegp_model** m) {
    return hbegp_fit_warped_f64(c, x, y, rv, n, d, nu, t0, lo, hi, ab0, alo, ahi, st, r, o, tb, ab, lb, m);
  }
  static int predict(hbegp_model* m, const double* xs, int k, double* mean, double* var, int* w) { return hbegp_predict_f64(m, xs, k, mean, var, w); }
  static int predict_grad(hbegp_model* m, const double* xs, int k, double* mean, double* var, double* dm, double* dv, int* w) {
    return hbegp_predict_grad_f64(m, xs, k, mean, var, dm, dv, w);
  }
  static int maximize_ei(hbegp_model* m, const double* st, int s, const double* lo, const double* hi, double fmin, int maxeval, double* x,
                         double* ei, int* ne) { return hbegp_maximize_ei_f64(m, st, s, lo, hi, fmin, maxeval, x, ei, ne); }
  static int predict_cov(hbegp_model* m, const double* xs, int k, double j, double* mean, double* cov) { return hbegp_predict_cov_f64(m, xs, k, j, mean, cov); }
  static int sample_posterior(hbegp_model* m, const double* xs, int k, const double* z, int s, double j, double* smp, int* amin, int* info) {
    return hbegp_sample_posterior_f64(m, xs, k, z, s, j, smp, amin, info);
  }
  static int select_batch(hbegp_model* m, const double* xs, int n, int k, double fmin, const double* lie, int* idx, double* ei, double* mean,
                          double* var) { return hbegp_select_batch_f64(m, xs, n, k, fmin, lie, idx, ei, mean, var); }
  static int knowledge_gradient(hbegp_model* m, const double* xs, int n, int mc, double* kg, int* best, int* imin, double* mean, double* var) {
    return hbegp_knowledge_gradient_f64(m, xs, n, mc, kg, best, imin, mean, var);
  }
  static int noisy_ei(hbegp_model* m, const double* xs, int n, int mb, const double* z, int s, double j, double* nei, int* best, double* fmin,
                      double* rho, int* info) { return hbegp_noisy_ei_f64(m, xs, n, mb, z, s, j, nei, best, fmin, rho, info); }
  static int sobol(hbegp_model* m, const double* a, const double* b, int n, double* first, double* total, double* f0, double* var, double* fa, double* fb,
                   double* fab) { return hbegp_sobol_f64(m, a, b, n, first, total, f0, var, fa, fb, fab); }
  static int main_effects(hbegp_model* m, const double* a, int n, const double* grid, int g, double* effect, double* fa) {
    return hbegp_main_effects_f64(m, a, n, grid, g, effect, fa);
  }
  static int qei(hbegp_model* m, const double* xb, int b, int q, const double* z, int s, double fmin, double j, double* v, double* g, int* info) {
    return hbegp_qei_f64(m, xb, b, q, z, s, fmin, j, v, g, info);
  }
  static int maximize_qei(hbegp_model* m, const double* st, int r, int q, const double* lo, const double* hi, const double* z, int s, double fmin,
                          double j, int maxeval, double* x, double* v, int* ne) {
    return hbegp_maximize_qei_f64(m, st, r, q, lo, hi, z, s, fmin, j, maxeval, x, v, ne);
  }
  static int paths_create(hbegp_model* m, const double* om, const double* ph, const double* w, const double* eps, int F, int S, hbegp_paths** p) {
    return hbegp_paths_create_f64(m, om, ph, w, eps, F, S, p);
  }
  static int paths_eval(hbegp_paths* p, const double* xs, int m, int per_path, double* f, double* df) {
    return hbegp_paths_eval_f64(p, xs, m, per_path, f, df);
  }
  static int paths_minimize(hbegp_paths* p, const double* st, int R, const double* lo, const double* hi, int maxeval, double* x, double* f, int* ne) {
    return hbegp_paths_minimize_f64(p, st, R, lo, hi, maxeval, x, f, ne);
  }
  static int ehvi(hbegp_model* const* ms, int no, const double* xs, int m, const double* front, int P, const double* ref, double* v, double* g, int* best,
                  double* mean, double* var) { return hbegp_ehvi_f64(ms, no, xs, m, front, P, ref, v, g, best, mean, var); }
  static int maximize_ehvi(hbegp_model* const* ms, int no, const double* st, int s, const double* lo, const double* hi, const double* front, int P,
                           const double* ref, int maxeval, double* x, double* v, int* ne) {
    return hbegp_maximize_ehvi_f64(ms, no, st, s, lo, hi, front, P, ref, maxeval, x, v, ne);
  }
  static int ehvi_nd(hbegp_model* const* ms, int no, const double* xs, int m, const double* front, int P, const double* ref, double* v, double* g,
                     int* best, double* mean, double* var) { return hbegp_ehvi_nd_f64(ms, no, xs, m, front, P, ref, v, g, best, mean, var); }
  static int maximize_ehvi_nd(hbegp_model* const* ms, int no, const double* st, int s, const double* lo, const double* hi, const double* front,
                              int P, const double* ref, int maxeval, double* x, double* v, int* ne) {
    return hbegp_maximize_ehvi_nd_f64(ms, no, st, s, lo, hi, front, P, ref, maxeval, x, v, ne);
  }
  static int constrained_ei(hbegp_model* o, hbegp_model* const* cs, int nc, const double* xs, int m, double fmin, const double* lim, double* v, double* g,
                            int* best, double* ei, double* pof, double* mean, double* var) {
    return hbegp_constrained_ei_f64(o, cs, nc, xs, m, fmin, lim, v, g, best, ei, pof, mean, var);
  }
  static int maximize_constrained_ei(hbegp_model* o, hbegp_model* const* cs, int nc, const double* st, int s, const double* lo, const double* hi,
                                     double fmin, const double* lim, int maxeval, double* x, double* v, int* ne) {
    return hbegp_maximize_constrained_ei_f64(o, cs, nc, st, s, lo, hi, fmin, lim, maxeval, x, v, ne);
  }
  static int log_constrained_ei(hbegp_model* o, hbegp_model* const* cs, int nc, const double* xs, int m, double fmin, const double* lim, double* v,
                                double* g, int* best, double* lei, double* lpof, double* mean, double* var) {
    return hbegp_log_constrained_ei_f64(o, cs, nc, xs, m, fmin, lim, v, g, best, lei, lpof, mean, var);
  }
  static int maximize_log_constrained_ei(hbegp_model* o, hbegp_model* const* cs, int nc, const double* st, int s, const double* lo, const double* hi,
                                         double fmin, const double* lim, int maxeval, double* x, double* v, int* ne) {
    return hbegp_maximize_log_constrained_ei_f64(o, cs, nc, st, s, lo, hi, fmin, lim, maxeval, x, v, ne);
  }
  static int mes(hbegp_model* m, const double* xs, int cnt, const double* ys, int s, double* v, double* g, int* best, double* mean, double* var) {
    return hbegp_mes_f64(m, xs, cnt, ys, s, v, g, best, mean, var);
  }
  static int maximize_mes(hbegp_model* m, const double* st, int r, const double* lo, const double* hi, const double* ys, int s, int maxeval,
                          double* x, double* v, int* ne) {
    return hbegp_maximize_mes_f64(m, st, r, lo, hi, ys, s, maxeval, x, v, ne);
  }
  static int confidence_bound(hbegp_model* m, const double* xs, int cnt, double kappa, double* v, double* g, int* best, double* mean, double* var) {
    return hbegp_confidence_bound_f64(m, xs, cnt, kappa, v, g, best, mean, var);
  }
  static int minimize_confidence_bound(hbegp_model* m, const double* st, int s, const double* lo, const double* hi, double kappa, int maxeval,
                                       double* x, double* v, int* ne) {
    return hbegp_minimize_confidence_bound_f64(m, st, s, lo, hi, kappa, maxeval, x, v, ne);
  }
  static int get(hbegp_model* m, double* t, double* a, double* ki) { return hbegp_model_get_f64(m, t, a, ki); }
};
template <> struct Abi<float> {
  static int fit(hbegp_ctx* c, const float* x, const float* y, int n, int d, double nu, const double* t0, const double* lo,
                 const double* hi, const double* st, int r, const hbegp_fit_options* o, double* tb, double* lb, hbegp_model** m) {
    return hbegp_fit_f32(c, x, y, n, d, nu, t0, lo, hi, st, r, o, tb, lb, m);
  }
  static int extend(hbegp_ctx* c, const float* x, const float* y, int n, int d, double nu, const double* t, const double* lo,
                    const double* hi, hbegp_model** m) { return hbegp_extend_f32(c, x, y, n, d, nu, t, lo, hi, m); }
  static int extend_from(hbegp_ctx* c, hbegp_model* p, const float* x, const float* y, int n, hbegp_model** m, int* inc) { return hbegp_extend_from_f32(c, p, x, y, n, m, inc); }
  // the same with known per-row noise variances rv[n] behind y (hbegp.h: row variances)
  static int fit_rv(hbegp_ctx* c, const float* x, const float* y, const double* rv, int n, int d, double nu, const double* t0, const double* lo,
                    const double* hi, const double* st, int r, const hbegp_fit_options* o, double* tb, double* lb, hbegp_model** m) {
    return hbegp_fit_rv_f32(c, x, y, rv, n, d, nu, t0, lo, hi, st, r, o, tb, lb, m);
  }
  static int extend_rv(hbegp_ctx* c, const float* x, const float* y, const double* rv, int n, int d, double nu, const double* t, const double* lo,
                       const double* hi, hbegp_model** m) { return hbegp_extend_rv_f32(c, x, y, rv, n, d, nu, t, lo, hi, m); }
  static int extend_from_rv(hbegp_ctx* c, hbegp_model* p, const float* x, const float* y, const double* rv, int n, hbegp_model** m, int* inc) { return hbegp_extend_from_rv_f32(c, p, x, y, rv, n, m, inc); }
  static int fit_warped(hbegp_ctx* c, const float* x, const float* y, const double* rv, int n, int d, double nu, const double* t0,
                        const double* lo, const double* hi, const double* ab0, const double* alo, const double* ahi, const double* st, int r,
                        const hbegp_fit_options* o, double* tb, double* ab, double* lb, hbegp_model** m) {
    return hbegp_fit_warped_f32(c, x, y, rv, n, d, nu, t0, lo, hi, ab0, alo, ahi, st, r, o, tb, ab, lb, m);
  }
  static int predict(hbegp_model* m, const float* xs, int k, float* mean, float* var, int* w) { return hbegp_predict_f32(m, xs, k, mean, var, w); }
  static int predict_grad(hbegp_model* m, const float* xs, int k, float* mean, float* var, float* dm, float* dv, int* w) {
    return hbegp_predict_grad_f32(m, xs, k, mean, var, dm, dv, w);
  }
  static int maximize_ei(hbegp_model* m, const float* st, int s, const double* lo, const double* hi, double fmin, int maxeval, float* x,
                         double* ei, int* ne) { return hbegp_maximize_ei_f32(m, st, s, lo, hi, fmin, maxeval, x, ei, ne); }
  static int predict_cov(hbegp_model* m, const float* xs, int k, double j, float* mean, float* cov) { return hbegp_predict_cov_f32(m, xs, k, j, mean, cov); }
  static int sample_posterior(hbegp_model* m, const float* xs, int k, const float* z, int s, double j, float* smp, int* amin, int* info) {
    return hbegp_sample_posterior_f32(m, xs, k, z, s, j, smp, amin, info);
  }
  static int select_batch(hbegp_model* m, const float* xs, int n, int k, double fmin, const double* lie, int* idx, double* ei, float* mean,
                          float* var) { return hbegp_select_batch_f32(m, xs, n, k, fmin, lie, idx, ei, mean, var); }
  static int knowledge_gradient(hbegp_model* m, const float* xs, int n, int mc, double* kg, int* best, int* imin, float* mean, float* var) {
    return hbegp_knowledge_gradient_f32(m, xs, n, mc, kg, best, imin, mean, var);
  }
  static int noisy_ei(hbegp_model* m, const float* xs, int n, int mb, const float* z, int s, double j, double* nei, int* best, double* fmin,
                      double* rho, int* info) { return hbegp_noisy_ei_f32(m, xs, n, mb, z, s, j, nei, best, fmin, rho, info); }
  static int sobol(hbegp_model* m, const float* a, const float* b, int n, double* first, double* total, double* f0, double* var, float* fa, float* fb,
                   float* fab) { return hbegp_sobol_f32(m, a, b, n, first, total, f0, var, fa, fb, fab); }
  static int main_effects(hbegp_model* m, const float* a, int n, const float* grid, int g, double* effect, float* fa) {
    return hbegp_main_effects_f32(m, a, n, grid, g, effect, fa);
  }
  static int qei(hbegp_model* m, const float* xb, int b, int q, const float* z, int s, double fmin, double j, double* v, float* g, int* info) {
    return hbegp_qei_f32(m, xb, b, q, z, s, fmin, j, v, g, info);
  }
  static int maximize_qei(hbegp_model* m, const float* st, int r, int q, const double* lo, const double* hi, const float* z, int s, double fmin,
                          double j, int maxeval, float* x, double* v, int* ne) {
    return hbegp_maximize_qei_f32(m, st, r, q, lo, hi, z, s, fmin, j, maxeval, x, v, ne);
  }
  static int paths_create(hbegp_model* m, const float* om, const float* ph, const float* w, const float* eps, int F, int S, hbegp_paths** p) {
    return hbegp_paths_create_f32(m, om, ph, w, eps, F, S, p);
  }
  static int paths_eval(hbegp_paths* p, const float* xs, int m, int per_path, float* f, float* df) {
    return hbegp_paths_eval_f32(p, xs, m, per_path, f, df);
  }
  static int paths_minimize(hbegp_paths* p, const float* st, int R, const double* lo, const double* hi, int maxeval, float* x, double* f, int* ne) {
    return hbegp_paths_minimize_f32(p, st, R, lo, hi, maxeval, x, f, ne);
  }
  static int ehvi(hbegp_model* const* ms, int no, const float* xs, int m, const double* front, int P, const double* ref, double* v, float* g, int* best,
                  float* mean, float* var) { return hbegp_ehvi_f32(ms, no, xs, m, front, P, ref, v, g, best, mean, var); }
  static int maximize_ehvi(hbegp_model* const* ms, int no, const float* st, int s, const double* lo, const double* hi, const double* front, int P,
                           const double* ref, int maxeval, float* x, double* v, int* ne) {
    return hbegp_maximize_ehvi_f32(ms, no, st, s, lo, hi, front, P, ref, maxeval, x, v, ne);
  }
  static int ehvi_nd(hbegp_model* const* ms, int no, const float* xs, int m, const double* front, int P, const double* ref, double* v, float* g,
                     int* best, float* mean, float* var) { return hbegp_ehvi_nd_f32(ms, no, xs, m, front, P, ref, v, g, best, mean, var); }
  static int maximize_ehvi_nd(hbegp_model* const* ms, int no, const float* st, int s, const double* lo, const double* hi, const double* front,
                              int P, const double* ref, int maxeval, float* x, double* v, int* ne) {
    return hbegp_maximize_ehvi_nd_f32(ms, no, st, s, lo, hi, front, P, ref, maxeval, x, v, ne);
  }
  static int constrained_ei(hbegp_model* o, hbegp_model* const* cs, int nc, const float* xs, int m, double fmin, const double* lim, double* v, float* g,
                            int* best, double* ei, double* pof, float* mean, float* var) {
    return hbegp_constrained_ei_f32(o, cs, nc, xs, m, fmin, lim, v, g, best, ei, pof, mean, var);
  }
  static int maximize_constrained_ei(hbegp_model* o, hbegp_model* const* cs, int nc, const float* st, int s, const double* lo, const double* hi,
                                     double fmin, const double* lim, int maxeval, float* x, double* v, int* ne) {
    return hbegp_maximize_constrained_ei_f32(o, cs, nc, st, s, lo, hi, fmin, lim, maxeval, x, v, ne);
  }
  static int log_constrained_ei(hbegp_model* o, hbegp_model* const* cs, int nc, const float* xs, int m, double fmin, const double* lim, double* v,
                                float* g, int* best, double* lei, double* lpof, float* mean, float* var) {
    return hbegp_log_constrained_ei_f32(o, cs, nc, xs, m, fmin, lim, v, g, best, lei, lpof, mean, var);
  }
  static int maximize_log_constrained_ei(hbegp_model* o, hbegp_model* const* cs, int nc, const float* st, int s, const double* lo, const double* hi,
                                         double fmin, const double* lim, int maxeval, float* x, double* v, int* ne) {
    return hbegp_maximize_log_constrained_ei_f32(o, cs, nc, st, s, lo, hi, fmin, lim, maxeval, x, v, ne);
  }
  static int mes(hbegp_model* m, const float* xs, int cnt, const double* ys, int s, double* v, float* g, int* best, float* mean, float* var) {
    return hbegp_mes_f32(m, xs, cnt, ys, s, v, g, best, mean, var);
  }
  static int maximize_mes(hbegp_model* m, const float* st, int r, const double* lo, const double* hi, const double* ys, int s, int maxeval,
                          float* x, double* v, int* ne) {
    return hbegp_maximize_mes_f32(m, st, r, lo, hi, ys, s, maxeval, x, v, ne);
  }
  static int confidence_bound(hbegp_model* m, const float* xs, int cnt, double kappa, double* v, float* g, int* best, float* mean, float* var) {
    return hbegp_confidence_bound_f32(m, xs, cnt, kappa, v, g, best, mean, var);
  }
  static int minimize_confidence_bound(hbegp_model* m, const float* st, int s, const double* lo, const double* hi, double kappa, int maxeval,
                                       float* x, double* v, int* ne) {
    return hbegp_minimize_confidence_bound_f32(m, st, s, lo, hi, kappa, maxeval, x, v, ne);
  }
  static int get(hbegp_model* m, double* t, float* a, float* ki) { return hbegp_model_get_f32(m, t, a, ki); }
};
}  // namespace detail

// Kernel = ConstantKernel(amplitude) * Matern(nu, length_scale) + noise (gpr.rs:51); bounds in linear space.
// The Kumaraswamy input warp u_k = 1 - (1 - x_k^a_k)^b_k of features in [0, 1] (hbegp_warp_apply / _invert: host fp64, no GPU).
// ab = [a_1..a_d, b_1..b_d].  Rows are m x d, row-major.
struct Warp {
  std::vector<double> ab;
  int d() const { return (int)(ab.size() / 2); }
  static Warp identity(int d) { return Warp{std::vector<double>(2 * (size_t)d, 1.0)}; }
  std::vector<double> apply(const double* x, int m) const {
    std::vector<double> u((size_t)m * d());
    check(hbegp_warp_apply(ab.data(), d(), x, m, u.data(), nullptr, nullptr, nullptr));
    return u;
  }
  // du/dln a and du/dln b next to u (each may be nullptr)
  void apply(const double* x, int m, double* u, double* du_dlna, double* du_dlnb) const {
    check(hbegp_warp_apply(ab.data(), d(), x, m, u, du_dlna, du_dlnb, nullptr));
  }
  std::vector<double> invert(const double* u, int m) const {
    std::vector<double> x((size_t)m * d());
    check(hbegp_warp_invert(ab.data(), d(), u, m, x.data()));
    return x;
  }
  // du_k/dx_k (the map is per coordinate); +inf at an end of [0, 1] whose exponent is below 1
  std::vector<double> jacobian(const double* x, int m) const {
    std::vector<double> j((size_t)m * d());
    check(hbegp_warp_apply(ab.data(), d(), x, m, nullptr, nullptr, nullptr, j.data()));
    return j;
  }
};

struct KernelBounds {
  std::vector<double> lo, hi;  // order [noise, amplitude, ell_1..ell_d]
};

template <typename A>
class PathsT;

template <typename A>
class FittedKernel {
 public:
  FittedKernel() = default;
  FittedKernel(const FittedKernel& o) : h_(o.h_), n_(o.n_), d_(o.d_), theta_(o.theta_), lml_(o.lml_) { if (h_) hbegp_model_retain(h_); }
  FittedKernel& operator=(FittedKernel o) { swap(o); return *this; }
  FittedKernel(FittedKernel&& o) noexcept { swap(o); }
  ~FittedKernel() { if (h_) hbegp_model_release(h_); }

  // fit.rs:18-31, 71-176.  theta0: log-space start [ln s2, ln c, ln ell..]; starts: n_restarts * p log-space start points.
  // row_variance (here and in extend / extend_with; may be nullptr): n known noise variances of the rows in the normalised y scale,
  // K = c Matern + diag(s2 + v) (hbegp.h: row variances); nullptr is the plain call.
  static FittedKernel new_(const Context& ctx, const A* x, const A* y, int n, int d, double nu, const std::vector<double>& theta0,
                           const KernelBounds& b, const std::vector<double>& starts, int maxeval = 150, const double* row_variance = nullptr) {
    const int p = d + 2;
    if ((int)theta0.size() != p || (int)b.lo.size() != p || (int)b.hi.size() != p || starts.size() % p != 0)
      throw Error(HBEGP_EINVAL, "theta0 / bounds / starts have the wrong length");
    hbegp_fit_options opt = HBEGP_FIT_OPTIONS_INIT;
    opt.maxeval = maxeval;
    FittedKernel fk;
    fk.n_ = n; fk.d_ = d; fk.theta_.resize(p);
    const double* st = starts.empty() ? nullptr : starts.data();
    const int nr = (int)(starts.size() / p);
    check(row_variance ? detail::Abi<A>::fit_rv(ctx.get(), x, y, row_variance, n, d, nu, theta0.data(), b.lo.data(), b.hi.data(), st, nr, &opt,
                                                fk.theta_.data(), &fk.lml_, &fk.h_)
                       : detail::Abi<A>::fit(ctx.get(), x, y, n, d, nu, theta0.data(), b.lo.data(), b.hi.data(), st, nr, &opt, fk.theta_.data(),
                                             &fk.lml_, &fk.h_));
    return fk;
  }
  // `new_` with one input warp per feature learned jointly with theta (hbegp_fit_warped_*; features in [0, 1]).  Run 0 starts at
  // (theta0, the identity): hand in a plain fit's theta() and the result's lml is no worse than that fit's.  starts: n_restarts *
  // (p + 2 d) log-space start points [theta, ln a, ln b].  The model works in u-space: query it with warp().apply(x) rows; the
  // gradients it returns are with respect to u (multiply by warp().jacobian(x)).
  static FittedKernel new_warped(const Context& ctx, const A* x, const A* y, int n, int d, double nu, const std::vector<double>& theta0,
                                 const KernelBounds& b, const std::vector<double>& starts, int maxeval = 150,
                                 const double* row_variance = nullptr, double warp_lo = 0.2, double warp_hi = 5.0) {
    const int p = d + 2, q = p + 2 * d;
    if ((int)theta0.size() != p || (int)b.lo.size() != p || (int)b.hi.size() != p || starts.size() % q != 0)
      throw Error(HBEGP_EINVAL, "theta0 / bounds / starts have the wrong length");
    hbegp_fit_options opt = HBEGP_FIT_OPTIONS_INIT;
    opt.maxeval = maxeval;
    FittedKernel fk;
    fk.n_ = n; fk.d_ = d; fk.theta_.resize(p);
    std::vector<double> ab(2 * (size_t)d), alo(2 * (size_t)d, warp_lo), ahi(2 * (size_t)d, warp_hi);
    check(detail::Abi<A>::fit_warped(ctx.get(), x, y, row_variance, n, d, nu, theta0.data(), b.lo.data(), b.hi.data(), nullptr, alo.data(),
                                     ahi.data(), starts.empty() ? nullptr : starts.data(), (int)(starts.size() / q), &opt, fk.theta_.data(),
                                     ab.data(), &fk.lml_, &fk.h_));
    return fk;
  }
  // the input warp a model from new_warped carries (hbegp_model_warp); an empty ab for every other model
  Warp warp() const {
    Warp w;
    if (hbegp_model_warp(h_, nullptr) != 1) return w;
    w.ab.resize(2 * (size_t)d_);
    hbegp_model_warp(h_, w.ab.data());
    return w;
  }
  // fit.rs:33-68
  static FittedKernel extend(const Context& ctx, const A* x, const A* y, int n, int d, double nu, const std::vector<double>& theta,
                             const KernelBounds* b = nullptr, const double* row_variance = nullptr) {
    FittedKernel fk;
    fk.n_ = n; fk.d_ = d; fk.theta_.resize(d + 2);
    const double* lo = b ? b->lo.data() : nullptr;
    const double* hi = b ? b->hi.data() : nullptr;
    check(row_variance ? detail::Abi<A>::extend_rv(ctx.get(), x, y, row_variance, n, d, nu, theta.data(), lo, hi, &fk.h_)
                       : detail::Abi<A>::extend(ctx.get(), x, y, n, d, nu, theta.data(), lo, hi, &fk.h_));
    check(detail::Abi<A>::get(fk.h_, fk.theta_.data(), nullptr, nullptr));
    check(hbegp_model_info(fk.h_, nullptr, nullptr, nullptr, nullptr, &fk.lml_));
    return fk;
  }
  // fit.rs:33-68 at this model's theta on data whose leading rows are this model's training rows (minimize.rs:629-644):
  // reuses the factorisation of the unchanged 128-blocks; *incremental (optional) tells whether it could
  // (a model that carries row variances needs row_variance here: their prefix must equal the model's too)
  FittedKernel extend_with(const Context& ctx, const A* x, const A* y, int n, bool* incremental = nullptr,
                           const double* row_variance = nullptr) const {
    FittedKernel fk;
    fk.n_ = n; fk.d_ = d_; fk.theta_.resize(d_ + 2);
    int inc = 0;
    check(row_variance ? detail::Abi<A>::extend_from_rv(ctx.get(), h_, x, y, row_variance, n, &fk.h_, &inc)
                       : detail::Abi<A>::extend_from(ctx.get(), h_, x, y, n, &fk.h_, &inc));
    if (incremental) *incremental = inc != 0;
    check(detail::Abi<A>::get(fk.h_, fk.theta_.data(), nullptr, nullptr));
    check(hbegp_model_info(fk.h_, nullptr, nullptr, nullptr, nullptr, &fk.lml_));
    return fk;
  }
  // the model's row variances (n doubles; for an f32 model the rounded values, widened); empty for a model without them
  std::vector<double> row_variance() const {
    std::vector<double> rv;
    if (hbegp_model_row_variance(h_, nullptr) != 1) return rv;
    rv.resize((size_t)n_);
    if (hbegp_model_row_variance(h_, rv.data()) != 1) throw Error(HBEGP_EHIP, hbegp_last_error());
    return rv;
  }
  // predict.rs:7-52: mean (and variance when var != nullptr); returns the number of variances below -sqrt(1e-5)
  int predict(const A* xs, int m, A* mean, A* var) const {
    int warn = 0;
    check(detail::Abi<A>::predict(h_, xs, m, mean, var, &warn));
    return warn;
  }
  // predict plus d mean / dx* and d var / dx* (dmean[m*d], dvar[m*d] row-major; var and dvar nullptr together)
  int predict_grad(const A* xs, int m, A* mean, A* var, A* dmean, A* dvar) const {
    int warn = 0;
    check(detail::Abi<A>::predict_grad(h_, xs, m, mean, var, dmean, dvar, &warn));
    return warn;
  }
  // S bounded L-BFGS ascents of EI (normalised y space) from starts[S*d] inside [lo, hi]; x_out[S*d], ei_out[S], nevals[S] (may be nullptr)
  void maximize_ei(const A* starts, int S, const double* lo, const double* hi, double fmin_normalized, int maxeval, A* x_out,
                   double* ei_out, int* nevals = nullptr) const {
    check(detail::Abi<A>::maximize_ei(h_, starts, S, lo, hi, fmin_normalized, maxeval, x_out, ei_out, nevals));
  }
  // joint posterior at xs[m*d]: mean[m] (may be nullptr), cov[m*m] = K** + (1e-5 + jitter) I - K*^T K^-1 K* (normalised y space)
  void predict_cov(const A* xs, int m, A* mean, A* cov, double jitter = 0.0) const {
    check(detail::Abi<A>::predict_cov(h_, xs, m, jitter, mean, cov));
  }
  // S joint draws mean + L z_s from the caller's normals z[S*m]: samples[S*m] and / or argmin[S] (either may be nullptr, not both);
  // throws Error(HBEGP_NOT_PD) when cov does not factor (retry with a larger jitter)
  void sample_posterior(const A* xs, int m, const A* z, int S, A* samples, int* argmin, double jitter = 0.0) const {
    check(detail::Abi<A>::sample_posterior(h_, xs, m, z, S, jitter, samples, argmin, nullptr));
  }
  // k candidates of xs[m*d] picked greedily by EI with fantasised observations (kriging believer, or the constant liar *lie):
  // idx[k]; ei[k], mean[m], var[m] may be nullptr (normalised y space; mean / var after the k conditionings)
  void select_batch(const A* xs, int m, int k, double fmin_normalized, int* idx, double* ei = nullptr, A* mean = nullptr,
                    A* var = nullptr, const double* lie = nullptr) const {
    check(detail::Abi<A>::select_batch(h_, xs, m, k, fmin_normalized, lie, idx, ei, mean, var));
  }
  // knowledge gradient of one more noisy sample at each of the first mc rows of xs[m*d], the minimum of the posterior mean taken
  // over all m rows (normalised y space): kg[mc]; best (the last index of the maximum of kg), imin (the lowest index of the
  // minimum of the mean), mean[m], var[m] may be nullptr
  void knowledge_gradient(const A* xs, int m, int mc, double* kg, int* best = nullptr, int* imin = nullptr, A* mean = nullptr,
                          A* var = nullptr) const {
    check(detail::Abi<A>::knowledge_gradient(h_, xs, m, mc, kg, best, imin, mean, var));
  }
  // noisy expected improvement of the candidates xs[mb*d ..] given S joint draws of the latent function at the baseline, the first mb
  // rows of xs[m*d], from the caller's normals z[S*mb] (normalised y space): nei[m - mb]; best (the last index of the maximum of
  // nei), fmin_draws[S], rho[m - mb] may be nullptr.  Only the baseline block is factored: throws Error(HBEGP_NOT_PD) when it does
  // not factor (retry with a larger jitter)
  void noisy_ei(const A* xs, int m, int mb, const A* z, int S, double* nei, int* best = nullptr, double* fmin_draws = nullptr,
                double* rho = nullptr, double jitter = 0.0) const {
    check(detail::Abi<A>::noisy_ei(h_, xs, m, mb, z, S, jitter, nei, best, fmin_draws, rho, nullptr));
  }
  // Sobol indices of the posterior mean by pick-freeze sampling from the caller's sample matrices a[N*d], b[N*d]: first[d], total[d];
  // f0, variance and the values f_a[N], f_b[N], f_ab[d*N] (f_ab[k*N + i]: row i of a with column k from b) may be nullptr
  void sobol_indices(const A* a, const A* b, int N, double* first, double* total, double* f0 = nullptr, double* variance = nullptr,
                     A* f_a = nullptr, A* f_b = nullptr, A* f_ab = nullptr) const {
    check(detail::Abi<A>::sobol(h_, a, b, N, first, total, f0, variance, f_a, f_b, f_ab));
  }
  // main-effect (partial dependence) curves: effect[k*G + g] = the mean over the rows of a[N*d] of the posterior mean with feature k
  // set to grid[k*G + g] (normalised y space); f_a[N] may be nullptr.  N = 1: one row's conditional curves
  void main_effects(const A* a, int N, const A* grid, int G, double* effect, A* f_a = nullptr) const {
    check(detail::Abi<A>::main_effects(h_, a, N, grid, G, effect, f_a));
  }
  // Monte Carlo q-EI of B batches xb[B*q*d] with the caller's normals z[S*q]: qei[B]; grad[B*q*d] and info[B] may be nullptr.
  // Returns HBEGP_OK or HBEGP_NOT_PD (some batch's Sigma did not factor: its qei is NaN, info says where); throws otherwise
  int qei(const A* xb, int B, int q, const A* z, int S, double fmin_normalized, double* qei, A* grad = nullptr, int* info = nullptr,
          double jitter = 0.0) const {
    const int rc = detail::Abi<A>::qei(h_, xb, B, q, z, S, fmin_normalized, jitter, qei, grad, info);
    if (rc != HBEGP_NOT_PD) check(rc);
    return rc;
  }
  // R bounded L-BFGS ascents of q-EI over whole batches from starts[R*q*d] inside [lo, hi]; x_out[R*q*d], qei_out[R], nevals[R]
  void maximize_qei(const A* starts, int R, int q, const double* lo, const double* hi, const A* z, int S, double fmin_normalized,
                    int maxeval, A* x_out, double* qei_out, int* nevals = nullptr, double jitter = 0.0) const {
    check(detail::Abi<A>::maximize_qei(h_, starts, R, q, lo, hi, z, S, fmin_normalized, jitter, maxeval, x_out, qei_out, nevals));
  }
  // S posterior sample paths (draws that are functions) from the caller's omega0[F*d], phase[F], w[S*F], eps[S*n] or nullptr
  PathsT<A> sample_paths(const A* omega0, const A* phase, const A* w, const A* eps, int F, int S) const;
  hbegp_model* handle() const { return h_; }
  double lml() const { return lml_; }
  double noise() const { return std::exp(theta_[0]); }
  double amplitude() const { return std::exp(theta_[1]); }
  std::vector<double> length_scale() const {
    std::vector<double> e(theta_.begin() + 2, theta_.end());
    for (auto& v : e) v = std::exp(v);
    return e;
  }
  std::vector<A> alpha() const { std::vector<A> a(n_); check(detail::Abi<A>::get(h_, nullptr, a.data(), nullptr)); return a; }
  std::vector<A> k_inv() const { std::vector<A> k((size_t)n_ * n_); check(detail::Abi<A>::get(h_, nullptr, nullptr, k.data())); return k; }

 private:
  void swap(FittedKernel& o) { std::swap(h_, o.h_); std::swap(n_, o.n_); std::swap(d_, o.d_); theta_.swap(o.theta_); std::swap(lml_, o.lml_); }
  hbegp_model* h_ = nullptr;
  int n_ = 0, d_ = 0;
  std::vector<double> theta_;
  double lml_ = 0;
};

// Expected hypervolume improvement of two minimised, independent objectives at xs[m*d], each objective modelled by its own
// FittedKernel (normalised y spaces): front[P*2] the points reached so far in any order, ref[2] the reference point; ehvi[m];
// grad[m*d], best (the last index of the maximum), mean[m*2], var[m*2] (objective 0 then 1 per row) may be nullptr
template <typename A>
void ehvi(const FittedKernel<A>& obj0, const FittedKernel<A>& obj1, const A* xs, int m, const double* front, int P, const double* ref,
          double* ehvi_out, A* grad = nullptr, int* best = nullptr, A* mean = nullptr, A* var = nullptr) {
  hbegp_model* ms[2] = {obj0.handle(), obj1.handle()};
  check(detail::Abi<A>::ehvi(ms, 2, xs, m, front, P, ref, ehvi_out, grad, best, mean, var));
}
// S bounded L-BFGS ascents of that EHVI from starts[S*d] inside [lo, hi]; x_out[S*d], ehvi_out[S], nevals[S] (may be nullptr)
template <typename A>
void maximize_ehvi(const FittedKernel<A>& obj0, const FittedKernel<A>& obj1, const A* starts, int S, const double* lo, const double* hi,
                   const double* front, int P, const double* ref, int maxeval, A* x_out, double* ehvi_out, int* nevals = nullptr) {
  hbegp_model* ms[2] = {obj0.handle(), obj1.handle()};
  check(detail::Abi<A>::maximize_ehvi(ms, 2, starts, S, lo, hi, front, P, ref, maxeval, x_out, ehvi_out, nevals));
}
// The same for n_obj = 2, 3 or 4 objectives, objs[n_obj] pointing at their FittedKernels (objective 0 first): front[P*n_obj],
// ref[n_obj], mean[m*n_obj], var[m*n_obj].  A front whose free region splits into more than HBEGP_EHVI_ND_MAX_BOXES boxes throws.
template <typename A>
void ehvi_nd(const FittedKernel<A>* const* objs, int n_obj, const A* xs, int m, const double* front, int P, const double* ref,
             double* ehvi_out, A* grad = nullptr, int* best = nullptr, A* mean = nullptr, A* var = nullptr) {
  hbegp_model* ms[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < n_obj && k < 4; ++k) ms[k] = objs[k]->handle();
  check(detail::Abi<A>::ehvi_nd(ms, n_obj, xs, m, front, P, ref, ehvi_out, grad, best, mean, var));
}
template <typename A>
void maximize_ehvi_nd(const FittedKernel<A>* const* objs, int n_obj, const A* starts, int S, const double* lo, const double* hi,
                      const double* front, int P, const double* ref, int maxeval, A* x_out, double* ehvi_out, int* nevals = nullptr) {
  hbegp_model* ms[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < n_obj && k < 4; ++k) ms[k] = objs[k]->handle();
  check(detail::Abi<A>::maximize_ehvi_nd(ms, n_obj, starts, S, lo, hi, front, P, ref, maxeval, x_out, ehvi_out, nevals));
}

// Constrained expected improvement at xs[m*d]: the EI of the minimised `objective` below fmin (normalised y space; +infinity: no
// feasible point is known, EI counts as 1) times the probability that every constraints[k] stays at or below limits[k], each
// quantity modelled by its own FittedKernel, taken as independent; at most HBEGP_CEI_MAX_CONSTRAINTS constraints.  cei[m]; grad[m*d],
// best (the last index of the maximum), ei[m], pof[m], mean[m*(1+C)], var[m*(1+C)] (the objective then the constraints per row) may
// be nullptr
template <typename A>
void constrained_ei(const FittedKernel<A>& objective, const std::vector<const FittedKernel<A>*>& constraints, const A* xs, int m, double fmin,
                    const double* limits, double* cei, A* grad = nullptr, int* best = nullptr, double* ei = nullptr, double* pof = nullptr,
                    A* mean = nullptr, A* var = nullptr) {
  std::vector<hbegp_model*> cs;
  for (const auto* c : constraints) cs.push_back(c ? c->handle() : nullptr);
  check(detail::Abi<A>::constrained_ei(objective.handle(), cs.data(), (int)cs.size(), xs, m, fmin, limits, cei, grad, best, ei, pof, mean, var));
}
// S bounded L-BFGS ascents of that cEI from starts[S*d] inside [lo, hi]; x_out[S*d], cei_out[S], nevals[S] (may be nullptr)
template <typename A>
void maximize_constrained_ei(const FittedKernel<A>& objective, const std::vector<const FittedKernel<A>*>& constraints, const A* starts, int S,
                             const double* lo, const double* hi, double fmin, const double* limits, int maxeval, A* x_out, double* cei_out,
                             int* nevals = nullptr) {
  std::vector<hbegp_model*> cs;
  for (const auto* c : constraints) cs.push_back(c ? c->handle() : nullptr);
  check(detail::Abi<A>::maximize_constrained_ei(objective.handle(), cs.data(), (int)cs.size(), starts, S, lo, hi, fmin, limits, maxeval, x_out,
                                                cei_out, nevals));
}

// The logarithm of that cEI by stable forms (hbegp_log_constrained_ei_*): lcei[m] = lei + lpof with lei = log EI (0 for fmin = +infinity)
// and lpof = sum_k log P[constraint k holds]; grad[m*d] is the gradient of lcei.  Finite, with a gradient, where constrained_ei
// underflows to exactly 0; -infinity only for a sigma = 0 on the wrong side.  Without constraints it is log EI.  Arguments as
// constrained_ei
template <typename A>
void log_constrained_ei(const FittedKernel<A>& objective, const std::vector<const FittedKernel<A>*>& constraints, const A* xs, int m,
                        double fmin, const double* limits, double* lcei, A* grad = nullptr, int* best = nullptr, double* lei = nullptr,
                        double* lpof = nullptr, A* mean = nullptr, A* var = nullptr) {
  std::vector<hbegp_model*> cs;
  for (const auto* c : constraints) cs.push_back(c ? c->handle() : nullptr);
  check(detail::Abi<A>::log_constrained_ei(objective.handle(), cs.data(), (int)cs.size(), xs, m, fmin, limits, lcei, grad, best, lei, lpof, mean,
                                           var));
}
// maximize_constrained_ei on lcei: the runs move where every start has cei = 0; a row at -infinity is a failed evaluation
template <typename A>
void maximize_log_constrained_ei(const FittedKernel<A>& objective, const std::vector<const FittedKernel<A>*>& constraints, const A* starts,
                                 int S, const double* lo, const double* hi, double fmin, const double* limits, int maxeval, A* x_out,
                                 double* lcei_out, int* nevals = nullptr) {
  std::vector<hbegp_model*> cs;
  for (const auto* c : constraints) cs.push_back(c ? c->handle() : nullptr);
  check(detail::Abi<A>::maximize_log_constrained_ei(objective.handle(), cs.data(), (int)cs.size(), starts, S, lo, hi, fmin, limits, maxeval,
                                                    x_out, lcei_out, nevals));
}

// Max-value entropy search at xs[m*d] under one minimised model (hbegp_mes_*): the information an observation is expected to give
// about the value of the global minimum, from S sampled minimum values ystar[S] (normalised y space; PathsT::minimize's f_best, or
// the row minima of sample_posterior over a grid).  mes[m] >= 0; grad[m*d], best (the last index of the maximum), mean[m], var[m]
// may be nullptr
template <typename A>
void mes(const FittedKernel<A>& model, const A* xs, int m, const double* ystar, int S, double* mes_out, A* grad = nullptr,
         int* best = nullptr, A* mean = nullptr, A* var = nullptr) {
  check(detail::Abi<A>::mes(model.handle(), xs, m, ystar, S, mes_out, grad, best, mean, var));
}
// R bounded L-BFGS ascents of that MES from starts[R*d] inside [lo, hi]; x_out[R*d], mes_out[R], nevals[R] (may be nullptr)
template <typename A>
void maximize_mes(const FittedKernel<A>& model, const A* starts, int R, const double* lo, const double* hi, const double* ystar, int S,
                  int maxeval, A* x_out, double* mes_out, int* nevals = nullptr) {
  check(detail::Abi<A>::maximize_mes(model.handle(), starts, R, lo, hi, ystar, S, maxeval, x_out, mes_out, nevals));
}

// The confidence bound mu + kappa sigma at xs[m*d] under one model (hbegp_confidence_bound_*; normalised y space): kappa > 0 is the
// reference's predict_confidence_bound, kappa < 0 GP-LCB.  cb[m]; grad[m*d], best (the FIRST index of the minimum), mean[m], var[m]
// may be nullptr
template <typename A>
void confidence_bound(const FittedKernel<A>& model, const A* xs, int m, double kappa, double* cb, A* grad = nullptr, int* best = nullptr,
                      A* mean = nullptr, A* var = nullptr) {
  check(detail::Abi<A>::confidence_bound(model.handle(), xs, m, kappa, cb, grad, best, mean, var));
}
// S bounded L-BFGS descents of that bound from starts[S*d] inside [lo, hi]; x_out[S*d], cb_out[S], nevals[S] (may be nullptr)
template <typename A>
void minimize_confidence_bound(const FittedKernel<A>& model, const A* starts, int S, const double* lo, const double* hi, double kappa,
                               int maxeval, A* x_out, double* cb_out, int* nevals = nullptr) {
  check(detail::Abi<A>::minimize_confidence_bound(model.handle(), starts, S, lo, hi, kappa, maxeval, x_out, cb_out, nevals));
}

// RAII owner of an hbegp_paths handle (FittedKernel::sample_paths); it keeps its model alive
template <typename A>
class PathsT {
 public:
  PathsT() = default;
  explicit PathsT(hbegp_paths* h) : h_(h) {}
  PathsT(const PathsT&) = delete;
  PathsT& operator=(const PathsT&) = delete;
  PathsT(PathsT&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  PathsT& operator=(PathsT&& o) noexcept { std::swap(h_, o.h_); return *this; }
  ~PathsT() { hbegp_paths_release(h_); }
  // f[S*m], df[S*m*d] (may be nullptr) at xs[m*d] (per_path = false) or xs[S*m*d] (per_path = true)
  void eval(const A* xs, int m, bool per_path, A* f, A* df) const { check(detail::Abi<A>::paths_eval(h_, xs, m, per_path ? 1 : 0, f, df)); }
  // per path the best point of R bounded L-BFGS descents from starts[S*R*d]: x_best[S*d], f_best[S], nevals[S] (may be nullptr)
  void minimize(const A* starts, int R, const double* lo, const double* hi, int maxeval, A* x_best, double* f_best, int* nevals = nullptr) const {
    check(detail::Abi<A>::paths_minimize(h_, starts, R, lo, hi, maxeval, x_best, f_best, nevals));
  }
  hbegp_paths* handle() const { return h_; }

 private:
  hbegp_paths* h_ = nullptr;
};

template <typename A>
PathsT<A> FittedKernel<A>::sample_paths(const A* omega0, const A* phase, const A* w, const A* eps, int F, int S) const {
  hbegp_paths* p = nullptr;
  check(detail::Abi<A>::paths_create(h_, omega0, phase, w, eps, F, S, &p));
  return PathsT<A>(p);
}

}  // namespace hbegp
