// warp.hpp -- the Kumaraswamy input warp u = 1 - (1 - x^a)^b of one feature, its parameter derivatives and its inverse, in fp64
// (DESIGN.md section 34).  ONE function for the host entry points (hbegp_warp_apply / _invert, hbegp.cpp) and for warp_kernel
// (kernels.hip): what the device writes into the feature buffer is bit for bit what the host call returns.
//
// That rules out the math libraries (the host's libm and the device's differ in the last place), so exp and log are built here from
// IEEE operations only (+, -, *, /, fma, rint; contraction off):
//   em1_small(r) = e^r - 1, |r| <= 0.35    Taylor to r^15 (truncation < 1e-17 relative)
//   exp_np(t)    = e^t                     t = k ln2 + r with a two-part ln2, 2^k (1 + em1_small(r)); 0 below -745, inf above 709.78
//   expm1_np(t)  = e^t - 1, t <= 0         em1_small near 0, exp_np(t) - 1 beyond
//   log_pos(x)   = ln x, x > 0 finite      x = 2^e m, m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), 2 atanh(s) + e ln2
//   log1mexp(t)  = ln(1 - e^t), t < 0      ln(-expm1(t)) near 0; through s = -e^t / (2 - e^t) where e^t < 1/4 (1 - e^t would
//                                          round the small term away: x = 1e-3, a = 5 has x^a = 1e-15)
// Each is good to a few units in the last place; the warp and its derivatives agree with 50-digit arithmetic to 1e-13 relative
// on the grid tests/test_warp_cpu.py walks.
//
//   u         = -expm1(b L),  L = ln(1 - x^a) = log1mexp(a ln x)
//   du/dln a  = b t e^((b - 1) L + t),  t = a ln x          (= a du/da)
//   du/dln b  = -v e^v,  v = b L                            (= b du/db)
//   du/dx     = a b e^((a - 1) ln x + (b - 1) L)
//   inverse   x = e^(M / a),  M = ln(1 - (1 - u)^(1/b)) = log1mexp(ln(1 - u) / b)
// At x = 0 and x = 1 the values are the limits: u = 0 / 1 exactly, both parameter derivatives 0 exactly, du/dx = +inf where the
// exponent at that end is below 1 (a at 0, b at 1), the other parameter where it is 1, 0 above.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HBEGP_WARP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HBEGP_WARP_HD inline __attribute__((always_inline))
#endif

namespace hbegp {
namespace warp {

HBEGP_WARP_HD double from_bits(uint64_t b) { return __builtin_bit_cast(double, b); }
HBEGP_WARP_HD uint64_t to_bits(double v) { return __builtin_bit_cast(uint64_t, v); }
HBEGP_WARP_HD double inf() { return from_bits(0x7ff0000000000000ull); }

HBEGP_WARP_HD double em1_small(double r) {
#pragma clang fp contract(off)
  double p = 7.6471637318198164759e-13;                // 1/15!
  p = __builtin_fma(p, r, 1.1470745597729724714e-11);  // 1/14!
  p = __builtin_fma(p, r, 1.6059043836821614599e-10);  // 1/13!
  p = __builtin_fma(p, r, 2.0876756987868098979e-09);  // 1/12!
  p = __builtin_fma(p, r, 2.5052108385441718775e-08);  // 1/11!
  p = __builtin_fma(p, r, 2.7557319223985890653e-07);  // 1/10!
  p = __builtin_fma(p, r, 2.7557319223985890653e-06);  // 1/9!
  p = __builtin_fma(p, r, 2.4801587301587301587e-05);  // 1/8!
  p = __builtin_fma(p, r, 1.9841269841269841270e-04);  // 1/7!
  p = __builtin_fma(p, r, 1.3888888888888888889e-03);  // 1/6!
  p = __builtin_fma(p, r, 8.3333333333333333333e-03);  // 1/5!
  p = __builtin_fma(p, r, 4.1666666666666666667e-02);  // 1/4!
  p = __builtin_fma(p, r, 1.6666666666666666667e-01);  // 1/3!
  p = __builtin_fma(p, r, 0.5);
  return __builtin_fma(p * r, r, r);
}

HBEGP_WARP_HD double exp_np(double t) {
#pragma clang fp contract(off)
  if (t != t) return t;
  if (t < -746.0) return 0.0;
  if (t > 709.78) return inf();
  const double k = __builtin_rint(t * 1.4426950408889634074);
  double r = __builtin_fma(-k, 6.93147180369123816490e-01, t);
  r = __builtin_fma(-k, 1.90821492927058770002e-10, r);
  const double m = 1.0 + em1_small(r);  // in [0.70, 1.42)
  // 2^k by exponent bits, in two factors: k may lie below the normal range (k >= -1077) or at its top (k <= 1024)
  const int ki = (int)k, k1 = ki / 2, k2 = ki - k1;
  return (m * from_bits((uint64_t)(1023 + k1) << 52)) * from_bits((uint64_t)(1023 + k2) << 52);
}

HBEGP_WARP_HD double expm1_np(double t) {
#pragma clang fp contract(off)
  if (t > -0.35) return em1_small(t);
  return exp_np(t) - 1.0;
}

// 2 atanh(s) = ln((1 + s) / (1 - s)), |s| <= 0.172
HBEGP_WARP_HD double atanh2(double s) {
#pragma clang fp contract(off)
  const double z = s * s;
  double q = 2.0 / 27.0;
  q = __builtin_fma(q, z, 2.0 / 25.0);
  q = __builtin_fma(q, z, 2.0 / 23.0);
  q = __builtin_fma(q, z, 2.0 / 21.0);
  q = __builtin_fma(q, z, 2.0 / 19.0);
  q = __builtin_fma(q, z, 2.0 / 17.0);
  q = __builtin_fma(q, z, 2.0 / 15.0);
  q = __builtin_fma(q, z, 2.0 / 13.0);
  q = __builtin_fma(q, z, 2.0 / 11.0);
  q = __builtin_fma(q, z, 2.0 / 9.0);
  q = __builtin_fma(q, z, 2.0 / 7.0);
  q = __builtin_fma(q, z, 2.0 / 5.0);
  q = __builtin_fma(q, z, 2.0 / 3.0);
  return __builtin_fma(s * z, q, 2.0 * s);
}

HBEGP_WARP_HD double log_pos(double x) {
#pragma clang fp contract(off)
  int e = 0;
  uint64_t b = to_bits(x);
  if ((b >> 52) == 0) {  // subnormal: scale into the normal range
    x *= 18014398509481984.0;  // 2^54
    b = to_bits(x);
    e = -54;
  }
  e += (int)(b >> 52) - 1023;
  double m = from_bits((b & 0x000fffffffffffffull) | 0x3ff0000000000000ull);  // [1, 2)
  if (m > 1.4142135623730951) {
    m *= 0.5;
    e += 1;
  }
  const double f = m - 1.0;  // exact
  const double l = atanh2(f / (2.0 + f));
  const double de = (double)e;
  return __builtin_fma(de, 6.93147180369123816490e-01, __builtin_fma(de, 1.90821492927058770002e-10, l));
}

// ln(1 - e^t), t < 0
HBEGP_WARP_HD double log1mexp(double t) {
#pragma clang fp contract(off)
  if (t > -0.6931471805599453) return log_pos(-expm1_np(t));
  const double e = exp_np(t);
  if (e < 0.25) return atanh2(-e / (2.0 - e));
  return log_pos(1.0 - e);
}

// One element.  a, b > 0 finite and 0 <= x <= 1 (the callers validate).  Any output may be null.
HBEGP_WARP_HD void apply(double a, double b, double x, double* u, double* du_dlna, double* du_dlnb, double* du_dx) {
#pragma clang fp contract(off)
  if (x <= 0.0 || x >= 1.0) {
    const bool top = x >= 1.0;
    if (u) *u = top ? 1.0 : 0.0;
    if (du_dlna) *du_dlna = 0.0;
    if (du_dlnb) *du_dlnb = 0.0;
    if (du_dx) {
      const double ex = top ? b : a, other = top ? a : b;
      *du_dx = ex < 1.0 ? inf() : (ex == 1.0 ? other : 0.0);
    }
    return;
  }
  const double lx = log_pos(x);
  const double t = a * lx;
  const double L = log1mexp(t);
  const double v = b * L;
  if (u) *u = -expm1_np(v);
  if (du_dlna) *du_dlna = b * t * exp_np((b - 1.0) * L + t);
  if (du_dlnb) *du_dlnb = -v * exp_np(v);
  if (du_dx) {
    *du_dx = a * b * exp_np((a - 1.0) * lx + (b - 1.0) * L);
  }
}

// One element of the inverse.  0 <= u <= 1.
HBEGP_WARP_HD double invert(double a, double b, double u) {
#pragma clang fp contract(off)
  if (u <= 0.0) return 0.0;
  if (u >= 1.0) return 1.0;
  // ln(1 - u): through atanh where u is small, so that the small term keeps its digits
  const double l1 = u < 0.25 ? atanh2(-u / (2.0 - u)) : log_pos(1.0 - u);
  const double q = l1 / b;
  if (!(q < 0.0)) return 0.0;  // u below the resolution of ln(1 - u) / b
  const double M = log1mexp(q);
  return exp_np(M / a);
}

}  // namespace warp
}  // namespace hbegp
