// C++ smoke of the EHVI over boxes through include/hbegp.hpp and the C ABI: three models on the same rows, hbegp::ehvi_nd against
// hbegp_ehvi_nd_f64 bit for bit, P = 0 against the product of the three one-dimensional expectations, two objectives against
// hbegp::ehvi, the host-only box count, and a refused call.  Built and run by tests/test_gpu_ehvi_nd.py on the GPU box.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hbegp.hpp"

static double g_of(double t, double mu, double sd) {  // E[(t - Y)^+], Y ~ N(mu, sd^2), sd > 0
  const double z = (t - mu) / sd;
  return sd * (z * 0.5 * std::erfc(-z / std::sqrt(2.0)) + std::exp(-0.5 * z * z) / std::sqrt(2.0 * M_PI));
}

int main() {
  using hbegp::FittedKernel;
  hbegp::Context ctx(1);
  const int n = 60, d = 2, m = 20;
  std::vector<double> X(n * d), Y0(n), Y1(n), Y2(n), Q(m * d);
  unsigned s = 4711;
  auto next = [&s]() { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
  for (auto& v : X) v = next();
  for (auto& v : Q) v = next();
  for (int i = 0; i < n; ++i) {
    Y0[i] = std::sin(3 * X[2 * i]) + X[2 * i + 1];
    Y1[i] = std::cos(2 * X[2 * i]) - 0.5 * X[2 * i + 1];
    Y2[i] = X[2 * i] * X[2 * i + 1] - std::sin(2 * X[2 * i + 1]);
  }
  const std::vector<double> th = {std::log(1e-2), 0.0, std::log(0.5), std::log(0.7)};
  auto f0 = FittedKernel<double>::extend(ctx, X.data(), Y0.data(), n, d, 2.5, th);
  auto f1 = FittedKernel<double>::extend(ctx, X.data(), Y1.data(), n, d, 1.5, th);
  auto f2 = FittedKernel<double>::extend(ctx, X.data(), Y2.data(), n, d, 0.5, th);
  const double front[12] = {0.2, 0.9, 0.3, 0.6, 0.4, 0.1, 1.0, 0.1, 0.5, 0.7, 0.8, -0.2}, ref[3] = {1.5, 1.2, 0.9};
  const FittedKernel<double>* objs[3] = {&f0, &f1, &f2};
  int bad = 0;
  std::vector<double> v(m), g(m * d), mean(3 * m), var(3 * m), v2(m), v0(m), w(m), w2(m);
  int best = -2, best2 = -2;
  hbegp::ehvi_nd(objs, 3, Q.data(), m, front, 4, ref, v.data(), g.data(), &best, mean.data(), var.data());
  hbegp_model* ms[3] = {f0.handle(), f1.handle(), f2.handle()};
  if (hbegp_ehvi_nd_f64(ms, 3, Q.data(), m, front, 4, ref, v2.data(), nullptr, &best2, nullptr, nullptr) != HBEGP_OK) ++bad;
  if (std::memcmp(v.data(), v2.data(), sizeof(double) * m) != 0 || best != best2 || best < 0 || best >= m) ++bad;
  for (int i = 0; i < m; ++i)
    if (!(v[i] >= 0.0) || v[i] > v[best] || (i > best && v[i] == v[best])) ++bad;  // best: the last index of the maximum
  hbegp::ehvi_nd(objs, 3, Q.data(), m, nullptr, 0, ref, v0.data(), static_cast<double*>(nullptr), nullptr, mean.data(), var.data());
  for (int i = 0; i < m; ++i) {
    double want = 1.0;
    for (int k = 0; k < 3; ++k) {
      if (!(var[3 * i + k] > 0)) ++bad;
      want *= g_of(ref[k], mean[3 * i + k], std::sqrt(var[3 * i + k]));
    }
    if (std::fabs(v0[i] - want) > 1e-12 * (1.0 + want)) ++bad;
    if (v[i] > v0[i] + 1e-12) ++bad;  // a front never adds improvement
  }
  // two objectives: the strips' sum and the boxes' sum of the same quantity
  const double front2[8] = {0.2, 0.9, 0.6, 0.4, 1.0, 0.1, 0.7, 0.8};
  hbegp::ehvi(f0, f1, Q.data(), m, front2, 4, ref, w.data());
  hbegp::ehvi_nd(objs, 2, Q.data(), m, front2, 4, ref, w2.data());
  for (int i = 0; i < m; ++i)
    if (std::fabs(w[i] - w2[i]) > 1e-12 * (1.0 + w[i])) ++bad;
  // the host-only decomposition: one point inside the box of three objectives leaves three boxes
  int counts[3] = {0, 0, 0}, n_boxes = 0;
  if (hbegp_debug_ehvi_boxes(front, 1, 3, ref, counts, nullptr, 0, &n_boxes, nullptr, 0) != HBEGP_OK || n_boxes != 3 || counts[0] != 3) ++bad;
  bool threw = false;
  const FittedKernel<double>* twice[3] = {&f0, &f1, &f0};
  try {
    hbegp::ehvi_nd(twice, 3, Q.data(), m, front, 4, ref, v.data());
  } catch (const hbegp::Error&) {
    threw = true;
  }
  std::printf("ehvi_nd[best=%d]=%.6e p0=%.6e bad=%d threw=%d\n", best, v[best], v0[best], bad, (int)threw);
  return (bad == 0 && threw) ? 0 : 1;
}
