// C++ smoke of the confidence bound through include/hbegp.hpp and the C ABI: hbegp::confidence_bound against
// hbegp_confidence_bound_f64 bit for bit, the closed form mu + kappa sqrt(var) with std::sqrt on the returned posteriors (the header
// promises single rounded fp64 operations, so the bits have to agree), the arg-min's rule, the minimiser's reproduction, and a
// refused call.  Built and run by tests/test_gpu_cb.py on the GPU box.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hbegp.hpp"

int main() {
  using hbegp::FittedKernel;
  hbegp::Context ctx(1);
  const int n = 60, d = 2, m = 20;
  std::vector<double> X(n * d), Y(n), Q(m * d);
  unsigned s = 4711;
  auto next = [&s]() { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
  for (auto& v : X) v = next();
  for (auto& v : Q) v = next();
  for (int i = 0; i < n; ++i) Y[i] = std::sin(3 * X[2 * i]) + X[2 * i + 1];
  const std::vector<double> th = {std::log(1e-2), 0.0, std::log(0.5), std::log(0.7)};
  auto fk = FittedKernel<double>::extend(ctx, X.data(), Y.data(), n, d, 2.5, th);
  int bad = 0;
  const double kappa = 1.5;
  std::vector<double> v(m), g(m * d), mean(m), var(m), v2(m), pm(m), pv(m), dm(m * d), dv(m * d);
  int best = -2, best2 = -2;
  hbegp::confidence_bound(fk, Q.data(), m, kappa, v.data(), g.data(), &best, mean.data(), var.data());
  if (hbegp_confidence_bound_f64(fk.handle(), Q.data(), m, kappa, v2.data(), nullptr, &best2, nullptr, nullptr) != HBEGP_OK) ++bad;
  if (std::memcmp(v.data(), v2.data(), sizeof(double) * m) != 0 || best != best2 || best < 0 || best >= m) ++bad;
  if (hbegp_predict_grad_f64(fk.handle(), Q.data(), m, pm.data(), pv.data(), dm.data(), dv.data(), nullptr) != HBEGP_OK) ++bad;
  if (std::memcmp(pm.data(), mean.data(), sizeof(double) * m) != 0 || std::memcmp(pv.data(), var.data(), sizeof(double) * m) != 0) ++bad;
  for (int i = 0; i < m; ++i) {
    if (!std::isfinite(v[i]) || v[i] < v[best] || (i < best && v[i] == v[best])) ++bad;  // best: the first index of the minimum
    const double sd = std::sqrt(var[i]);
    if (!(sd > 1e-3)) ++bad;  // away from the sigma = 0 branch
    volatile double ks = kappa * sd;  // volatile: two rounded operations, never a fused one
    const double want = mean[i] + ks;
    if (v[i] != want) ++bad;
    for (int k = 0; k < d; ++k) {
      volatile double q = dv[i * d + k] / (2.0 * sd);
      volatile double kq = kappa * q;
      const double gw = dm[i * d + k] + kq;
      if (g[i * d + k] != gw) ++bad;
    }
  }
  // the minimiser from the best candidate: never worse, and reproduced bit for bit
  const double lo[2] = {0.0, 0.0}, hi[2] = {1.0, 1.0};
  double x[2], vm = 1e300, again = -2.0;
  int ne = 0;
  hbegp::minimize_confidence_bound(fk, &Q[best * d], 1, lo, hi, kappa, 40, x, &vm, &ne);
  hbegp::confidence_bound(fk, x, 1, kappa, &again);
  if (!(vm <= v[best]) || again != vm || ne < 1 || ne > 40 || x[0] < 0 || x[0] > 1 || x[1] < 0 || x[1] > 1) ++bad;
  bool threw = false;
  try {
    hbegp::confidence_bound(fk, Q.data(), m, std::numeric_limits<double>::infinity(), v2.data());
  } catch (const hbegp::Error&) {
    threw = true;
  }
  if (std::memcmp(v.data(), v2.data(), sizeof(double) * m) != 0) ++bad;  // a refused call writes nothing
  std::printf("cb[best=%d]=%.6e minimised=%.6e evals=%d bad=%d threw=%d\n", best, v[best], vm, ne, bad, (int)threw);
  return (bad == 0 && threw) ? 0 : 1;
}
