// C++ smoke of the log-space constrained expected improvement through include/hbegp.hpp and the C ABI: an objective and two
// constraints on the same rows, hbegp::log_constrained_ei against hbegp_log_constrained_ei_f64 bit for bit, lcei = lei + lpof in the
// stated order, agreement with std::log of the closed forms on the returned posteriors where they are normal, fmin = +infinity,
// the maximiser's reproduction, and a refused call.  Built and run by tests/test_gpu_lcei.py on the GPU box.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hbegp.hpp"

static double cdf(double z) { return 0.5 * std::erfc(-z / std::sqrt(2.0)); }
static double g_of(double t, double mu, double sd) {  // E[(t - Y)^+], Y ~ N(mu, sd^2), sd > 0
  const double z = (t - mu) / sd;
  return sd * (z * cdf(z) + std::exp(-0.5 * z * z) / std::sqrt(2.0 * M_PI));
}

int main() {
  using hbegp::FittedKernel;
  hbegp::Context ctx(1);
  const int n = 60, d = 2, m = 20, K = 3;
  std::vector<double> X(n * d), Y0(n), Y1(n), Y2(n), Q(m * d);
  unsigned s = 4711;
  auto next = [&s]() { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
  for (auto& v : X) v = next();
  for (auto& v : Q) v = next();
  for (int i = 0; i < n; ++i) {
    Y0[i] = std::sin(3 * X[2 * i]) + X[2 * i + 1];
    Y1[i] = std::cos(2 * X[2 * i]) - 0.5 * X[2 * i + 1];
    Y2[i] = X[2 * i] * X[2 * i + 1];
  }
  const std::vector<double> th = {std::log(1e-2), 0.0, std::log(0.5), std::log(0.7)};
  auto f0 = FittedKernel<double>::extend(ctx, X.data(), Y0.data(), n, d, 2.5, th);
  auto f1 = FittedKernel<double>::extend(ctx, X.data(), Y1.data(), n, d, 1.5, th);
  auto f2 = FittedKernel<double>::extend(ctx, X.data(), Y2.data(), n, d, 0.5, th);
  const std::vector<const FittedKernel<double>*> cons = {&f1, &f2};
  const double fmin = 0.6, limits[2] = {0.4, 0.25}, inf = std::numeric_limits<double>::infinity();
  int bad = 0;
  std::vector<double> v(m), g(m * d), lei(m), lpof(m), mean(K * m), var(K * m), v2(m), vi(m), pi(m), li(m);
  int best = -2, best2 = -2;
  hbegp::log_constrained_ei(f0, cons, Q.data(), m, fmin, limits, v.data(), g.data(), &best, lei.data(), lpof.data(), mean.data(), var.data());
  hbegp_model* cs[2] = {f1.handle(), f2.handle()};
  if (hbegp_log_constrained_ei_f64(f0.handle(), cs, 2, Q.data(), m, fmin, limits, v2.data(), nullptr, &best2, nullptr, nullptr, nullptr,
                                   nullptr) != HBEGP_OK)
    ++bad;
  if (std::memcmp(v.data(), v2.data(), sizeof(double) * m) != 0 || best != best2 || best < 0 || best >= m) ++bad;
  for (int i = 0; i < m; ++i) {
    if (!std::isfinite(v[i]) || v[i] > v[best] || (i > best && v[i] == v[best])) ++bad;  // best: the last index of the maximum
    const double* mu = &mean[K * i];
    const double* vr = &var[K * i];
    if (!(vr[0] > 0 && vr[1] > 0 && vr[2] > 0)) ++bad;
    const double ei = g_of(fmin, mu[0], std::sqrt(vr[0]));
    const double F1 = cdf((limits[0] - mu[1]) / std::sqrt(vr[1])), F2 = cdf((limits[1] - mu[2]) / std::sqrt(vr[2]));
    // where the closed forms are normal their logarithms are good to 1e-9 (the plain EI cancels up to z^2 below z = 0)
    if (ei > 1e-100 && std::fabs(lei[i] - std::log(ei)) > 1e-9 * (1.0 + std::fabs(lei[i]))) ++bad;
    if (F1 > 1e-100 && F2 > 1e-100 && std::fabs(lpof[i] - (std::log(F1) + std::log(F2))) > 1e-9 * (1.0 + std::fabs(lpof[i]))) ++bad;
    if (v[i] != lei[i] + lpof[i]) ++bad;
    for (int k = 0; k < d; ++k)
      if (!std::isfinite(g[i * d + k])) ++bad;
  }
  // no feasible incumbent: the log probability of feasibility
  hbegp::log_constrained_ei(f0, cons, Q.data(), m, inf, limits, vi.data(), static_cast<double*>(nullptr), nullptr, li.data(), pi.data());
  if (std::memcmp(vi.data(), pi.data(), sizeof(double) * m) != 0 || std::memcmp(pi.data(), lpof.data(), sizeof(double) * m) != 0) ++bad;
  for (int i = 0; i < m; ++i)
    if (li[i] != 0.0) ++bad;
  // the maximiser from the best candidate: never worse, and reproduced bit for bit
  const double lo[2] = {0.0, 0.0}, hi[2] = {1.0, 1.0};
  double x[2], vm = -1.0, again = -2.0;
  int ne = 0;
  hbegp::maximize_log_constrained_ei(f0, cons, &Q[best * d], 1, lo, hi, fmin, limits, 40, x, &vm, &ne);
  hbegp::log_constrained_ei(f0, cons, x, 1, fmin, limits, &again);
  if (!(vm >= v[best]) || again != vm || ne < 1 || ne > 40) ++bad;
  bool threw = false;
  try {
    const std::vector<const FittedKernel<double>*> twice = {&f1, &f0};
    hbegp::log_constrained_ei(f0, twice, Q.data(), m, fmin, limits, v.data());
  } catch (const hbegp::Error&) {
    threw = true;
  }
  std::printf("lcei[best=%d]=%.6e maximised=%.6e bad=%d threw=%d\n", best, v[best], vm, bad, (int)threw);
  return (bad == 0 && threw) ? 0 : 1;
}
