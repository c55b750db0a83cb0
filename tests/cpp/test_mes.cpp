// C++ smoke of max-value entropy search through include/hbegp.hpp and the C ABI: hbegp::mes against hbegp_mes_f64 bit for bit,
// agreement with the std::log / std::erfc closed forms on the returned posteriors away from the tails (|gamma| < 5), the
// maximiser's reproduction, and a refused call.  Built and run by tests/test_gpu_mes.py on the GPU box.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hbegp.hpp"

static double cdf(double z) { return 0.5 * std::erfc(-z / std::sqrt(2.0)); }
static double pdf(double z) { return std::exp(-0.5 * z * z) / std::sqrt(2.0 * M_PI); }

int main() {
  using hbegp::FittedKernel;
  hbegp::Context ctx(1);
  const int n = 60, d = 2, m = 20, S = 5;
  std::vector<double> X(n * d), Y(n), Q(m * d);
  unsigned s = 4711;
  auto next = [&s]() { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
  for (auto& v : X) v = next();
  for (auto& v : Q) v = next();
  for (int i = 0; i < n; ++i) Y[i] = std::sin(3 * X[2 * i]) + X[2 * i + 1];
  const std::vector<double> th = {std::log(1e-2), 0.0, std::log(0.5), std::log(0.7)};
  auto fk = FittedKernel<double>::extend(ctx, X.data(), Y.data(), n, d, 2.5, th);
  int bad = 0;
  std::vector<double> v(m), g(m * d), mean(m), var(m), v2(m), ys(S);
  int best = -2, best2 = -2;
  // sampled minimum values around the posterior at the candidates: first the posteriors (one MES call with any y*), then y* a
  // fraction of a sigma below the lowest mean, so that every |gamma| stays small
  for (int k = 0; k < S; ++k) ys[k] = 0.0;
  hbegp::mes(fk, Q.data(), m, ys.data(), S, v.data(), static_cast<double*>(nullptr), nullptr, mean.data(), var.data());
  double lowest = mean[0], sd_min = std::sqrt(var[0]), sd_max = sd_min;
  for (int i = 0; i < m; ++i) {
    lowest = std::fmin(lowest, mean[i]);
    sd_min = std::fmin(sd_min, std::sqrt(var[i]));
    sd_max = std::fmax(sd_max, std::sqrt(var[i]));
  }
  if (!(sd_min > 0)) ++bad;
  for (int k = 0; k < S; ++k) ys[k] = lowest - 0.2 * (k + 1) * sd_min;
  hbegp::mes(fk, Q.data(), m, ys.data(), S, v.data(), g.data(), &best, mean.data(), var.data());
  if (hbegp_mes_f64(fk.handle(), Q.data(), m, ys.data(), S, v2.data(), nullptr, &best2, nullptr, nullptr) != HBEGP_OK) ++bad;
  if (std::memcmp(v.data(), v2.data(), sizeof(double) * m) != 0 || best != best2 || best < 0 || best >= m) ++bad;
  int checked = 0;
  for (int i = 0; i < m; ++i) {
    if (!std::isfinite(v[i]) || v[i] < 0 || v[i] > v[best] || (i > best && v[i] == v[best])) ++bad;  // best: the last index of the maximum
    const double sd = std::sqrt(var[i]);
    double sum = 0.0;
    bool tame = true;
    for (int k = 0; k < S; ++k) {
      const double gam = (mean[i] - ys[k]) / sd;
      tame = tame && std::fabs(gam) < 5.0;
      sum += gam * pdf(gam) / (2.0 * cdf(gam)) - std::log(cdf(gam));
    }
    if (tame) {
      ++checked;
      if (std::fabs(v[i] - sum / S) > 1e-10 * std::fmax(1.0, std::fabs(sum / S))) ++bad;
    }
    for (int k = 0; k < d; ++k)
      if (!std::isfinite(g[i * d + k])) ++bad;
  }
  if (checked == 0) ++bad;
  // the maximiser from the best candidate: never worse, and reproduced bit for bit
  const double lo[2] = {0.0, 0.0}, hi[2] = {1.0, 1.0};
  double x[2], vm = -1.0, again = -2.0;
  int ne = 0;
  hbegp::maximize_mes(fk, &Q[best * d], 1, lo, hi, ys.data(), S, 40, x, &vm, &ne);
  hbegp::mes(fk, x, 1, ys.data(), S, &again);
  if (!(vm >= v[best]) || again != vm || ne < 1 || ne > 40) ++bad;
  bool threw = false;
  try {
    ys[2] = std::numeric_limits<double>::infinity();
    hbegp::mes(fk, Q.data(), m, ys.data(), S, v2.data());
  } catch (const hbegp::Error&) {
    threw = true;
  }
  if (std::memcmp(v.data(), v2.data(), sizeof(double) * m) != 0) ++bad;  // a refused call writes nothing
  std::printf("mes[best=%d]=%.6e maximised=%.6e checked=%d bad=%d threw=%d\n", best, v[best], vm, checked, bad, (int)threw);
  return (bad == 0 && threw) ? 0 : 1;
}
