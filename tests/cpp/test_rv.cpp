// C++ smoke of the row variances through include/hbegp.hpp: extend / new_ / extend_with with row_variance against the C ABI's
// hbegp_extend_rv_f64 bit for bit, row_variance() round trip, nullptr = the plain call, the incremental path on a matching prefix,
// and the refusals (a negative variance; a model with variances extended without them).  Built and run by tests/test_gpu_rv.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hbegp.hpp"

int main() {
  using hbegp::FittedKernel;
  hbegp::Context ctx(1);
  const int n0 = 256, n = 300, d = 2, m = 9;
  std::vector<double> X(n * d), Y(n), V(n), Q(m * d);
  unsigned s = 1234;
  auto next = [&s]() { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.0; };
  for (auto& v : X) v = next();
  for (auto& v : Q) v = next();
  for (int i = 0; i < n; ++i) { Y[i] = std::sin(3 * X[2 * i]) + X[2 * i + 1]; V[i] = i % 7 == 0 ? 0.0 : 0.2 * next(); }
  const std::vector<double> th = {std::log(0.05), std::log(1.3), std::log(0.5), std::log(0.7)};
  int bad = 0;
  auto same = [&](const FittedKernel<double>& a, hbegp_model* b) {
    std::vector<double> ma(m), va(m), mb(m), vb(m);
    a.predict(Q.data(), m, ma.data(), va.data());
    if (hbegp_predict_f64(b, Q.data(), m, mb.data(), vb.data(), nullptr) != HBEGP_OK) return false;
    return std::memcmp(ma.data(), mb.data(), sizeof(double) * m) == 0 && std::memcmp(va.data(), vb.data(), sizeof(double) * m) == 0;
  };
  // extend with variances = hbegp_extend_rv_f64; the model hands them back
  auto fk = FittedKernel<double>::extend(ctx, X.data(), Y.data(), n, d, 2.5, th, nullptr, V.data());
  hbegp_model* raw = nullptr;
  if (hbegp_extend_rv_f64(ctx.get(), X.data(), Y.data(), V.data(), n, d, 2.5, th.data(), nullptr, nullptr, &raw) != HBEGP_OK) ++bad;
  if (!raw || !same(fk, raw)) ++bad;
  const std::vector<double> back = fk.row_variance();
  if ((int)back.size() != n || std::memcmp(back.data(), V.data(), sizeof(double) * n) != 0) ++bad;
  // without them: the plain model, and it differs
  auto plain = FittedKernel<double>::extend(ctx, X.data(), Y.data(), n, d, 2.5, th);
  if (!plain.row_variance().empty() || same(plain, raw)) ++bad;
  if (raw) hbegp_model_release(raw);
  // extend_with on a matching prefix runs incrementally and keeps the variances
  auto prior = FittedKernel<double>::extend(ctx, X.data(), Y.data(), n0, d, 2.5, th, nullptr, V.data());
  bool inc = false;
  auto ext = prior.extend_with(ctx, X.data(), Y.data(), n, &inc, V.data());
  if (!inc || ext.row_variance() != back || std::fabs(ext.lml() - fk.lml()) > 1e-8 * std::fmax(1.0, std::fabs(fk.lml()))) ++bad;
  // a fit with variances returns a model that carries them
  hbegp::KernelBounds b{{0.045, 0.8, 0.25, 0.25}, {0.3, 1.5, 1.3, 1.3}};
  auto fit = FittedKernel<double>::new_(ctx, X.data(), Y.data(), 100, d, 2.5, th, b, {}, 20, V.data());
  if ((int)fit.row_variance().size() != 100 || !std::isfinite(fit.lml())) ++bad;
  // refusals
  int threw = 0;
  try { prior.extend_with(ctx, X.data(), Y.data(), n); } catch (const hbegp::Error& e) { threw += e.code == HBEGP_EINVAL; }
  std::vector<double> neg(V);
  neg[3] = -1.0;
  try { FittedKernel<double>::extend(ctx, X.data(), Y.data(), n, d, 2.5, th, nullptr, neg.data()); } catch (const hbegp::Error& e) { threw += e.code == HBEGP_EINVAL; }
  std::printf("bad=%d threw=%d\n", bad, threw);
  return bad == 0 && threw == 2 ? 0 : 1;
}
