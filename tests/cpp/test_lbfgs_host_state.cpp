// The host-only L-BFGS state (LbfgsStateHost, csrc/lbfgs_step.hpp: arrays sized per run) must drive the same state machine as the
// fixed-size LbfgsState that small_fit_kernel shares: at n <= LBFGS_MAXN both ask for the same points, bit for bit, and end in the
// same state; beyond LBFGS_MAXN it evaluates the points of the loop form (lbfgsb_minimize_loops).  LbfgsState's layout is pinned.
// Build + run (CPU): g++ -O2 -std=c++17 -ffp-contract=off -Icsrc tests/cpp/test_lbfgs_host_state.cpp -o build/t && build/t
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lbfgsb.hpp"

using namespace hbegp;

// the layout small_fit_kernel shares through engine.hpp (the state lives in device memory)
static_assert(sizeof(LbfgsState) == 13896, "LbfgsState size");
static_assert(offsetof(LbfgsState, pgtol) == 16 && offsetof(LbfgsState, fixed_work) == 32 && offsetof(LbfgsState, lo) == 40 &&
                  offsetof(LbfgsState, hi) == 568 && offsetof(LbfgsState, phase) == 1096 && offsetof(LbfgsState, hcount) == 1112 &&
                  offsetof(LbfgsState, f) == 1120 && offsetof(LbfgsState, gs) == 1136 && offsetof(LbfgsState, x) == 1144 &&
                  offsetof(LbfgsState, g) == 1672 && offsetof(LbfgsState, xn) == 2200 && offsetof(LbfgsState, d) == 2728 &&
                  offsetof(LbfgsState, S) == 3256 && offsetof(LbfgsState, Y) == 8536 && offsetof(LbfgsState, rho) == 13816,
              "LbfgsState field offsets");

static double objective(int kind, int n, const double* x, double* g) {
  double f = 0;
  switch (kind) {
    case 0:  // slanted plane: ends in the corner of the box
      for (int i = 0; i < n; ++i) { f += (i + 1) * x[i]; g[i] = i + 1; }
      return f;
    case 1:  // Rosenbrock
      for (int i = 0; i < n; ++i) g[i] = 0;
      for (int i = 0; i + 1 < n; ++i) {
        const double a = x[i + 1] - x[i] * x[i], b = 1 - x[i];
        f += 100 * a * a + b * b;
        g[i] += -400 * x[i] * a - 2 * b;
        g[i + 1] += 200 * a;
      }
      return f;
    case 2:  // ill-conditioned quadratic
      for (int i = 0; i < n; ++i) { const double w = std::pow(10.0, 3.0 * i / (n - 1.0)); f += 0.5 * w * (x[i] - 0.3) * (x[i] - 0.3); g[i] = w * (x[i] - 0.3); }
      return f;
    default: {  // fails (+inf) outside a ball, NaN further out
      double r2 = 0;
      for (int i = 0; i < n; ++i) r2 += x[i] * x[i];
      if (r2 > 9.0) return NAN;
      if (r2 > 4.0) return INFINITY;
      for (int i = 0; i < n; ++i) { f += std::cos(x[i]) + 0.1 * x[i]; g[i] = -std::sin(x[i]) + 0.1; }
      return f;
    }
  }
}

template <class St>
static void run(St& st, int n, int kind, const std::vector<double>& x0, const std::vector<double>& lo, const std::vector<double>& hi,
                const LbfgsOptions& o, std::vector<std::vector<double>>& seq) {
  std::vector<double> g(n);
  lbfgs_begin(st, x0.data(), lo.data(), hi.data(), n, o.maxeval, o.memory, o.pgtol, o.ftol, o.fixed_work);
  for (;;) {
    const double* q = lbfgs_request(st);
    seq.push_back(std::vector<double>(q, q + n));
    const double f = objective(kind, n, q, g.data());
    if (!lbfgs_advance(st, f, g.data())) break;
  }
}

int main() {
  struct C { const char* name; int n, kind, maxeval, memory; bool fixed; double x0, lo, hi; };
  const C cases[] = {
      {"plane", 3, 0, 150, 10, false, 0.5, -1, 2},          {"rosenbrock", 8, 1, 150, 10, false, -0.5, -2.5, 2.5},
      {"rosenbrock memory 3", 8, 1, 150, 3, false, -0.5, -2.5, 2.5}, {"rosenbrock 66", 66, 1, 150, 10, true, -0.5, -2.5, 2.5},
      {"quadratic maxeval 7", 10, 2, 7, 10, true, 2.0, -5, 5},  {"failing region", 4, 3, 150, 10, false, 0.4, -5, 5},
      {"quadratic 40", 40, 2, 150, 10, false, 2.0, -5, 5},     {"rosenbrock 80", 80, 1, 150, 10, false, -0.5, -2.5, 2.5},
      {"quadratic 640", 640, 2, 150, 10, false, 2.0, -5, 5},   {"failing region 300", 300, 3, 150, 10, true, 0.04, -5, 5},
  };
  int bad = 0;
  for (const C& c : cases) {
    std::vector<double> x0(c.n), lo(c.n, c.lo), hi(c.n, c.hi);
    for (int i = 0; i < c.n; ++i) x0[i] = c.x0 + 0.37 * std::sin(1.0 + 3.0 * i);
    LbfgsOptions o;
    o.maxeval = c.maxeval; o.memory = c.memory; o.fixed_work = c.fixed;
    std::vector<std::vector<double>> seq[2];
    LbfgsStateHost hs(c.n);
    run(hs, c.n, c.kind, x0, lo, hi, o, seq[1]);
    bool ok = true;
    if (c.n <= LBFGS_MAXN) {
      std::vector<LbfgsState> fs(1);
      LbfgsState& s = fs[0];
      run(s, c.n, c.kind, x0, lo, hi, o, seq[0]);
      ok = s.nevals == hs.nevals && s.iterations == hs.iterations && s.converged == hs.converged && s.phase == hs.phase &&
           s.hcount == hs.hcount && std::memcmp(&s.f, &hs.f, 8) == 0 && std::memcmp(s.x, hs.x, 8 * c.n) == 0;
      for (int h = 0; ok && h < s.hcount; ++h)
        ok = std::memcmp(s.S[h], hs.S[h], 8 * c.n) == 0 && std::memcmp(s.Y[h], hs.Y[h], 8 * c.n) == 0 &&
             std::memcmp(&s.rho[h], &hs.rho[h], 8) == 0;
    } else {
      std::vector<double> x = x0;
      Objective fun = [&](const double* xx, double* g) {
        seq[0].push_back(std::vector<double>(xx, xx + c.n));
        return objective(c.kind, c.n, xx, g);
      };
      const LbfgsResult r = lbfgsb_minimize_loops(fun, x.data(), lo.data(), hi.data(), c.n, o);
      ok = r.nevals == hs.nevals && r.iterations == hs.iterations && std::memcmp(&r.f, &hs.f, 8) == 0 &&
           std::memcmp(x.data(), hs.x, 8 * c.n) == 0;
    }
    ok = ok && seq[0].size() == seq[1].size();
    for (size_t e = 0; ok && e < seq[0].size(); ++e) ok = std::memcmp(seq[0][e].data(), seq[1][e].data(), 8 * c.n) == 0;
    std::printf("%-24s n=%-4d %s: %zu evaluations, %d iterations, f = %.17g\n", c.name, c.n, ok ? "same" : "DIFFERENT", seq[1].size(),
                hs.iterations, hs.f);
    if (!ok) ++bad;
  }
  return bad ? 1 : 0;
}
