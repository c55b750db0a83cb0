// The decision query of csrc/lbfgs_step.hpp (lbfgs_is_trial / lbfgs_trial_accepted) is what a fit asks before it pays for the
// gradient of a line-search trial.  It has to say exactly what lbfgs_advance then does:
//   * at every evaluation, "accepted" == lbfgs_advance took its accepted branch (the only place a trial's gradient is read);
//   * a run in which every trial the query rejects is handed a POISONED gradient (NaN) evaluates exactly the points of the loop
//     form (lbfgsb_minimize_loops) with the true gradients, bit for bit, and ends in the same state;
//   * a rejected trial can still be the best value so far (between f + 1e-4 gs and f): the constructed case has one.
// Randomised bounded objectives, with regions that fail (+inf) and regions that return NaN.
// Build + run (CPU): g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Icsrc tests/cpp/test_lbfgs_decision.cpp -o build/test_lbfgs_decision && build/test_lbfgs_decision
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "lbfgsb.hpp"

using namespace hbegp;

struct Rng {
  uint64_t s;
  double uni() {  // [0, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
  }
};

struct Case {
  int kind = 0;  // 0: random quadratic + ripple with failing shells, 1: the constructed overshoot
  int n = 1;
  std::vector<double> x0, lo, hi, w, c;
  double ripple = 0, r_inf = 1e300, r_nan = 1e300;
  LbfgsOptions opt;
};

static double objective(const Case& k, const double* x, double* g) {
  const int n = k.n;
  if (k.kind == 1) {  // 100 x^2 in every coordinate: the unit first step from just right of 0.5 lands just left of -0.5
    double f = 0;
    for (int i = 0; i < n; ++i) { f += 100.0 * x[i] * x[i]; g[i] = 200.0 * x[i]; }
    return f;
  }
  double r2 = 0;
  for (int i = 0; i < n; ++i) r2 += (x[i] - k.c[i]) * (x[i] - k.c[i]);
  if (r2 > k.r_nan * k.r_nan) return NAN;
  if (r2 > k.r_inf * k.r_inf) return INFINITY;
  double f = 0;
  for (int i = 0; i < n; ++i) {
    const double u = x[i] - k.c[i];
    f += 0.5 * k.w[i] * u * u + k.ripple * std::cos(3.0 * u + i);
    g[i] = k.w[i] * u - 3.0 * k.ripple * std::sin(3.0 * u + i);
  }
  return f;
}

int main() {
  std::vector<Case> cases;
  Rng rng{20240607};
  for (int t = 0; t < 48; ++t) {
    Case k;
    k.n = 1 + (int)(rng.uni() * 12);
    if (t % 12 == 11) k.n = 66;
    k.x0.resize(k.n); k.lo.resize(k.n); k.hi.resize(k.n); k.w.resize(k.n); k.c.resize(k.n);
    for (int i = 0; i < k.n; ++i) {
      k.c[i] = 2.0 * rng.uni() - 1.0;
      k.w[i] = std::pow(10.0, 3.0 * rng.uni() - 1.0);
      k.lo[i] = k.c[i] - 0.2 - 3.0 * rng.uni();  // the optimum is inside for some coordinates, on a face for others
      k.hi[i] = k.c[i] - 0.4 + 3.0 * rng.uni();
      if (k.hi[i] < k.lo[i] + 0.1) k.hi[i] = k.lo[i] + 0.1;
      k.x0[i] = k.lo[i] + (k.hi[i] - k.lo[i]) * rng.uni();
    }
    k.ripple = t % 3 == 0 ? 0.0 : 0.3 * rng.uni();
    if (t % 2 == 1) {  // failing shells around the centre: trials overshoot into them and have to back off
      double r0 = 0;
      for (int i = 0; i < k.n; ++i) r0 += (k.x0[i] - k.c[i]) * (k.x0[i] - k.c[i]);
      k.r_inf = std::sqrt(r0) * (1.02 + 0.3 * rng.uni());
      k.r_nan = k.r_inf * (1.1 + 0.5 * rng.uni());
      if (t % 8 == 7) k.r_inf = 0.5 * std::sqrt(r0);  // the start point itself fails
    }
    k.opt.maxeval = t % 5 == 4 ? 1 + (int)(rng.uni() * 9) : 150;
    k.opt.memory = t % 7 == 6 ? 3 : 10;
    k.opt.fixed_work = t % 4 < 2;
    cases.push_back(k);
  }
  for (int n : {1, 3}) {
    Case k;
    k.kind = 1; k.n = n;
    k.x0.assign(n, 0.50002); k.lo.assign(n, -4.0); k.hi.assign(n, 4.0);
    if (n == 3) { k.x0[1] = 0.0; k.x0[2] = 0.0; }  // (the direction's norm stays that of the first coordinate)
    k.opt.maxeval = 40; k.opt.fixed_work = n == 1;
    cases.push_back(k);
  }

  int bad = 0, n_trials = 0, n_rejected = 0, n_rejected_best = 0, n_nonfinite = 0;
  for (size_t ci = 0; ci < cases.size(); ++ci) {
    const Case& k = cases[ci];
    // the loop form with the true gradients
    std::vector<std::vector<double>> seq_loops;
    std::vector<double> x = k.x0;
    Objective fun = [&](const double* xx, double* g) {
      seq_loops.push_back(std::vector<double>(xx, xx + k.n));
      return objective(k, xx, g);
    };
    const LbfgsResult rl = lbfgsb_minimize_loops(fun, x.data(), k.lo.data(), k.hi.data(), k.n, k.opt);
    // the state machine, asked before every evaluation's gradient is handed over
    std::unique_ptr<LbfgsState> st(new LbfgsState);
    lbfgs_begin(*st, k.x0.data(), k.lo.data(), k.hi.data(), k.n, k.opt.maxeval, k.opt.memory, k.opt.pgtol, k.opt.ftol, k.opt.fixed_work);
    std::vector<std::vector<double>> seq_sm;
    std::vector<double> g(k.n), poison(k.n, NAN);
    double best = INFINITY;
    bool ok = true;
    int case_rejected_best = 0;
    for (;;) {
      const double* q = lbfgs_request(*st);
      seq_sm.push_back(std::vector<double>(q, q + k.n));
      const double f = objective(k, q, g.data());
      const bool trial = lbfgs_is_trial(*st);
      const bool accepted = lbfgs_trial_accepted(*st, f);
      if (accepted && !trial) ok = false;
      if (!(f - f == 0.0)) { ++n_nonfinite; if (accepted) ok = false; }
      const bool new_best = f - f == 0.0 && f < best;
      if (new_best) best = f;
      if (trial) {
        ++n_trials;
        if (!accepted) { ++n_rejected; if (new_best) { ++n_rejected_best; ++case_rejected_best; } }
      }
      const int it0 = st->iterations;
      const bool more = lbfgs_advance(*st, f, (trial && !accepted) ? poison.data() : g.data());
      if ((st->iterations != it0) != accepted) ok = false;  // the accepted branch is the one that counts an iteration
      if (!more) break;
    }
    ok = ok && seq_sm.size() == seq_loops.size() && st->nevals == rl.nevals && st->iterations == rl.iterations &&
         (st->converged != 0) == rl.converged && std::memcmp(&st->f, &rl.f, 8) == 0 && std::memcmp(st->x, x.data(), 8 * k.n) == 0;
    for (size_t e = 0; ok && e < seq_sm.size(); ++e) ok = std::memcmp(seq_sm[e].data(), seq_loops[e].data(), 8 * k.n) == 0;
    if (k.kind == 1 && case_rejected_best == 0) ok = false;  // the constructed case must show a rejected trial that is a new best
    std::printf("case %2zu n=%2d %s: %zu evaluations, %d iterations\n", ci, k.n, ok ? "same" : "DIFFERENT", seq_sm.size(), st->iterations);
    if (!ok) ++bad;
  }
  std::printf("%d trials, %d rejected, %d of them a new best, %d non-finite values, %d problems\n", n_trials, n_rejected, n_rejected_best,
              n_nonfinite, bad);
  // the cases must really exercise what they are for
  if (n_rejected < 20 || n_rejected_best < 2 || n_nonfinite < 5) { std::printf("the cases do not cover the decision\n"); return 2; }
  return bad ? 1 : 0;
}
