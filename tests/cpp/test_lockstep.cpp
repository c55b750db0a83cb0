// The lockstep driver of csrc/lockstep.hpp (the loop of maximize_ei / maximize_ehvi / maximize_qei / paths_minimize) on host
// objectives: a bounded quadratic and a Rosenbrock, each with a shell that returns +inf and one that returns NaN.  Every one of
// the R runs is compared, bit for bit, with the same run driven ALONE through lbfgs_begin / lbfgs_request / lbfgs_advance:
//   * every requested point after to_box, the best point, the best value, nevals;
//   * R = 1 and 7, nvar = 1, 3, 8, LbfgsStateHost at nvar = 70 (> LBFGS_MAXN), T = double and float (starts on the box's faces, whose
//     bounds no float represents: every point handed to the evaluator lies in the box), maxeval = 1 and 150, both signs;
//   * a run whose every evaluation fails keeps its start and the failure value (+inf, -inf when maximising);
//   * the gradient of a failed evaluation is poisoned (NaN in one pass, 1e300 in the other): nothing depends on it;
//   * an evaluator that returns a status in round 2 ends the call with that status, and is not called again.
// And finite_gradient_eval, the evaluator of the maximisers whose batched call returns T gradient rows (adaptor_case below).
// Build + run (CPU): g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Icsrc tests/cpp/test_lockstep.cpp -o build/test_lockstep && build/test_lockstep
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "lockstep.hpp"

using namespace hbegp;

struct Rng {
  uint64_t s;
  double uni() {  // [0, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
  }
};

struct Obj {
  int kind = 0;  // 0: quadratic whose optimum lies outside the box in some coordinates, 1: Rosenbrock
  int n = 1;
  std::vector<double> c, w;
  double r_inf = 1e300, r_nan = 1e300;  // distance from c beyond which the value is +inf / NaN
};

static double objective(const Obj& o, const double* x, double* g) {
  const int n = o.n;
  double r2 = 0;
  for (int i = 0; i < n; ++i) r2 += (x[i] - o.c[i]) * (x[i] - o.c[i]);
  if (r2 > o.r_nan * o.r_nan) return NAN;
  if (r2 > o.r_inf * o.r_inf) return INFINITY;
  double f = 0;
  if (o.kind == 0) {
    for (int i = 0; i < n; ++i) {
      const double u = x[i] - o.c[i];
      f += 0.5 * o.w[i] * u * u;
      g[i] = o.w[i] * u;
    }
    return f;
  }
  for (int i = 0; i < n; ++i) g[i] = 0;
  for (int i = 0; i < n; ++i) {
    f += (1.0 - x[i]) * (1.0 - x[i]);
    g[i] += -2.0 * (1.0 - x[i]);
    if (i + 1 < n) {
      const double t = x[i + 1] - x[i] * x[i];
      f += 100.0 * t * t;
      g[i] += -400.0 * t * x[i];
      g[i + 1] += 200.0 * t;
    }
  }
  return f;
}

struct Counts {
  long evals = 0, inf = 0, nan = 0, all_failed = 0, long_runs = 0, outside = 0;
};

template <typename T>
struct RunTrace {
  std::vector<T> req, best;
  double fbest = 0;
  int nevals = 0;
};

static const int kMemory = 10;
static const double kPgtol = 1e-7, kFtol = 1e-13;

// one run alone, as the four loops of hbegp.cpp each spelled it out
template <typename T, class St>
static void solo(St& st, const Obj& o, const T* start, const double* lo, const double* hi, int maxeval, bool maximize, RunTrace<T>* tr,
                 Counts* cn) {
  const int n = o.n;
  std::vector<double> x0(n), xd(n), g(n);
  std::vector<T> x(n);
  for (int k = 0; k < n; ++k) x0[k] = (double)start[k];
  lbfgs_begin(st, x0.data(), lo, hi, n, maxeval, kMemory, kPgtol, kFtol, false);
  tr->best.assign(start, start + n);
  double bestf = INFINITY;
  long ok_evals = 0;
  for (;;) {
    const double* q = lbfgs_request(st);
    for (int k = 0; k < n; ++k) {
      x[k] = to_box<T>(q[k], lo[k], hi[k]);
      xd[k] = (double)x[k];
      if (!(xd[k] >= lo[k] && xd[k] <= hi[k])) ++cn->outside;
    }
    tr->req.insert(tr->req.end(), x.begin(), x.end());
    double f = objective(o, xd.data(), g.data());
    ++cn->evals;
    if (std::isnan(f)) ++cn->nan;
    if (std::isinf(f)) ++cn->inf;
    if (!std::isfinite(f)) {
      f = INFINITY;
      for (int k = 0; k < n; ++k) g[k] = 0.0;
    } else {
      ++ok_evals;
      if (f < bestf) {
        bestf = f;
        tr->best = x;
      }
    }
    if (!lbfgs_advance(st, f, g.data())) break;
  }
  tr->fbest = maximize ? -bestf : bestf;
  tr->nevals = st.nevals;
  if (ok_evals == 0) ++cn->all_failed;
  if (ok_evals > 10) ++cn->long_runs;
}

template <typename T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static int g_cases = 0, g_problems = 0;

template <typename T, class St>
static void run_case(const char* name, int kind, int R, int n, bool maximize, int maxeval, uint64_t seed, Counts* cn) {
  Rng rng{seed};
  Obj o;
  o.kind = kind;
  o.n = n;
  o.c.resize(n);
  o.w.resize(n);
  std::vector<double> lo(n), hi(n);
  for (int i = 0; i < n; ++i) {
    o.c[i] = kind == 0 ? 2.0 * rng.uni() - 1.0 : 1.0;
    o.w[i] = std::pow(10.0, 2.0 * rng.uni() - 1.0);
    // bounds that no float represents; the quadratic's optimum is inside for some coordinates and beyond a face for others
    lo[i] = o.c[i] - 0.1 - 2.1 * rng.uni();
    hi[i] = o.c[i] - 0.3 + 2.3 * rng.uni();
    if (hi[i] < lo[i] + 0.1) hi[i] = lo[i] + 0.1;
  }
  // the shells cut the box: some starts lie inside them (a run whose every evaluation fails), trial steps overshoot into them
  o.r_inf = (0.9 + 0.5 * rng.uni()) * std::sqrt((double)n);
  o.r_nan = o.r_inf * (1.15 + 0.3 * rng.uni());
  std::vector<T> starts((size_t)R * n);
  for (int r = 0; r < R; ++r)
    for (int k = 0; k < n; ++k) {
      const double u = rng.uni();
      double v = lo[k] + (hi[k] - lo[k]) * rng.uni();
      if (u < 0.15) v = lo[k];  // on a face: to_box has to bring the rounded value back into the box
      else if (u < 0.3) v = hi[k];
      starts[(size_t)r * n + k] = to_box<T>(v, lo[k], hi[k]);
    }
  if (R > 1) {  // one run that starts in the NaN shell's corner when the box reaches it, whatever the draw
    for (int k = 0; k < n; ++k) starts[k] = to_box<T>(lo[k], lo[k], hi[k]);
  }
  // each run alone
  std::vector<RunTrace<T>> ref(R);
  for (int r = 0; r < R; ++r) {
    std::unique_ptr<St> st;
    if constexpr (std::is_constructible<St, int>::value) st.reset(new St(n));
    else st.reset(new St);
    solo<T, St>(*st, o, starts.data() + (size_t)r * n, lo.data(), hi.data(), maxeval, maximize, &ref[r], cn);
  }
  // all runs in lockstep, the gradient of every failed evaluation poisoned
  const LockstepOptions opt{maxeval, kMemory, kPgtol, kFtol, maximize};
  bool same = true;
  const double poisons[2] = {NAN, 1e300};
  for (double poison : poisons) {
    std::vector<std::vector<T>> req(R);
    std::vector<T> xb((size_t)R * n, (T)-7);
    std::vector<double> fb(R, -7.0);
    std::vector<int> ne(R, -7);
    std::vector<double> xd(n);
    int last_cnt = R + 1;
    bool order_ok = true;
    const int rc = lockstep_optimize<T, St>(
        starts.data(), R, n, lo.data(), hi.data(), opt,
        [&](const T* xs, const int* runs, int cnt, double* val, double* grad, char* ok) {
          if (cnt < 1 || cnt > last_cnt) order_ok = false;  // runs only ever leave
          last_cnt = cnt;
          for (int i = 0; i < cnt; ++i) {
            if (runs[i] < 0 || runs[i] >= R || (i > 0 && runs[i] <= runs[i - 1])) {
              order_ok = false;
              continue;
            }
            req[runs[i]].insert(req[runs[i]].end(), xs + (size_t)i * n, xs + (size_t)(i + 1) * n);
            for (int k = 0; k < n; ++k) xd[k] = (double)xs[(size_t)i * n + k];
            double* g = grad + (size_t)i * n;
            const double f = objective(o, xd.data(), g);
            ok[i] = std::isfinite(f) ? 1 : 0;
            val[i] = maximize ? -f : f;
            for (int k = 0; k < n; ++k) g[k] = ok[i] ? (maximize ? -g[k] : g[k]) : poison;
          }
          return 0;
        },
        xb.data(), fb.data(), ne.data());
    same = same && rc == 0 && order_ok;
    for (int r = 0; r < R; ++r) {
      const std::vector<T> xr(xb.begin() + (size_t)r * n, xb.begin() + (size_t)(r + 1) * n);
      same = same && same_bits(req[r], ref[r].req) && same_bits(xr, ref[r].best) && memcmp(&fb[r], &ref[r].fbest, sizeof(double)) == 0 &&
             ne[r] == ref[r].nevals && (int)(req[r].size() / n) == ne[r];
      if (ref[r].nevals > maxeval) same = false;
      // a run without a successful evaluation: its start and the failure value
      if (!std::isfinite(ref[r].fbest)) {
        const std::vector<T> s0(starts.begin() + (size_t)r * n, starts.begin() + (size_t)(r + 1) * n);
        same = same && same_bits(xr, s0) && fb[r] == (maximize ? -INFINITY : INFINITY);
      }
    }
  }
  ++g_cases;
  if (!same) ++g_problems;
  printf("%s kind %d R %d n %d %s maxeval %d %s\n", name, kind, R, n, maximize ? "max" : "min", maxeval, same ? "same: yes" : "DIFFERENT");
}

// an evaluator that fails in round 2: the driver returns its status and stops calling
static void status_case() {
  const int R = 4, n = 3;
  std::vector<double> lo(n, -2.0), hi(n, 2.0), starts((size_t)R * n, 0.5), xb((size_t)R * n), fb(R);
  std::vector<int> ne(R, -7);
  int calls = 0;
  const LockstepOptions opt{150, kMemory, kPgtol, kFtol, false};
  const int rc = lockstep_optimize<double, LbfgsState>(
      starts.data(), R, n, lo.data(), hi.data(), opt,
      [&](const double* xs, const int*, int cnt, double* val, double* grad, char* ok) {
        if (++calls == 2) return 42;
        for (int i = 0; i < cnt; ++i) {
          val[i] = 0;
          for (int k = 0; k < n; ++k) {
            const double u = xs[(size_t)i * n + k] - 1.0;
            val[i] += u * u;
            grad[(size_t)i * n + k] = 2.0 * u;
          }
          ok[i] = 1;
        }
        return 0;
      },
      xb.data(), fb.data(), ne.data());
  const bool same = rc == 42 && calls == 2;
  ++g_cases;
  if (!same) ++g_problems;
  printf("status in round 2: rc %d after %d calls %s\n", rc, calls, same ? "same: yes" : "DIFFERENT");
}

// finite_gradient_eval: the evaluator around a batched call that returns fp64 values and gradient rows of type T.  Row i of a case
// is of kind (first + i) % 7: clean; the value NaN, +inf, -inf; the LAST gradient component alone NaN, +inf, -inf.  Only the clean
// row is ok; every gradient component arrives as the double of the T the call wrote (exactly: the way back gives the same T bits),
// the values stay as the call wrote them, the call sees the driver's xs and cnt, nothing behind row cnt is written, and a status
// of the call is handed on with nothing written at all.
static int g_adaptor_cases = 0, g_adaptor_problems = 0;

template <typename T>
static void adaptor_case(const char* name, int d, int cnt, int first) {
  const int R = cnt + 2;  // the buffers hold more rows than the round has
  const double sentinel = -7.25;
  std::vector<T> xs((size_t)R * d, (T)0.5), wrote((size_t)cnt * d);
  std::vector<double> wrote_val(cnt);
  const T* seen_xs = nullptr;
  int seen_cnt = -1, status = 0;
  auto rows = [&](const T* x, int c, double* val, T* gr) {
    seen_xs = x;
    seen_cnt = c;
    if (status) return status;
    for (int i = 0; i < c; ++i) {
      const int kind = (first + i) % 7;
      val[i] = kind == 1 ? (double)NAN : kind == 2 ? (double)INFINITY : kind == 3 ? -(double)INFINITY : 0.3 * (i + 1);
      for (int k = 0; k < d; ++k) gr[(size_t)i * d + k] = (T)(0.1 * (i + 1) - 0.7 * k);  // not representable: the float rounds
      T& last = gr[(size_t)i * d + d - 1];
      if (kind == 4) last = (T)NAN;
      if (kind == 5) last = (T)INFINITY;
      if (kind == 6) last = -(T)INFINITY;
    }
    std::copy(val, val + c, wrote_val.begin());
    std::copy(gr, gr + (size_t)c * d, wrote.begin());
    return 0;
  };
  auto eval = finite_gradient_eval<T>(R, d, rows);
  bool good = true;
  for (int pass = 0; pass < 2; ++pass) {  // the second pass: the call refuses
    status = pass ? 42 : 0;
    std::vector<double> val(R, sentinel), grad((size_t)R * d, sentinel);
    std::vector<char> ok(R, 9);
    const int rc = eval(xs.data(), nullptr, cnt, val.data(), grad.data(), ok.data());
    good = good && rc == status && seen_xs == xs.data() && seen_cnt == cnt;
    const int written = pass ? 0 : cnt;
    for (int i = 0; i < written; ++i) {
      good = good && ok[i] == ((first + i) % 7 == 0 ? 1 : 0) && memcmp(&val[i], &wrote_val[i], sizeof(double)) == 0;
      for (int k = 0; k < d; ++k) {
        const double g = grad[(size_t)i * d + k];
        const T w = wrote[(size_t)i * d + k], back = (T)g;
        good = good && (std::isnan(w) ? std::isnan(g) : (g == (double)w && memcmp(&back, &w, sizeof(T)) == 0));
      }
    }
    for (int i = written; i < R; ++i) {
      good = good && ok[i] == 9 && val[i] == sentinel;
      for (int k = 0; k < d; ++k) good = good && grad[(size_t)i * d + k] == sentinel;
    }
  }
  ++g_adaptor_cases;
  if (!good) ++g_adaptor_problems;
  printf("adaptor %s d %d cnt %d first kind %d %s\n", name, d, cnt, first, good ? "adaptor: ok" : "adaptor: WRONG");
}

int main() {
  for (int d : {1, 2, 5})
    for (int first = 0; first < 7; ++first) {  // cnt = 1: every kind alone
      adaptor_case<double>("f64", d, 1, first);
      adaptor_case<float>("f32", d, 1, first);
    }
  for (int d : {1, 2, 5})
    for (int first : {0, 3}) {  // every kind in one round, a clean row first and in the middle
      adaptor_case<double>("f64", d, 9, first);
      adaptor_case<float>("f32", d, 9, first);
    }
  printf("%d adaptor cases, %d problems\n", g_adaptor_cases, g_adaptor_problems);
  if (g_adaptor_problems) ++g_problems;
  Counts cn;
  uint64_t seed = 20251019;
  for (int kind = 0; kind < 2; ++kind)
    for (int R : {1, 7})
      for (int n : {1, 3, 8})
        for (int maximize = 0; maximize < 2; ++maximize) {
          run_case<double, LbfgsState>("f64", kind, R, n, maximize != 0, 150, ++seed, &cn);
          run_case<float, LbfgsState>("f32", kind, R, n, maximize != 0, 150, ++seed, &cn);
        }
  for (int kind = 0; kind < 2; ++kind) {
    run_case<double, LbfgsState>("f64", kind, 7, 3, kind != 0, 1, ++seed, &cn);
    run_case<float, LbfgsState>("f32", kind, 7, 8, kind == 0, 1, ++seed, &cn);
    run_case<double, LbfgsStateHost>("f64 host state", kind, 7, 70, true, 150, ++seed, &cn);
    run_case<float, LbfgsStateHost>("f32 host state", kind, 1, 70, false, 150, ++seed, &cn);
    run_case<double, LbfgsStateHost>("f64 host state", kind, 7, 3, false, 150, ++seed, &cn);
  }
  status_case();
  // the cases have to reach what they are about
  const bool reached = cn.inf > 20 && cn.nan > 20 && cn.all_failed > 5 && cn.long_runs > 50 && cn.outside == 0;
  printf("%ld evaluations: %ld +inf, %ld NaN, %ld runs without a success, %ld runs of > 10 successes, %ld points outside the box: %s\n", cn.evals,
         cn.inf, cn.nan, cn.all_failed, cn.long_runs, cn.outside, reached ? "reached" : "NOT REACHED");
  if (!reached) ++g_problems;
  printf("%d cases, %d problems\n", g_cases, g_problems);
  return g_problems ? 1 : 0;
}
