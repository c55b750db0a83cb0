// lockstep.hpp -- R bounded L-BFGS runs (lbfgs_step.hpp) driven in lockstep against ONE batched evaluation per round.
//
// Every multi-start optimiser of the posterior side (hbegp.cpp: maximize_ei, maximize_ehvi, maximize_qei, paths_minimize) is this
// loop around its own evaluator; nothing here knows about the device, so the loop is tested on the host
// (tests/cpp/test_lockstep.cpp replays every run alone through lbfgs_begin / lbfgs_request / lbfgs_advance, bit for bit).
#pragma once
#include <cmath>
#include <cstddef>
#include <limits>
#include <memory>
#include <type_traits>
#include <vector>

#include "lbfgs_step.hpp"

namespace hbegp {

// the element of type T nearest to v that lies in [lo, hi] (an f32 run evaluates, and returns, points of the box)
template <typename T>
inline T to_box(double v, double lo, double hi) {
  T t = (T)v;
  if ((double)t > hi) t = std::nextafter(t, -std::numeric_limits<T>::infinity());
  if ((double)t < lo) t = std::nextafter(t, std::numeric_limits<T>::infinity());
  return t;
}

struct LockstepOptions {
  int maxeval;    // evaluations per run
  int memory;     // lbfgs_begin's memory, pgtol, ftol
  double pgtol, ftol;
  bool maximize;  // the runs maximise the evaluator's value (they minimise its negative)
};

// Runs R optimisations over nvar variables in the box [lo, hi] (nvar each) from starts [R][nvar], St = LbfgsState (nvar <=
// LBFGS_MAXN) or LbfgsStateHost (any nvar).  Every round the points the unfinished runs ask for are snapped into the box
// (to_box<T>), packed in ascending run order and handed to
//     int eval(const T* xs /*[cnt][nvar]*/, const int* runs /*[cnt]*/, int cnt, double* val /*[cnt]*/, double* grad /*[cnt][nvar]*/,
//              char* ok /*[cnt]*/)
// which fills, per point, the value, its gradient and whether the evaluation worked (all three in the caller's sense: a
// maximiser reports the value it maximises).  A return other than 0 ends the call at once with that status.  An evaluation that
// is not ok is a failed one: the run sees f = +inf and it never becomes a best point.
// Out: per run the best point it evaluated and its value (x_best [R][nvar], f_best [R]; a run without a successful evaluation keeps
// its start and the failure value: +inf, -inf when maximising) and the evaluations it used (nevals [R], may be null).  x_best /
// f_best are current whenever eval is called: an evaluator may read them.
template <class T, class St, class Eval>
int lockstep_optimize(const T* starts, int R, int nvar, const double* lo, const double* hi, const LockstepOptions& o, Eval&& eval,
                      T* x_best, double* f_best, int* nevals) {
  const size_t n = (size_t)nvar;
  const double sign = o.maximize ? -1.0 : 1.0;  // the one place where maximising differs: the runs minimise sign * value
  std::vector<std::unique_ptr<St>> st((size_t)R);
  std::vector<double> x0(n);
  for (int r = 0; r < R; ++r) {
    if constexpr (std::is_constructible<St, int>::value) st[r].reset(new St(nvar));
    else st[r].reset(new St());
    for (size_t k = 0; k < n; ++k) x0[k] = (double)starts[r * n + k];
    lbfgs_begin(*st[r], x0.data(), lo, hi, nvar, o.maxeval, o.memory, o.pgtol, o.ftol, false);
    for (size_t k = 0; k < n; ++k) x_best[r * n + k] = starts[r * n + k];
    f_best[r] = sign * std::numeric_limits<double>::infinity();
  }
  std::vector<char> running((size_t)R, 1), ok((size_t)R);
  std::vector<int> act;
  act.reserve((size_t)R);
  std::vector<T> xs((size_t)R * n);
  std::vector<double> val((size_t)R), grad((size_t)R * n);
  for (;;) {
    act.clear();
    for (int r = 0; r < R; ++r)
      if (running[r]) act.push_back(r);
    if (act.empty()) break;
    const int cnt = (int)act.size();
    for (int i = 0; i < cnt; ++i) {
      const double* q = lbfgs_request(*st[act[i]]);
      for (size_t k = 0; k < n; ++k) xs[i * n + k] = to_box<T>(q[k], lo[k], hi[k]);
    }
    if (const int rc = eval((const T*)xs.data(), (const int*)act.data(), cnt, val.data(), grad.data(), ok.data())) return rc;
    for (int i = 0; i < cnt; ++i) {
      const int r = act[i];
      double* g = grad.data() + i * n;
      double f = std::numeric_limits<double>::infinity();
      if (ok[i]) {
        f = sign * val[i];
        for (size_t k = 0; k < n; ++k) g[k] = sign * g[k];
        if (f < sign * f_best[r]) {
          f_best[r] = val[i];
          for (size_t k = 0; k < n; ++k) x_best[r * n + k] = xs[i * n + k];
        }
      } else {
        // lbfgs_advance never reads the gradient of a failed evaluation (f not finite); it gets zeros, never what eval left there
        for (size_t k = 0; k < n; ++k) g[k] = 0.0;
      }
      running[r] = lbfgs_advance(*st[r], f, g) ? 1 : 0;
    }
  }
  if (nevals)
    for (int r = 0; r < R; ++r) nevals[r] = st[r]->nevals;
  return 0;
}

// The evaluator of an optimiser whose batched call hands back fp64 values and gradient rows of type T (hbegp.cpp: maximize_ehvi,
// maximize_constrained_ei, maximize_mes):
//     int rows(const T* xs /*[cnt][nvar]*/, int cnt, double* val /*[cnt]*/, T* gr /*[cnt][nvar]*/)
// The gradient rows are converted to double (exact for float and double), and an evaluation is ok iff its value and every
// component of its gradient row are finite.  A return of rows other than 0 is handed on and nothing else is touched.  R: the most
// rows a round can have.
template <class T, class Rows>
auto finite_gradient_eval(int R, int nvar, Rows rows) {
  return [rows, nvar, gr = std::vector<T>((size_t)R * (size_t)nvar)](const T* xs, const int*, int cnt, double* val, double* grad,
                                                                      char* ok) mutable -> int {
    if (const int rc = rows(xs, cnt, val, gr.data())) return rc;
    const size_t n = (size_t)nvar;
    for (int i = 0; i < cnt; ++i) {
      bool finite = std::isfinite(val[i]);
      for (size_t k = 0; k < n; ++k) {
        grad[i * n + k] = (double)gr[i * n + k];
        finite = finite && std::isfinite(grad[i * n + k]);
      }
      ok[i] = finite ? 1 : 0;
    }
    return 0;
  };
}

}  // namespace hbegp
