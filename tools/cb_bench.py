"""Times of the confidence bound mu + kappa sigma (hbegp_confidence_bound_*, hbegp_minimize_confidence_bound_*) beside what the
library offered before them.  extend() at a fixed theta on the C2 workload (Rosenbrock, d = 8), f64, kappa = 1:

 (a) n = 4096: confidence_bound with a gradient at m in {16, 256, 4096} -- its phases by device events (hbegp_debug_cb_phases: the
     predict with the gradient's launches; the kernel with the arg-min) and the wall time of the call -- beside the same numbers
     composed on the host: predict_with_gradient, then tests/cb_ref.py in NumPy.
 (b) n = 4096: minimize_confidence_bound, S = 10 runs from the ten training rows of lowest bound, maxeval = 150, beside the
     reference's pattern as the library served it: 150 single-point predict_confidence_bound calls at the scan's winner (what a
     derivative-free minimiser pays for its evaluations, whatever points it chooses).
 (c) the same at n = 128.

    python tools/cb_bench.py [--reps 5] [--out FILE]

Prints one JSON object per measurement and two tables at the end (medians of synchronous calls).  There is no pass bar."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cb_ref  # noqa: E402
from hbetune_rs_amd import _lib  # noqa: E402
from hbetune_rs_amd import estimator as E  # noqa: E402
from hbetune_rs_amd import gpr, synth  # noqa: E402

KAPPA = 1.0


def wall_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    dtype = np.float64
    calls, runs = [], []
    phases = np.zeros(2)
    for n in (4096, 128):
        w = synth.make_workload("C2", n=n)
        X = np.asarray(w["X"], dtype=np.float64).astype(dtype)
        y = np.asarray(w["y"], dtype=np.float64)
        d = X.shape[1]
        theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
        fk = gpr.FittedKernel.extend(X, y.astype(dtype), theta, nu=2.5)
        if n == 4096:
            lib.hbegp_debug_cb_phases(1, None)
            for m in (16, 256, 4096):
                Xs = synth.candidates("C2", m, d).astype(dtype)
                fk.confidence_bound(Xs, KAPPA, want_grad=True)
                wall, ph = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    val, best, grad = fk.confidence_bound(Xs, KAPPA, want_grad=True)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    lib.hbegp_debug_cb_phases(1, _lib.dptr(phases))
                    ph.append(phases.copy())
                ph = np.median(np.array(ph), axis=0)
                lib.hbegp_debug_cb_phases(0, None)
                untimed = wall_ms(lambda: fk.confidence_bound(Xs, KAPPA, want_grad=True), a.reps)
                lib.hbegp_debug_cb_phases(1, None)
                post = fk.predict_with_gradient(Xs)
                host_predict = wall_ms(lambda: fk.predict_with_gradient(Xs), a.reps)
                host_compose = wall_ms(lambda: cb_ref.cb_grad(post[0], post[1], post[2], post[3], KAPPA), a.reps, warmup=0)
                rv, rg, _ = cb_ref.cb_grad(post[0], post[1], post[2], post[3], KAPPA)
                rec = dict(part="a", n=n, d=d, m=m, predict_ms=round(float(ph[0]), 4), kernel_ms=round(float(ph[1]), 4),
                           call_ms=round(float(np.median(wall)), 4), untimed_call_ms=round(untimed, 4),
                           host_predict_grad_ms=round(host_predict, 4), host_compose_ms=round(host_compose, 4),
                           kernel_share=round(float(ph[1] / ph[0]), 5), best=best, dev_value=float(np.abs(val - rv).max()),
                           dev_grad=float(np.abs(grad - rg).max()))
                print(json.dumps(rec), flush=True)
                calls.append(rec)
            lib.hbegp_debug_cb_phases(0, None)
        # (b), (c): the ten training rows of lowest bound start the runs; the box is the data's
        lo, hi = X.min(axis=0).astype(np.float64), X.max(axis=0).astype(np.float64)
        cb_train, winner = fk.confidence_bound(X, KAPPA)
        starts = X[np.argsort(cb_train, kind="stable")[:10]]
        x, val, nevals = fk.minimize_confidence_bound(starts, lo, hi, KAPPA, maxeval=150)
        t_min = wall_ms(lambda: fk.minimize_confidence_bound(starts, lo, hi, KAPPA, maxeval=150), a.reps, warmup=0)
        x1, val1, nevals1 = fk.minimize_confidence_bound(starts[:1], lo, hi, KAPPA, maxeval=150)
        t_min1 = wall_ms(lambda: fk.minimize_confidence_bound(starts[:1], lo, hi, KAPPA, maxeval=150), a.reps, warmup=0)
        model = E.SurrogateModelGPR(fk, None, None, None, E.YNormalize(1.0, 0.0, "linear"), dtype)
        x0 = X[winner]

        def single_points():
            for _ in range(150):
                model.predict_confidence_bound(x0, KAPPA)

        t_ref = wall_ms(single_points, a.reps)
        rec = dict(part="b" if n == 4096 else "c", n=n, d=d, S=10, maxeval=150, minimize_ms=round(t_min, 3), rounds=int(nevals.max()),
                   evaluations=int(nevals.sum()), minimize_one_run_ms=round(t_min1, 3), one_run_evaluations=int(nevals1[0]),
                   single_point_150_ms=round(t_ref, 3), start_bound=float(cb_train[winner]), best_bound=float(val.min()),
                   one_run_bound=float(val1[0]))
        print(json.dumps(rec), flush=True)
        runs.append(rec)
        fk.release()

    print("\n| m | predict + gradient | kernel + arg-min | kernel / predict | call (timed) | call (untimed) | host: predict_with_gradient | "
          "host: NumPy composition |")
    print("|---|---|---|---|---|---|---|---|")
    for r in calls:
        print(f"| {r['m']} | {r['predict_ms']:.3f} | {r['kernel_ms']:.4f} | {r['kernel_share']:.4f} | {r['call_ms']:.3f} | "
              f"{r['untimed_call_ms']:.3f} | {r['host_predict_grad_ms']:.3f} | {r['host_compose_ms']:.4f} |")
    print("\n| n | 10 runs, maxeval 150 | rounds | evaluations | one run | its evaluations | 150 single-point bounds | bound: start | "
          "best of 10 | one run |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in runs:
        print(f"| {r['n']} | {r['minimize_ms']:.2f} | {r['rounds']} | {r['evaluations']} | {r['minimize_one_run_ms']:.2f} | "
              f"{r['one_run_evaluations']} | {r['single_point_150_ms']:.2f} | {r['start_bound']:.6g} | {r['best_bound']:.6g} | "
              f"{r['one_run_bound']:.6g} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(calls=calls, runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
