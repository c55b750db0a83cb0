"""Times of input warping (hbegp_problem_eval_xgrad, hbegp_problem_eval_warped, hbegp_fit_warped_*) beside the
plain calls.  f64, Matern 5/2:

 (a) the C2 workload (Rosenbrock, d = 8) at n = 4096 and a fixed theta, one single-slot problem: a plain evaluation with its
     gradient, the same with the x-gradient tail (hbegp_problem_eval_xgrad), and a warped evaluation with its p + 2 d gradient
     (hbegp_problem_eval_warped at a, b = 1.5, 0.7: warp, evaluation, tail, chain, restore).  Wall times of the synchronous calls.
 (b) the warped fit beside the plain one on the fit fixture of tests/warp_cases.py (d = 2, a response that is stationary only after
     a warp) at n = 96, 200 and 1024, no restarts, maxeval = 150: FittedKernel.new, then FittedKernel.new_warped started from its
     result (plain=), so that the second time is the warped runs alone.

    python tools/warp_bench.py [--reps 5] [--out FILE]

Prints one JSON object per measurement and two tables at the end (medians of `reps` synchronous calls after a warm-up; part a takes
its five calls in turn, round after round).  There is no pass bar."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import warp_cases as WC  # noqa: E402
from hbetune_rs_amd import gpr, synth  # noqa: E402


def wall_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall))


def big_fit_data(n):
    """warp_cases.fit_data's recipe at any n."""
    rng = np.random.default_rng(n)
    X = rng.uniform(0, 1, (n, 2))
    U = 1.0 - (1.0 - X ** WC.FIT_AB[:2]) ** WC.FIT_AB[2:]
    y = np.sin(6 * U[:, 0]) + np.cos(4 * U[:, 1]) + 0.05 * rng.standard_normal(n)
    return X, (y - y.mean()) / y.std()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    # (a)
    n = 4096
    w = synth.make_workload("C2", n=n)
    X = np.asarray(w["X"], dtype=np.float64)
    X = (X - X.min(axis=0)) / (X.max(axis=0) - X.min(axis=0))  # the warp's domain
    y = np.asarray(w["y"], dtype=np.float64)
    d = X.shape[1]
    theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
    ab = np.concatenate([np.full(d, 1.5), np.full(d, 0.7)])
    prob = gpr.Problem(X, y, nu=2.5)
    calls = dict(eval_ms=lambda: prob.lml_with_gradient(theta),
                 eval_no_grad_ms=lambda: prob.lml_with_gradient(theta, want_grad=False),
                 eval_xgrad_ms=lambda: prob.lml_with_x_gradient(theta),
                 eval_warped_ms=lambda: prob.warped_lml_with_gradient(theta, ab),
                 eval_warped_no_grad_ms=lambda: prob.warped_lml_with_gradient(theta, ab, want_grad=False))
    # the five calls in turn, round after round (three warm-up rounds: graph instantiation, pool blocks, clocks), so that whatever
    # drifts over the run drifts under all of them alike
    walls = {k: [] for k in calls}
    for rnd in range(3 + a.reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if rnd >= 3:
                walls[k].append((time.perf_counter() - t0) * 1e3)
    rec = dict(part="a", n=n, d=d, **{k: round(float(np.median(v)), 4) for k, v in walls.items()})
    rec["xgrad_tail_ms"] = round(rec["eval_xgrad_ms"] - rec["eval_ms"], 4)
    rec["warp_overhead_ms"] = round(rec["eval_warped_ms"] - rec["eval_ms"], 4)
    emit(rec)
    prob.close()

    # (b)
    fits = []
    for n in (96, 200, 1024):
        Xf, yf = WC.fit_data(n) if n in WC.FIT_SIZES else big_fit_data(n)
        args = (Xf, yf, WC.FIT_THETA0, WC.FIT_LO, WC.FIT_HI)
        plain = gpr.FittedKernel.new(*args, nu=WC.FIT_NU)
        t_plain = wall_ms(lambda: gpr.FittedKernel.new(*args, nu=WC.FIT_NU).release(), a.reps, warmup=0)
        wk = gpr.FittedKernel.new_warped(*args, nu=WC.FIT_NU, plain=plain)
        t_warped = wall_ms(lambda: gpr.FittedKernel.new_warped(*args, nu=WC.FIT_NU, plain=plain).release(), a.reps, warmup=0)
        rec = dict(part="b", n=n, d=2, plain_fit_ms=round(t_plain, 3), plain_evaluations=plain.n_evals, plain_lml=round(plain.lml, 4),
                   warped_fit_ms=round(t_warped, 3), warped_evaluations=wk.inner.n_evals, warped_lml=round(wk.lml_best, 4),
                   gain=round(wk.lml_best - plain.lml, 4), a=[round(float(v), 4) for v in wk.warp.a], b=[round(float(v), 4) for v in wk.warp.b])
        emit(rec)
        fits.append(rec)
        wk.release()
        plain.release()

    r = lines[0]
    table = ["", "| n | d | evaluation | without its gradient | + x-gradient tail | the tail | warped evaluation | over the plain one | warped, no gradient |",
             "|---|---|---|---|---|---|---|---|---|",
             f"| {r['n']} | {r['d']} | {r['eval_ms']:.3f} | {r['eval_no_grad_ms']:.3f} | {r['eval_xgrad_ms']:.3f} | {r['xgrad_tail_ms']:.3f} | "
             f"{r['eval_warped_ms']:.3f} | {r['warp_overhead_ms']:.3f} | {r['eval_warped_no_grad_ms']:.3f} |",
             "", "| n | plain fit | its evaluations | lml | warped fit (from the plain optimum) | its evaluations | lml | gain |", "|---|---|---|---|---|---|---|---|"]
    for f in fits:
        table.append(f"| {f['n']} | {f['plain_fit_ms']:.2f} | {f['plain_evaluations']} | {f['plain_lml']:.3f} | {f['warped_fit_ms']:.2f} | "
                     f"{f['warped_evaluations']} | {f['warped_lml']:.3f} | {f['gain']:.3f} |")
    print("\n".join(table))
    if a.out:
        head = ("tools/warp_bench.py on one MI355X: input warping beside the plain calls, f64, Matern 5/2; medians of "
                f"{a.reps} synchronous calls after a warm-up, in ms.\n"
                "part a (C2 workload scaled into [0, 1], n = 4096, d = 8, fixed theta, one single-slot problem): hbegp_problem_eval with its gradient\n"
                "and without; hbegp_problem_eval_xgrad (the same evaluation plus the x-gradient tail; xgrad_tail_ms is the difference);\n"
                "hbegp_problem_eval_warped with its p + 2 d gradient (warp, evaluation, tail, chain, restore) and without a gradient.\n"
                "part b (the fit fixture of tests/warp_cases.py, d = 2, no restarts, maxeval 150): FittedKernel.new, then the warped runs of\n"
                "FittedKernel.new_warped started from that fit's optimum with the identity warp (one run, host-driven, one slot).\n\n")
        with open(a.out, "w") as f:
            f.write(head + "\n".join(json.dumps(rec) for rec in lines) + "\n" + "\n".join(table) + "\n")


if __name__ == "__main__":
    main()
