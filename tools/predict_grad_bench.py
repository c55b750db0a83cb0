"""Times of predict and predict_with_gradient on one model (wall-clock medians of synchronous calls), and of maximize_ei
end to end.  Models: extend() at a fixed theta on the C2 workload (Rosenbrock, d = 8), n = 1024 and 4096, f64 and f32.

    python tools/predict_grad_bench.py [--reps 7] [--out FILE]

Prints one JSON object per measurement and a table at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hbetune_rs_amd import estimator as E  # noqa: E402
from hbetune_rs_amd import gpr, synth  # noqa: E402


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        rows.append(rec)

    for n in (1024, 4096):
        for dtype in (np.float64, np.float32):
            w = synth.make_workload("C2", n=n)
            X, y = w["X"].astype(dtype), w["y"].astype(dtype)
            d = X.shape[1]
            theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
            fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
            for m in (1, 8, 64, 256, 1600):
                Xs = synth.candidates("C2", m, d).astype(dtype)
                t_pred = median_ms(lambda: fk.predict(Xs), a.reps)
                t_grad = median_ms(lambda: fk.predict_with_gradient(Xs), a.reps)
                t_gmean = median_ms(lambda: fk.predict_with_gradient(Xs, want_variance=False), a.reps)
                emit(dict(kind="predict", n=n, d=d, dtype=np.dtype(dtype).name, m=m, predict_ms=round(t_pred, 4),
                          predict_grad_ms=round(t_grad, 4), predict_grad_mean_only_ms=round(t_gmean, 4)))
            fk.release()

    # maximize_ei: S = 64 starts at n = 1024 on a fitted estimator model
    for dtype in (np.float64, np.float32):
        w = synth.make_workload("C2", n=1024)
        X, y = w["X"].astype(dtype), w["y"].astype(dtype)
        d = X.shape[1]
        model = E.EstimatorGPR.new(d).estimate(X, y, None, E.RNG.new_with_seed(1))
        starts = np.random.default_rng(0).uniform(0, 1, (64, d)).astype(dtype)
        bounds = [(0.0, 1.0)] * d
        fmin = float(y.min())
        model.maximize_ei(starts, bounds, fmin)  # warm-up (scratch allocation)
        t0 = time.perf_counter()
        x, ei, nevals = model.maximize_ei(starts, bounds, fmin)
        t = (time.perf_counter() - t0) * 1e3
        emit(dict(kind="maximize_ei", n=1024, d=d, dtype=np.dtype(dtype).name, S=64, rounds=int(nevals.max()),
                  evaluations=int(nevals.sum()), ms=round(t, 2), ms_per_round=round(t / max(1, int(nevals.max())), 4),
                  best_ei=float(ei.max())))

    print("\n  n     dtype    m     predict ms  grad ms  grad(mean only) ms")
    for r in rows:
        if r["kind"] == "predict":
            print(f"  {r['n']:<5} {r['dtype']:<8} {r['m']:<5} {r['predict_ms']:>10.3f} {r['predict_grad_ms']:>8.3f} "
                  f"{r['predict_grad_mean_only_ms']:>10.3f}")
    for r in rows:
        if r["kind"] == "maximize_ei":
            print(f"  maximize_ei {r['dtype']} n=1024 S=64: {r['rounds']} rounds, {r['evaluations']} evaluations, "
                  f"{r['ms']:.1f} ms ({r['ms_per_round']:.3f} ms per round)")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
