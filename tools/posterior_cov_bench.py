"""Times of the joint posterior on one model: hbegp_sample_posterior with the phases split by device events
(hbegp_debug_posterior_phases: Q, Sigma, factor, draws), the wall time of the argmin-only call (S ints back) and of
predict_cov (Sigma copied out).  Models: extend() at a fixed theta on the C2 workload (Rosenbrock, d = 8), n = 1024 and 4096,
f64 and f32; m in {64, 512, 2048, 8192}, S in {1, 256}.

    python tools/posterior_cov_bench.py [--reps 5] [--out FILE]

Prints one JSON object per measurement and a table at the end (medians of synchronous calls)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hbetune_rs_amd import _lib  # noqa: E402
from hbetune_rs_amd import estimator as E  # noqa: E402
from hbetune_rs_amd import gpr, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    rows = []
    phases = np.zeros(4)

    def timed(fn, reps, warmup=1):
        for _ in range(warmup):
            fn()
        wall, ph = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            lib.hbegp_debug_posterior_phases(1, _lib.dptr(phases))
            ph.append(phases.copy())
        return float(np.median(wall)), np.median(np.array(ph), axis=0)

    for n in (1024, 4096):
        for dtype in (np.float64, np.float32):
            w = synth.make_workload("C2", n=n)
            X, y = w["X"].astype(dtype), w["y"].astype(dtype)
            d = X.shape[1]
            theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
            fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
            lib.hbegp_debug_posterior_phases(1, None)
            for m in (64, 512, 2048, 8192):
                Xs = synth.candidates("C2", m, d).astype(dtype)
                t_cov, _ = timed(lambda: fk.predict_cov(Xs), a.reps)
                for S in (1, 256):
                    z = E.RNG(S).standard_normal((S, m)).astype(dtype)
                    t_arg, ph = timed(lambda: fk.sample_posterior(Xs, z, want_samples=False), a.reps)
                    t_smp, _ = timed(lambda: fk.sample_posterior(Xs, z), a.reps)
                    rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, m=m, S=S, q_ms=round(ph[0], 4), sigma_ms=round(ph[1], 4),
                               factor_ms=round(ph[2], 4), draws_ms=round(ph[3], 4), device_ms=round(float(ph.sum()), 4),
                               argmin_call_ms=round(t_arg, 4), samples_call_ms=round(t_smp, 4), predict_cov_call_ms=round(t_cov, 4))
                    print(json.dumps(rec), flush=True)
                    rows.append(rec)
            lib.hbegp_debug_posterior_phases(0, None)
            fk.release()

    print("\n| n | type | m | S | Q | Sigma | factor | draws | device total | argmin call | samples call | predict_cov call |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['dtype']} | {r['m']} | {r['S']} | {r['q_ms']:.3f} | {r['sigma_ms']:.3f} | {r['factor_ms']:.3f} | "
              f"{r['draws_ms']:.3f} | {r['device_ms']:.3f} | {r['argmin_call_ms']:.3f} | {r['samples_call_ms']:.3f} | "
              f"{r['predict_cov_call_ms']:.3f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
