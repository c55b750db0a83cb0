"""Times of the greedy batch selection on one model: hbegp_select_batch with the phases split by device events
(hbegp_debug_batch_select_phases: Sigma, select) and the wall time of the whole call (k ints and k doubles back).  Models:
extend() at a fixed theta on the C2 workload (Rosenbrock, d = 8), n = 1024 and 4096, f64 and f32; m in {64, 512, 2048, 8192},
k in {1, 16, 64} (kriging believer).

    python tools/batch_select_bench.py [--reps 5] [--out FILE]

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
from hbetune_rs_amd import gpr, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    rows = []
    phases = np.zeros(2)

    def timed(fn, reps, warmup=1):
        for _ in range(warmup):
            fn()
        wall, ph = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            lib.hbegp_debug_batch_select_phases(1, _lib.dptr(phases))
            ph.append(phases.copy())
        return float(np.median(wall)), np.median(np.array(ph), axis=0)

    for n in (1024, 4096):
        for dtype in (np.float64, np.float32):
            w = synth.make_workload("C2", n=n)
            X, y = w["X"].astype(dtype), w["y"].astype(dtype)
            d = X.shape[1]
            theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
            fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
            fmin = float(np.min(y))
            lib.hbegp_debug_batch_select_phases(1, None)
            for m in (64, 512, 2048, 8192):
                Xs = synth.candidates("C2", m, d).astype(dtype)
                for k in (1, 16, 64):
                    t_call, ph = timed(lambda: fk.select_batch(Xs, k, fmin), a.reps)
                    # what the select kernel reads of C: sum over steps of t m fp64 values, plus row j of Sigma per step
                    c_bytes = 8.0 * m * k * (k - 1) / 2 + np.dtype(dtype).itemsize * m * k
                    rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, m=m, k=k, sigma_ms=round(float(ph[0]), 4),
                               select_ms=round(float(ph[1]), 4), device_ms=round(float(ph.sum()), 4), call_ms=round(t_call, 4),
                               select_read_mb=round(c_bytes / 1e6, 2),
                               select_gbps=round(c_bytes / (ph[1] * 1e-3) / 1e9, 1) if ph[1] > 0 else None)
                    print(json.dumps(rec), flush=True)
                    rows.append(rec)
            lib.hbegp_debug_batch_select_phases(0, None)
            fk.release()

    print("\n| n | type | m | k | Sigma | select | device total | call | select reads (MB) | GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['dtype']} | {r['m']} | {r['k']} | {r['sigma_ms']:.3f} | {r['select_ms']:.3f} | {r['device_ms']:.3f} | "
              f"{r['call_ms']:.3f} | {r['select_read_mb']} | {r['select_gbps']} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
