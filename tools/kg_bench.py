"""Times of the knowledge gradient over a candidate set on one model: hbegp_knowledge_gradient with the phases split by device
events (hbegp_debug_kg_phases: Sigma, kg) and the wall time of the whole call (mc doubles and two ints back).  Models: extend()
at a fixed theta on the C2 workload (Rosenbrock, d = 8), n = 1024 and 4096, f64 and f32; m in {64, 512, 2048, 8192}, mc = m.

    python tools/kg_bench.py [--reps 5] [--out FILE]

Prints one JSON object per measurement and a table at the end (medians of synchronous calls).  lines_per_us: m * mc lines
sorted and scanned per microsecond of the kg phase."""
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
            lib.hbegp_debug_kg_phases(1, _lib.dptr(phases))
            ph.append(phases.copy())
        return float(np.median(wall)), np.median(np.array(ph), axis=0)

    for n in (1024, 4096):
        for dtype in (np.float64, np.float32):
            w = synth.make_workload("C2", n=n)
            X, y = w["X"].astype(dtype), w["y"].astype(dtype)
            d = X.shape[1]
            theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
            fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
            lib.hbegp_debug_kg_phases(1, None)
            for m in (64, 512, 2048, 8192):
                Xs = synth.candidates("C2", m, d).astype(dtype)
                t_call, ph = timed(lambda: fk.knowledge_gradient(Xs), a.reps)
                kg, best, imin = fk.knowledge_gradient(Xs)
                rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, m=m, mc=m, sigma_ms=round(float(ph[0]), 4), kg_ms=round(float(ph[1]), 4),
                           device_ms=round(float(ph.sum()), 4), call_ms=round(t_call, 4),
                           lines_per_us=round(m * m / (ph[1] * 1e3), 1) if ph[1] > 0 else None, kg_max=float(kg.max()), best=best,
                           imin=imin)
                print(json.dumps(rec), flush=True)
                rows.append(rec)
            lib.hbegp_debug_kg_phases(0, None)
            fk.release()

    print("\n| n | type | m = mc | Sigma | kg | device total | call | lines / us |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['dtype']} | {r['m']} | {r['sigma_ms']:.3f} | {r['kg_ms']:.3f} | {r['device_ms']:.3f} | {r['call_ms']:.3f} | "
              f"{r['lines_per_us']} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
