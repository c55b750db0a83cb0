"""Times of the Monte Carlo batch expected improvement on one model: hbegp_qei with its gradient, the phases split by device events
(hbegp_debug_qei_phases: the shared launches -- upload, Kstar, mean, Q, dmean, G, W = G X^T, z -- and the qEI kernel) and the wall
time of the whole call.  Models: extend() at a fixed theta on the C2 workload (Rosenbrock, d = 8), n = 1024 and 4096, f64 and f32;
q in {4, 10, 32}, B in {1, 64, 256}, S in {256, 2048}.  Then the maximiser: R = 16 runs of q = 10 at n = 256 and 1024 (rounds,
evaluations, time).

    python tools/qei_bench.py [--reps 3] [--out FILE]

Prints one JSON object per measurement and tables at the end (medians of synchronous calls)."""
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


def _model(n, dtype):
    w = synth.make_workload("C2", n=n)
    X, y = w["X"].astype(dtype), w["y"].astype(dtype)
    d = X.shape[1]
    theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
    return gpr.FittedKernel.extend(X, y, theta, nu=2.5), float(np.min(y)), d, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    rows, mrows = [], []
    phases = np.zeros(2)

    def timed(fn, reps, warmup=1):
        for _ in range(warmup):
            fn()
        wall, ph = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            lib.hbegp_debug_qei_phases(1, _lib.dptr(phases))
            ph.append(phases.copy())
        return float(np.median(wall)), np.median(np.array(ph), axis=0)

    rng = np.random.default_rng(0)
    for n in (1024, 4096):
        for dtype in (np.float64, np.float32):
            fk, fmin, d, w = _model(n, dtype)
            lib.hbegp_debug_qei_phases(1, None)
            for q in (4, 10, 32):
                for B in (1, 64, 256):
                    Xb = synth.candidates("C2", B * q, d).astype(dtype).reshape(B, q, d)
                    for S in (256, 2048):
                        z = rng.standard_normal((S, q)).astype(dtype)
                        t_call, ph = timed(lambda: fk.qei(Xb, z, fmin), a.reps)
                        # what the qEI kernel reads per batch: Q rows (q (q + 1) / 2 dots) and the W rows (q d, each against q Q rows)
                        kb = np.dtype(dtype).itemsize * B * fk.n * (q * (q + 1) / 2 + 2.0 * q * d * q)
                        rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, q=q, B=B, S=S, shared_ms=round(float(ph[0]), 4),
                                   qei_ms=round(float(ph[1]), 4), device_ms=round(float(ph.sum()), 4), call_ms=round(t_call, 4),
                                   kernel_reads_mb=round(kb / 1e6, 1))
                        print(json.dumps(rec), flush=True)
                        rows.append(rec)
            lib.hbegp_debug_qei_phases(0, None)
            fk.release()

    for n in (256, 1024):
        for dtype in (np.float64, np.float32):
            fk, fmin, d, w = _model(n, dtype)
            lo, hi = w["X"].min(axis=0).astype(np.float64), w["X"].max(axis=0).astype(np.float64)  # the box of the training points
            starts = (lo + (hi - lo) * rng.uniform(0, 1, (16, 10, d))).astype(dtype)
            z = rng.standard_normal((512, 10)).astype(dtype)
            fmed = float(np.median(w["y"]))  # half the training values improve on it: the ascents have a slope to follow
            fk.maximize_qei(starts, lo, hi, z, fmed, maxeval=20)  # warm-up
            t0 = time.perf_counter()
            x, v, ne = fk.maximize_qei(starts, lo, hi, z, fmed, maxeval=150)
            ms = (time.perf_counter() - t0) * 1e3
            rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, R=16, q=10, S=512, rounds=int(ne.max()), evals=int(ne.sum()),
                       ms=round(ms, 2), ms_per_round=round(ms / max(1, int(ne.max())), 3), qei_best=float(v.max()))
            print(json.dumps(rec), flush=True)
            mrows.append(rec)
            fk.release()

    print("\n| n | type | q | B | S | shared | qEI kernel | device total | call |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['dtype']} | {r['q']} | {r['B']} | {r['S']} | {r['shared_ms']:.3f} | {r['qei_ms']:.3f} | "
              f"{r['device_ms']:.3f} | {r['call_ms']:.3f} |")
    print("\n| n | type | R | q | S | rounds | evaluations | ms | ms / round |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in mrows:
        print(f"| {r['n']} | {r['dtype']} | {r['R']} | {r['q']} | {r['S']} | {r['rounds']} | {r['evals']} | {r['ms']:.1f} | "
              f"{r['ms_per_round']:.3f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(qei=rows, maximize=mrows), f, indent=1)


if __name__ == "__main__":
    main()
