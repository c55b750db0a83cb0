"""Times of the sensitivity queries on one model: hbegp_sobol (N = 4096) and hbegp_main_effects (N = 512, G = 32) with the
phases split by device events (hbegp_debug_sens_phases: upload, substituted means, chunk and row sums, reduction and download)
and the wall time of the whole call, next to the MATERIALISED route on the same model in the same run: build the query matrix on
the host, FittedKernel.predict(want_variance=False), reduce in NumPy -- what a user could do without these entry points.
Model: extend() at a fixed theta on the C2 workload (Rosenbrock, d = 8), n = 4096, f64, nu = 2.5.

    python tools/sens_bench.py [--reps 5] [--n 4096] [--out FILE]

Prints one JSON object per measurement (medians of synchronous calls after a warm-up, in ms) and a table at the end."""
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


def pick_freeze(A, B):
    d = A.shape[1]
    AB = np.repeat(A[None], d, axis=0)
    for k in range(d):
        AB[k, :, k] = B[:, k]
    return AB


def sobol_materialised(fk, A, B):
    N, d = A.shape
    pts = np.concatenate([A, B, pick_freeze(A, B).reshape(d * N, d)])
    f, _, _ = fk.predict(pts, want_variance=False)
    f_a, f_b, f_ab = f[:N], f[N:2 * N], f[2 * N:].reshape(d, N)
    both = f[:2 * N]
    f0 = both.mean()
    V = ((both - f0) ** 2).mean()
    first = ((f_b - f0)[None, :] * (f_ab - f_a[None, :])).sum(axis=1) / N / V
    total = ((f_a[None, :] - f_ab) ** 2).sum(axis=1) / (2.0 * N) / V
    return first, total, f0, V


def effects_materialised(fk, A, grid):
    N, d = A.shape
    G = grid.shape[1]
    pts = np.repeat(A[None], d * G, axis=0).reshape(d, G, N, d)
    for k in range(d):
        pts[k, :, :, k] = grid[k][:, None]
    f, _, _ = fk.predict(pts.reshape(d * G * N, d), want_variance=False)
    return f.reshape(d, G, N).mean(axis=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    phases = np.zeros(4)

    def timed(fn, reps, warmup=1, want_phases=False):
        for _ in range(warmup):
            fn()
        wall, ph = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            if want_phases:
                lib.hbegp_debug_sens_phases(1, _lib.dptr(phases))
                ph.append(phases.copy())
        return float(np.median(wall)), (np.median(np.array(ph), axis=0) if want_phases else None)

    dtype = np.float64
    w = synth.make_workload("C2", n=a.n)
    X, y = w["X"].astype(dtype), w["y"].astype(dtype)
    d = X.shape[1]
    theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
    fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
    lo, hi = X.min(axis=0), X.max(axis=0)
    rng = np.random.default_rng(1)
    rows = []

    def record(what, N, G, fused, mat, check):
        lib.hbegp_debug_sens_phases(1, None)
        t_call, ph = timed(fused, a.reps, want_phases=True)
        lib.hbegp_debug_sens_phases(0, None)
        t_mat, _ = timed(mat, a.reps)
        rec = dict(what=what, n=a.n, d=d, dtype=np.dtype(dtype).name, N=N, G=G, upload_ms=round(float(ph[0]), 4),
                   means_ms=round(float(ph[1]), 4), sums_ms=round(float(ph[2]), 4), reduce_ms=round(float(ph[3]), 4),
                   device_ms=round(float(ph.sum()), 4), call_ms=round(t_call, 4), materialised_ms=round(t_mat, 4),
                   ratio=round(t_mat / t_call, 2), max_difference=float(check()))
        print(json.dumps(rec), flush=True)
        rows.append(rec)

    N = 4096
    A = (lo + (hi - lo) * rng.uniform(0, 1, (N, d))).astype(dtype)
    B = (lo + (hi - lo) * rng.uniform(0, 1, (N, d))).astype(dtype)

    def sobol_check():
        f1, t1, _, _ = fk.sobol_indices(A, B)
        f2, t2, _, _ = sobol_materialised(fk, A, B)
        return max(np.abs(f1 - f2).max(), np.abs(t1 - t2).max())
    record("sobol", N, 0, lambda: fk.sobol_indices(A, B), lambda: sobol_materialised(fk, A, B), sobol_check)

    N, G = 512, 32
    A2 = A[:N]
    grid = (lo[:, None] + (hi - lo)[:, None] * ((np.arange(G) + 0.5) / G)[None, :]).astype(dtype)
    record("main_effects", N, G, lambda: fk.main_effects(A2, grid), lambda: effects_materialised(fk, A2, grid),
           lambda: np.abs(fk.main_effects(A2, grid) - effects_materialised(fk, A2, grid)).max())
    fk.release()

    print("\n| call | N | G | upload | means | sums | reduce | device total | call | materialised | materialised / call |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['what']} | {r['N']} | {r['G']} | {r['upload_ms']:.3f} | {r['means_ms']:.3f} | {r['sums_ms']:.3f} | {r['reduce_ms']:.3f} | "
              f"{r['device_ms']:.3f} | {r['call_ms']:.3f} | {r['materialised_ms']:.3f} | {r['ratio']:.2f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
