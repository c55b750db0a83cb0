"""Times of the two-objective expected hypervolume improvement over a candidate set: hbegp_ehvi with the phases split by device
events (hbegp_debug_ehvi_phases: the two predicts, each on its model's stream, and the EHVI kernel), the wall time of the whole
call, and the wall time of the same numbers obtained the old way -- two predict() calls and the NumPy restatement
(tests/ehvi_ref.py) on the host.  Models: extend() at a fixed theta on the C2 workload (Rosenbrock, d = 8), n = 4096, two
response functions, f64 and f32; m in {4096, 65536}, P in {16, 256, 2048} (a convex front, every point non-dominated).

    python tools/ehvi_bench.py [--reps 5] [--out FILE] [--no-host]

Prints one JSON object per measurement and a table at the end (medians of synchronous calls).  strips_per_us: m * (P + 1) strips
per microsecond of the EHVI phase; each strip is two evaluations of (G, Phi, phi): one erfc and one exp each."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ehvi_ref  # noqa: E402
from hbetune_rs_amd import _lib  # noqa: E402
from hbetune_rs_amd import gpr, synth  # noqa: E402


def host_ehvi(fks, Xs, front, ref, rows=4096):
    """What a caller did before hbegp_ehvi: both posteriors back to the host, then the Pareto arithmetic in NumPy (in slabs of rows:
    the restatement holds [rows, P + 1] arrays)."""
    pm = [fk.predict(Xs) for fk in fks]
    mu = np.stack([pm[0][0], pm[1][0]], axis=1).astype(np.float64)
    var = np.stack([pm[0][1], pm[1][1]], axis=1).astype(np.float64)
    return np.concatenate([ehvi_ref.ehvi(mu[r:r + rows], var[r:r + rows], front, ref)[0] for r in range(0, len(Xs), rows)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the two-predicts-plus-NumPy timing")
    a = ap.parse_args()
    lib = _lib.load()
    rows = []
    phases = np.zeros(3)

    def timed(fn, reps, warmup=1):
        for _ in range(warmup):
            fn()
        wall, ph = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            lib.hbegp_debug_ehvi_phases(1, _lib.dptr(phases))
            ph.append(phases.copy())
        return float(np.median(wall)), np.median(np.array(ph), axis=0)

    n = 4096
    for dtype in (np.float64, np.float32):
        w = synth.make_workload("C2", n=n)
        X = w["X"].astype(dtype)
        d = X.shape[1]
        y0 = np.asarray(w["y"], dtype=np.float64)
        y1 = ((np.asarray(w["X"], dtype=np.float64) - 0.3) ** 2).sum(axis=1)
        y1 = y1 / y1.mean()
        theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
        fks = [gpr.FittedKernel.extend(X, y.astype(dtype), theta, nu=nu) for y, nu in ((y0, 2.5), (y1, 1.5))]
        lo = np.array([y0.min(), y1.min()])
        hi = np.array([y0.max(), y1.max()])
        ref = hi + 0.1 * (hi - lo)
        lib.hbegp_debug_ehvi_phases(1, None)
        for m in (4096, 65536):
            Xs = synth.candidates("C2", m, d).astype(dtype)
            for P in (16, 256, 2048):
                t = np.arange(P) / P
                front = np.stack([lo[0] + (hi[0] - lo[0]) * t, lo[1] + (hi[1] - lo[1]) * (1 - np.sqrt(t)) ** 2], axis=1)
                t_call, ph = timed(lambda: gpr.ehvi(fks, Xs, front, ref), a.reps)
                t_grad, phg = timed(lambda: gpr.ehvi(fks, Xs[:4096], front, ref, want_grad=True), a.reps)
                val, best = gpr.ehvi(fks, Xs, front, ref)
                rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, m=m, P=P, predict0_ms=round(float(ph[0]), 4), predict1_ms=round(float(ph[1]), 4),
                           ehvi_ms=round(float(ph[2]), 4), call_ms=round(t_call, 4),
                           strips_per_us=round(m * (P + 1) / (ph[2] * 1e3), 1) if ph[2] > 0 else None,
                           grad4096_call_ms=round(t_grad, 4), grad4096_ehvi_ms=round(float(phg[2]), 4), ehvi_max=float(val.max()), best=best)
                if not a.no_host:
                    t0 = time.perf_counter()
                    hv = host_ehvi(fks, Xs, front, ref)
                    rec["host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                    rec["host_max_dev"] = float(np.abs(hv - val).max())
                print(json.dumps(rec), flush=True)
                rows.append(rec)
        lib.hbegp_debug_ehvi_phases(0, None)
        for fk in fks:
            fk.release()

    print("\n| type | m | P | predict 0 | predict 1 | EHVI kernel | call | strips / us | two predicts + NumPy | call with gradient, m = 4096 |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['dtype']} | {r['m']} | {r['P']} | {r['predict0_ms']:.3f} | {r['predict1_ms']:.3f} | {r['ehvi_ms']:.3f} | {r['call_ms']:.3f} | "
              f"{r['strips_per_us']} | {r.get('host_ms', '-')} | {r['grad4096_call_ms']:.3f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
