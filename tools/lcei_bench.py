"""Times of the log-space constrained expected improvement beside the plain-space one: hbegp_log_constrained_ei and
hbegp_constrained_ei in the same process on the same models and candidates, each with its phases split by device events
(hbegp_debug_lcei_phases / hbegp_debug_cei_phases: the 1 + C predicts from the objective's upload to the join of the streams; the
kernel with the arg-max) and the wall time of the whole call.  The shapes are tools/cei_bench.py's: extend() at a fixed theta on the
C2 workload (Rosenbrock, d = 8), n = 4096, one response function per model, f64 and f32; m in {4096, 65536}, C in {1, 4, 8}; the
calls with a gradient on the first 4096 candidates.

    python tools/lcei_bench.py [--reps 5] [--out FILE]

Prints one JSON object per measurement and a table at the end (medians of synchronous calls).  There is no pass bar."""
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

    def timed(fn, hook, reps, warmup=1):
        for _ in range(warmup):
            fn()
        wall, ph = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            hook(1, _lib.dptr(phases))
            ph.append(phases.copy())
        return float(np.median(wall)), np.median(np.array(ph), axis=0)

    n, c_max = 4096, 8
    for dtype in (np.float64, np.float32):
        w = synth.make_workload("C2", n=n)
        X64 = np.asarray(w["X"], dtype=np.float64)
        X = X64.astype(dtype)
        d = X.shape[1]
        ys = [np.asarray(w["y"], dtype=np.float64)]
        for k in range(1, 1 + c_max):  # tools/cei_bench.py's constraints: a bowl around its own centre plus a wave, scaled to mean 1
            g = ((X64 - 0.1 * k) ** 2).sum(axis=1) + np.cos((1.0 + 0.5 * k) * X64[:, k % d])
            ys.append(g / np.abs(g).mean())
        theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
        fks = [gpr.FittedKernel.extend(X, y.astype(dtype), theta, nu=(2.5, 1.5, 0.5, np.inf)[k % 4]) for k, y in enumerate(ys)]
        fmin = float(np.quantile(ys[0], 0.1))
        all_limits = np.array([float(np.median(y)) for y in ys[1:]])
        lib.hbegp_debug_cei_phases(1, None)
        lib.hbegp_debug_lcei_phases(1, None)
        for m in (4096, 65536):
            Xs = synth.candidates("C2", m, d).astype(dtype)
            for n_con in (1, 4, 8):
                obj, cons, limits = fks[0], fks[1:1 + n_con], all_limits[:n_con]
                t_log, pl = timed(lambda: gpr.log_constrained_ei(obj, cons, Xs, fmin, limits), lib.hbegp_debug_lcei_phases, a.reps)
                t_cei, pc = timed(lambda: gpr.constrained_ei(obj, cons, Xs, fmin, limits), lib.hbegp_debug_cei_phases, a.reps)
                t_logg, plg = timed(lambda: gpr.log_constrained_ei(obj, cons, Xs[:4096], fmin, limits, want_grad=True),
                                    lib.hbegp_debug_lcei_phases, a.reps)
                t_ceig, pcg = timed(lambda: gpr.constrained_ei(obj, cons, Xs[:4096], fmin, limits, want_grad=True),
                                    lib.hbegp_debug_cei_phases, a.reps)
                val, best = gpr.log_constrained_ei(obj, cons, Xs, fmin, limits)
                cval, cbest = gpr.constrained_ei(obj, cons, Xs, fmin, limits)
                rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, m=m, C=n_con, predicts_ms=round(float(pl[0]), 4), lcei_ms=round(float(pl[1]), 4),
                           call_ms=round(t_log, 4), cei_predicts_ms=round(float(pc[0]), 4), cei_ms=round(float(pc[1]), 4),
                           cei_call_ms=round(t_cei, 4), ratio=round(float(pl[1] / pc[1]), 2) if pc[1] > 0 else None,
                           grad4096_call_ms=round(t_logg, 4), grad4096_lcei_ms=round(float(plg[1]), 4), grad4096_cei_call_ms=round(t_ceig, 4),
                           grad4096_cei_ms=round(float(pcg[1]), 4), lcei_max=float(val.max()), log_of_cei_max=float(np.log(cval.max())),
                           best=best, cei_best=cbest)
                print(json.dumps(rec), flush=True)
                rows.append(rec)
        lib.hbegp_debug_cei_phases(0, None)
        lib.hbegp_debug_lcei_phases(0, None)
        for fk in fks:
            fk.release()

    print("\n| type | m | C | predicts (first upload .. join) | log kernel + arg-max | call | cEI's predicts | cEI kernel + arg-max | cEI call | "
          "log / cEI kernel phase | with gradient, m = 4096: log kernel | cEI kernel |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['dtype']} | {r['m']} | {r['C']} | {r['predicts_ms']:.3f} | {r['lcei_ms']:.3f} | {r['call_ms']:.3f} | {r['cei_predicts_ms']:.3f} | "
              f"{r['cei_ms']:.3f} | {r['cei_call_ms']:.3f} | {r['ratio']} | {r['grad4096_lcei_ms']:.3f} | {r['grad4096_cei_ms']:.3f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
