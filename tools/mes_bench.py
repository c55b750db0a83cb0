"""Times of max-value entropy search: hbegp_mes with its phases split by device events (hbegp_debug_mes_phases: the predict from
the uploads to its last launch -- with a gradient the gradient's launches too; the MES kernel with the arg-max) and the wall time
of the whole call, beside the same values computed on the host with NumPy / scipy (tests/mes_ref.py) from predict_with_gradient's
outputs.  extend() at a fixed theta on the C2 workload (Rosenbrock, d = 8), n = 4096, f64 and f32; m in {256, 4096},
S in {64, 1024}, with and without a gradient; y* spread below the lowest training target.

    python tools/mes_bench.py [--reps 5] [--out FILE]

Prints one JSON object per measurement and a table at the end (medians of synchronous calls).  There is no pass bar."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mes_ref  # noqa: E402
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
            lib.hbegp_debug_mes_phases(1, _lib.dptr(phases))
            ph.append(phases.copy())
        return float(np.median(wall)), np.median(np.array(ph), axis=0)

    def host_ms(fn, reps):
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(wall))

    n = 4096
    for dtype in (np.float64, np.float32):
        w = synth.make_workload("C2", n=n)
        X = np.asarray(w["X"], dtype=np.float64).astype(dtype)
        y = np.asarray(w["y"], dtype=np.float64)
        d = X.shape[1]
        theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
        fk = gpr.FittedKernel.extend(X, y.astype(dtype), theta, nu=2.5)
        lib.hbegp_debug_mes_phases(1, None)
        for m in (256, 4096):
            Xs = synth.candidates("C2", m, d).astype(dtype)
            mean, var, dmean, dvar, _ = fk.predict_with_gradient(Xs)
            for S in (64, 1024):
                ys = y.min() - y.std() * np.linspace(0.0, 1.0, S)
                t_val, pv = timed(lambda: fk.mes(Xs, ys), a.reps)
                t_grad, pg = timed(lambda: fk.mes(Xs, ys, want_grad=True), a.reps)
                h_val = host_ms(lambda: mes_ref.mes(mean, var, ys), a.reps)
                h_grad = host_ms(lambda: mes_ref.mes_grad_x(mean, var, dmean, dvar, ys), a.reps)
                val, best, grad = fk.mes(Xs, ys, want_grad=True)
                rv, rg, _ = mes_ref.mes_grad_x(mean, var, dmean, dvar, ys)
                rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, m=m, S=S, predict_ms=round(float(pv[0]), 4), mes_ms=round(float(pv[1]), 4),
                           call_ms=round(t_val, 4), host_mes_ms=round(h_val, 4), grad_predict_ms=round(float(pg[0]), 4),
                           grad_mes_ms=round(float(pg[1]), 4), grad_call_ms=round(t_grad, 4), host_grad_mes_ms=round(h_grad, 4),
                           mes_max=float(val.max()), best=best, dev_value=float(np.abs(val - rv).max()),
                           dev_grad=float(np.abs(grad.astype(np.float64) - rg).max()))
                print(json.dumps(rec), flush=True)
                rows.append(rec)
        lib.hbegp_debug_mes_phases(0, None)
        fk.release()

    print("\n| type | m | S | predict | MES kernel + arg-max | call | host MES (NumPy) | with gradient: predict | MES kernel + arg-max | call | "
          "host MES (NumPy) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['dtype']} | {r['m']} | {r['S']} | {r['predict_ms']:.3f} | {r['mes_ms']:.3f} | {r['call_ms']:.3f} | {r['host_mes_ms']:.3f} | "
              f"{r['grad_predict_ms']:.3f} | {r['grad_mes_ms']:.3f} | {r['grad_call_ms']:.3f} | {r['host_grad_mes_ms']:.3f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
