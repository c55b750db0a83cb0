"""Times of the constrained expected improvement over a candidate set: hbegp_constrained_ei with the phases split by device events
(hbegp_debug_cei_phases: the 1 + C predicts, each on its model's stream, from the objective's upload to the join; the cEI kernel
with the arg-max), the wall time of the whole call, and the wall time of the same numbers obtained the old way -- 1 + C predict()
calls and the NumPy restatement (tests/cei_ref.py) on the host.  Models: extend() at a fixed theta on the C2 workload (Rosenbrock,
d = 8), n = 4096, one response function per model, f64 and f32; m in {4096, 65536}, C in {1, 4, 8}.

    python tools/cei_bench.py [--reps 5] [--out FILE] [--no-host]

Prints one JSON object per measurement and a table at the end (medians of synchronous calls)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cei_ref  # noqa: E402
from hbetune_rs_amd import _lib  # noqa: E402
from hbetune_rs_amd import gpr, synth  # noqa: E402


def host_cei(fks, Xs, fmin, limits):
    """What a caller did before hbegp_constrained_ei: every posterior back to the host, then EI times the feasibility
    probabilities in NumPy."""
    pm = [fk.predict(Xs) for fk in fks]
    mu = np.stack([p[0] for p in pm], axis=1).astype(np.float64)
    var = np.stack([p[1] for p in pm], axis=1).astype(np.float64)
    return cei_ref.cei(mu, var, fmin, limits)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the predicts-plus-NumPy timing")
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
            lib.hbegp_debug_cei_phases(1, _lib.dptr(phases))
            ph.append(phases.copy())
        return float(np.median(wall)), np.median(np.array(ph), axis=0)

    n, c_max = 4096, 8
    for dtype in (np.float64, np.float32):
        w = synth.make_workload("C2", n=n)
        X64 = np.asarray(w["X"], dtype=np.float64)
        X = X64.astype(dtype)
        d = X.shape[1]
        ys = [np.asarray(w["y"], dtype=np.float64)]
        for k in range(1, 1 + c_max):  # constraint k: a bowl around its own centre plus a wave, scaled to mean 1
            g = ((X64 - 0.1 * k) ** 2).sum(axis=1) + np.cos((1.0 + 0.5 * k) * X64[:, k % d])
            ys.append(g / np.abs(g).mean())
        theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
        fks = [gpr.FittedKernel.extend(X, y.astype(dtype), theta, nu=(2.5, 1.5, 0.5, np.inf)[k % 4]) for k, y in enumerate(ys)]
        fmin = float(np.quantile(ys[0], 0.1))
        all_limits = np.array([float(np.median(y)) for y in ys[1:]])
        lib.hbegp_debug_cei_phases(1, None)
        for m in (4096, 65536):
            Xs = synth.candidates("C2", m, d).astype(dtype)
            for n_con in (1, 4, 8):
                obj, cons, limits = fks[0], fks[1:1 + n_con], all_limits[:n_con]
                t_call, ph = timed(lambda: gpr.constrained_ei(obj, cons, Xs, fmin, limits), a.reps)
                t_grad, phg = timed(lambda: gpr.constrained_ei(obj, cons, Xs[:4096], fmin, limits, want_grad=True), a.reps)
                val, best = gpr.constrained_ei(obj, cons, Xs, fmin, limits)
                rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, m=m, C=n_con, predicts_ms=round(float(ph[0]), 4), cei_ms=round(float(ph[1]), 4),
                           call_ms=round(t_call, 4), rows_per_us=round(m / (ph[1] * 1e3), 1) if ph[1] > 0 else None,
                           grad4096_call_ms=round(t_grad, 4), grad4096_predicts_ms=round(float(phg[0]), 4),
                           grad4096_cei_ms=round(float(phg[1]), 4), cei_max=float(val.max()), best=best)
                if not a.no_host:
                    t0 = time.perf_counter()
                    hv = host_cei(fks[:1 + n_con], Xs, fmin, limits)
                    rec["host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                    rec["host_max_dev"] = float(np.abs(hv - val).max())
                print(json.dumps(rec), flush=True)
                rows.append(rec)
        lib.hbegp_debug_cei_phases(0, None)
        for fk in fks:
            fk.release()

    print("\n| type | m | C | predicts (first upload .. join) | cEI kernel + arg-max | call | rows / us | 1 + C predicts + NumPy | "
          "call with gradient, m = 4096 | its predicts | its cEI kernel |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['dtype']} | {r['m']} | {r['C']} | {r['predicts_ms']:.3f} | {r['cei_ms']:.3f} | {r['call_ms']:.3f} | {r['rows_per_us']} | "
              f"{r.get('host_ms', '-')} | {r['grad4096_call_ms']:.3f} | {r['grad4096_predicts_ms']:.3f} | {r['grad4096_cei_ms']:.3f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
