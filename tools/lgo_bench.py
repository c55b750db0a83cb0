"""Cost of a leave-group-out evaluation next to a leave-one-out evaluation, on the same build and the same slot.

On the workload of a config (default M: n = 4096, d = 8) at its reference theta, for f64 and f32 and for consecutive groups of 1, 8
and 64 rows: hbegp_problem_eval_loo with gradient and hbegp_problem_eval_lgo with gradient on ONE slot of ONE problem, alternating,
after a warm-up of both; wall-clock medians of the synchronous calls.  Then the four phases of the leave-group-out tail from device
events (hbegp_debug_lgo_phases) -- the group pass, u and Y, the SYRK C = Y Y^T, the weighted trace -- beside leave-one-out's
(hbegp_debug_loo_phases): the SYRK and the trace are the same launches, the difference is the group pass plus the Y pass.

    python tools/lgo_bench.py [--config M] [--n N] [--reps 15] [--sizes 1,8,64] [--out FILE]

Prints one JSON object per (element type, group size) and writes them all to --out."""
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

NAMES = ("first_pass", "u_and_Y", "syrk", "trace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="M")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sizes", default="1,8,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    w = synth.make_workload(a.config) if a.n is None else synth.make_workload(a.config, n=a.n)
    rows = []
    for dtype in (np.float64, np.float32):
        X, y, theta = w["X"].astype(dtype), w["y"].astype(dtype), w["theta"]
        n, d = X.shape
        prob = gpr.Problem(X, y)
        for size in [int(v) for v in a.sizes.split(",")]:
            groups = (np.arange(n) // size).astype(np.int32)
            for _ in range(2):  # warm-up of both
                loo, _ = prob.loo_with_gradient(theta)
                lgo, _ = prob.lgo_with_gradient(theta, groups)
            t_loo, t_lgo = [], []
            ph, acc_loo, acc_lgo = np.zeros(4), np.zeros(4), np.zeros(4)
            lib.hbegp_debug_loo_phases(1, None)
            lib.hbegp_debug_lgo_phases(1, None)
            for _ in range(a.reps):  # alternating
                t0 = time.perf_counter()
                prob.loo_with_gradient(theta)
                t1 = time.perf_counter()
                prob.lgo_with_gradient(theta, groups)
                t2 = time.perf_counter()
                t_loo.append((t1 - t0) * 1e3)
                t_lgo.append((t2 - t1) * 1e3)
                lib.hbegp_debug_loo_phases(1, _lib.dptr(ph))
                acc_loo += ph
                lib.hbegp_debug_lgo_phases(1, _lib.dptr(ph))
                acc_lgo += ph
            lib.hbegp_debug_loo_phases(0, None)
            lib.hbegp_debug_lgo_phases(0, None)
            med = lambda v: float(np.median(v))  # noqa: E731
            row = {"config": a.config, "n": n, "d": d, "dtype": np.dtype(dtype).name, "group_size": size, "reps": a.reps,
                   "loo": loo, "lgo": lgo, "eval_loo_grad_ms": round(med(t_loo), 4), "eval_lgo_grad_ms": round(med(t_lgo), 4),
                   "ratio": round(med(t_lgo) / med(t_loo), 3),
                   "spread_loo_ms": [round(min(t_loo), 4), round(max(t_loo), 4)], "spread_lgo_ms": [round(min(t_lgo), 4), round(max(t_lgo), 4)],
                   "loo_phase_ms": {k: round(v, 4) for k, v in zip(NAMES, acc_loo / a.reps)},
                   "lgo_phase_ms": {k: round(v, 4) for k, v in zip(NAMES, acc_lgo / a.reps)}}
            print(json.dumps(row), flush=True)
            rows.append(row)
        prob.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
