"""Cost of a leave-one-out evaluation next to a log-marginal-likelihood evaluation, on the same build and the same slot.

On the workload of a config (default M: n = 4096, d = 8, f64) at its reference theta: hbegp_problem_eval with gradient and
hbegp_problem_eval_loo with gradient on ONE slot of ONE problem, alternating, after a warm-up of both (graph instantiation, the
borrowed work matrices' first allocation); wall-clock medians of the synchronous calls.  Then the four phases of the
leave-one-out tail from device events (hbegp_debug_loo_phases): the diagonal pass, u and Y, the SYRK C = Y Y^T, the weighted
trace, with the rates they imply -- bytes of the triangle of L^-1 read by the diagonal pass, the algorithmic flops of the SYRK.

    python tools/loo_bench.py [--config M] [--f32] [--reps 15] [--out FILE]

Prints one JSON object.  ratio = eval_loo_ms / eval_lml_ms: the tail adds one symmetric n^3 product to an evaluation whose
factor, inverse and K^-1 together are about n^3 flops, so roughly 2 is expected; well above 2 means a phase is off its rate."""
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
    ap.add_argument("--config", default="M")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--f32", action="store_true")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    w = synth.make_workload(a.config) if a.n is None else synth.make_workload(a.config, n=a.n)
    dtype = np.float32 if a.f32 else np.float64
    X, y, theta = w["X"].astype(dtype), w["y"].astype(dtype), w["theta"]
    n, d = X.shape
    prob = gpr.Problem(X, y)
    for _ in range(2):  # warm-up of both
        lml, _ = prob.lml_with_gradient(theta)
        loo, _ = prob.loo_with_gradient(theta)
    t_lml, t_loo, t_tail = [], [], []
    phases = np.zeros(4)
    acc = np.zeros(4)
    lib.hbegp_debug_loo_phases(1, None)
    for _ in range(a.reps):  # alternating
        t0 = time.perf_counter()
        prob.lml_with_gradient(theta)
        t1 = time.perf_counter()
        prob.loo_with_gradient(theta)
        t2 = time.perf_counter()
        t_lml.append((t1 - t0) * 1e3)
        t_loo.append((t2 - t1) * 1e3)
        lib.hbegp_debug_loo_phases(1, _lib.dptr(phases))
        acc += phases
    lib.hbegp_debug_loo_phases(0, None)
    # the evaluation without the lml gradient, which eval_loo runs in front of its tail
    for _ in range(a.reps):
        t0 = time.perf_counter()
        prob.lml_with_gradient(theta, want_grad=False)
        t_tail.append((time.perf_counter() - t0) * 1e3)
    prob.close()
    ph = acc / a.reps
    npad = (n + 127) // 128 * 128
    esz = np.dtype(dtype).itemsize
    tri_bytes = esz * n * (n + 1) / 2
    syrk_flop = 2.0 * npad * (npad + 1) / 2 * npad
    med = lambda v: float(np.median(v))  # noqa: E731
    row = {"config": a.config, "n": n, "d": d, "dtype": np.dtype(dtype).name, "reps": a.reps, "lml": lml, "loo": loo,
           "eval_lml_grad_ms": round(med(t_lml), 4), "eval_loo_grad_ms": round(med(t_loo), 4),
           "eval_lml_nograd_ms": round(med(t_tail), 4), "ratio": round(med(t_loo) / med(t_lml), 3),
           "spread_lml_ms": [round(min(t_lml), 4), round(max(t_lml), 4)], "spread_loo_ms": [round(min(t_loo), 4), round(max(t_loo), 4)],
           "phase_ms": {"diag": round(ph[0], 4), "u_and_Y": round(ph[1], 4), "syrk": round(ph[2], 4), "trace": round(ph[3], 4)},
           "diag_GBps": round(tri_bytes / (ph[0] * 1e-3) / 1e9, 1) if ph[0] > 0 else None,
           "u_and_Y_GBps": round((tri_bytes + esz * npad * npad) / (ph[1] * 1e-3) / 1e9, 1) if ph[1] > 0 else None,
           "syrk_TFLOPs": round(syrk_flop / (ph[2] * 1e-3) / 1e12, 2) if ph[2] > 0 else None}
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
