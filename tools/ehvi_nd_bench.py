"""Times of the expected hypervolume improvement of three objectives over a candidate set: hbegp_ehvi_nd with the phases split by
device events (hbegp_debug_ehvi_nd_phases: the three predicts, each on its model's stream, and the box kernel), the wall time of
the whole call, the host's box decomposition on its own (hbegp_debug_ehvi_boxes, counts only), and the wall time of the same
numbers obtained the old way -- three predict() calls and the NumPy restatement (tests/ehvi_nd_ref.py, its decomposition not
counted) on the host.  Models: extend() at a fixed theta on the C2 workload (Rosenbrock, d = 8), n = 4096, three response
functions, f64 and f32; m in {4096, 65536}, P in {16, 64, 256} (points of a sphere shell, every one non-dominated), and
P = 1024 at m = 4096 for the maximiser's sake.

    python tools/ehvi_nd_bench.py [--reps 5] [--out FILE] [--no-host]

Prints one JSON object per measurement and a table at the end (medians of synchronous calls).  boxes_per_us: m * boxes per
microsecond of the kernel phase.  grad64_*: the call with a gradient on the first 64 candidates -- one round of a maximiser with
64 runs as a call of its own, so with one decomposition.  round_ms: the wall time of hbegp_maximize_ehvi_nd with 64 runs and
maxeval = 8, less decompose_ms (it decomposes once), per round (the largest nevals) -- a round uploads the boxes (box_bytes)
and decomposes nothing.  host_rows: the rows the host path was timed on (the largest of m, 4096 and 256 with
rows * boxes <= 2^26)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ehvi_nd_ref  # noqa: E402
from hbetune_rs_amd import _lib  # noqa: E402
from hbetune_rs_amd import gpr, synth  # noqa: E402

M = 3


def host_ehvi(fks, Xs, front, ref, dec):
    """What a caller did before hbegp_ehvi_nd: the posteriors back to the host, then the box arithmetic in NumPy."""
    pm = [fk.predict(Xs) for fk in fks]
    mu = np.stack([p[0] for p in pm], axis=1).astype(np.float64)
    var = np.stack([p[1] for p in pm], axis=1).astype(np.float64)
    return ehvi_nd_ref.ehvi(mu, var, front, ref, dec)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the predicts-plus-NumPy timing")
    a = ap.parse_args()
    lib = _lib.load()
    rows = []
    phases = np.zeros(5)

    def timed(fn, reps, warmup=1):
        for _ in range(warmup):
            fn()
        wall, ph = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            lib.hbegp_debug_ehvi_nd_phases(1, _lib.dptr(phases))
            ph.append(phases.copy())
        return float(np.median(wall)), np.median(np.array(ph), axis=0)

    def decompose_ms(front, ref, reps):
        counts, nb, ip = np.zeros(M, np.int32), C.c_int(0), C.POINTER(C.c_int)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            _lib.check(lib.hbegp_debug_ehvi_boxes(_lib.dptr(front), len(front), M, _lib.dptr(ref), counts.ctypes.data_as(ip), None, 0,
                                                  C.byref(nb), None, 0))
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t)), nb.value, int(counts.sum())

    n = 4096
    for dtype in (np.float64, np.float32):
        w = synth.make_workload("C2", n=n)
        X = w["X"].astype(dtype)
        Xd = np.asarray(w["X"], dtype=np.float64)
        d = X.shape[1]
        y0 = np.asarray(w["y"], dtype=np.float64)
        y1 = ((Xd - 0.3) ** 2).sum(axis=1)
        y1 = y1 / y1.mean()
        y2 = np.cos(2.0 * Xd).sum(axis=1) + Xd[:, 0]
        theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
        ys = (y0, y1, y2)
        fks = [gpr.FittedKernel.extend(X, y.astype(dtype), theta, nu=nu) for y, nu in zip(ys, (2.5, 1.5, 0.5))]
        lo = np.array([y.min() for y in ys])
        hi = np.array([y.max() for y in ys])
        ref = np.ascontiguousarray(hi + 0.1 * (hi - lo))
        lib.hbegp_debug_ehvi_nd_phases(1, None)
        for m in (4096, 65536):
            Xs = synth.candidates("C2", m, d).astype(dtype)
            for P in (16, 64, 256) + ((1024,) if m == 4096 else ()):
                x = np.abs(np.random.default_rng(P).standard_normal((P, M))) + 0.05
                front = np.ascontiguousarray(lo + (hi - lo) * x / np.linalg.norm(x, axis=1, keepdims=True))
                t_dec, n_boxes, n_thr = decompose_ms(front, ref, a.reps)
                t_call, ph = timed(lambda: gpr.ehvi_nd(fks, Xs, front, ref), a.reps)
                t_grad, phg = timed(lambda: gpr.ehvi_nd(fks, Xs[:64], front, ref, want_grad=True), a.reps)
                val, best = gpr.ehvi_nd(fks, Xs, front, ref)
                bounds = np.stack([Xs.min(axis=0), Xs.max(axis=0)], axis=1)
                rounds = []

                def ascend():
                    rounds.append(int(gpr.maximize_ehvi_nd(fks, Xs[:64], bounds, front, ref, maxeval=8)[2].max()))

                t_max, _ = timed(ascend, a.reps)
                rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, m=m, P=P, boxes=n_boxes, thresholds=n_thr, box_bytes=8 * M * n_boxes,
                           predict0_ms=round(float(ph[0]), 4), predict1_ms=round(float(ph[1]), 4), predict2_ms=round(float(ph[2]), 4),
                           kernel_ms=round(float(ph[3]), 4), call_ms=round(t_call, 4), decompose_ms=round(t_dec, 4),
                           boxes_per_us=round(m * n_boxes / (ph[3] * 1e3), 1) if ph[3] > 0 else None,
                           grad64_call_ms=round(t_grad, 4), grad64_kernel_ms=round(float(phg[3]), 4),
                           round_ms=round((t_max - t_dec) / rounds[-1], 4), rounds=rounds[-1], ehvi_max=float(val.max()), best=best)
                if not a.no_host:
                    hr = next((r for r in (m, 4096, 256) if r <= m and r * n_boxes <= 1 << 26), 256)
                    dec = ehvi_nd_ref.boxes(front, ref)
                    t0 = time.perf_counter()
                    hv = host_ehvi(fks, Xs[:hr], front, ref, dec)
                    rec["host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                    rec["host_rows"] = hr
                    rec["host_max_dev"] = float(np.abs(hv - val[:hr]).max())
                print(json.dumps(rec), flush=True)
                rows.append(rec)
        lib.hbegp_debug_ehvi_nd_phases(0, None)
        for fk in fks:
            fk.release()

    print("\n| type | m | P | boxes | predict 0 | predict 1 | predict 2 | box kernel | call | boxes / us | decomposition | "
          "predicts + NumPy (rows) | call with gradient, m = 64 | maximiser round, 64 runs |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        host = f"{r['host_ms']} ({r['host_rows']})" if "host_ms" in r else "-"
        print(f"| {r['dtype']} | {r['m']} | {r['P']} | {r['boxes']} | {r['predict0_ms']:.3f} | {r['predict1_ms']:.3f} | {r['predict2_ms']:.3f} | "
              f"{r['kernel_ms']:.3f} | {r['call_ms']:.3f} | {r['boxes_per_us']} | {r['decompose_ms']:.3f} | {host} | {r['grad64_call_ms']:.3f} | {r['round_ms']:.3f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
