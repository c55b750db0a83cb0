"""Times of noisy expected improvement over a candidate set on one model: hbegp_noisy_ei with the phases split by device events
(hbegp_debug_nei_phases: Sigma, the baseline's factor, the panel and draw products, the reductions) and the wall time of the whole
call.  Model: extend() at a fixed theta on the C2 workload (Rosenbrock, d = 8), n = 4096, f64 and f32 (f32 with a noise of the
amplitude's size, as the f32 tests: DESIGN section 11); baseline = the training rows, mc = 1600 candidates, S = 256 draws.

Next to it the composition that needs no noisy-EI call: sample_posterior on the union of baseline and candidates (one factor of all
mb + mc rows) and the plain Monte Carlo estimate mean_s max(0, min_i f_s(b_i) - f_s(x_j)) in NumPy.

    python tools/nei_bench.py [--reps 5] [--n 4096] [--mc 1600] [--draws 256] [--out FILE]

Prints one JSON object per measurement and a table at the end (medians of synchronous calls, ms)."""
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
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--mc", type=int, default=1600)
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    rows = []
    phases = np.zeros(4)

    def timed(fn, reps, hook, warmup=1):
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

    n, mc, S = a.n, a.mc, a.draws
    for dtype in (np.float64, np.float32):
        w = synth.make_workload("C2", n=n)
        X, y = w["X"].astype(dtype), w["y"].astype(dtype)
        d = X.shape[1]
        noise = 1e-2 if dtype == np.float64 else 1.0
        theta = np.log(np.concatenate([[noise, 1.0], np.full(d, 0.5)]))
        fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
        cand = synth.candidates("C2", mc, d).astype(dtype)
        rng = np.random.default_rng(0)
        z = rng.standard_normal((S, n)).astype(dtype)
        zu = np.hstack([z, rng.standard_normal((S, mc)).astype(dtype)])
        union = np.vstack([X, cand])
        rec = dict(n=n, d=d, dtype=np.dtype(dtype).name, mb=n, mc=mc, S=S, noise=noise)
        try:
            lib.hbegp_debug_nei_phases(1, None)
            t_call, ph = timed(lambda: fk.noisy_ei(X, cand, z), a.reps, lib.hbegp_debug_nei_phases)
            nei, best = fk.noisy_ei(X, cand, z)
            rec.update(sigma_ms=round(float(ph[0]), 4), factor_ms=round(float(ph[1]), 4), products_ms=round(float(ph[2]), 4),
                       reduce_ms=round(float(ph[3]), 4), device_ms=round(float(ph.sum()), 4), call_ms=round(t_call, 4),
                       nei_max=float(nei.max()), best=best)
        except _lib.HbegpError as e:
            rec.update(nei_error=str(e))
        finally:
            lib.hbegp_debug_nei_phases(0, None)

        def composed():
            f, _ = fk.sample_posterior(union, zu)
            f = f.astype(np.float64)
            return np.maximum(0.0, f[:, :n].min(axis=1)[:, None] - f[:, n:]).mean(axis=0)

        try:
            lib.hbegp_debug_posterior_phases(1, None)
            t_comp, php = timed(composed, a.reps, lib.hbegp_debug_posterior_phases)
            plain = composed()
            rec.update(composed_call_ms=round(t_comp, 4), composed_device_ms=round(float(php.sum()), 4),
                       composed_factor_ms=round(float(php[2]), 4), composed_best=int(len(plain) - 1 - np.argmax(plain[::-1])))
        except _lib.HbegpError as e:
            rec.update(composed_error=str(e))
        finally:
            lib.hbegp_debug_posterior_phases(0, None)
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        fk.release()

    print("\n| n = mb | type | mc | S | Sigma | factor | products | reductions | device total | call | sample_posterior + NumPy: device | call |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        mine = (f"{r['sigma_ms']:.3f} | {r['factor_ms']:.3f} | {r['products_ms']:.3f} | {r['reduce_ms']:.3f} | {r['device_ms']:.3f} | "
                f"{r['call_ms']:.3f}") if "call_ms" in r else "failed | | | | |"
        comp = f"{r['composed_device_ms']:.3f} | {r['composed_call_ms']:.3f}" if "composed_call_ms" in r else "failed |"
        print(f"| {r['n']} | {r['dtype']} | {r['mc']} | {r['S']} | {mine} | {comp} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
