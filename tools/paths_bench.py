"""Times of the posterior sample paths on one model: the preparation (hbegp_paths_create, its phases split by device events:
uploads + frequency scaling, feature projection, the two triangular products), the shared-point evaluation with gradients at
m = 1600 / 16k / 128k, and one minimiser run (R = 8 starts per path, maxeval = 150).  Models: extend() at a fixed theta on the C2
workload (Rosenbrock, d = 8), n = 1024 and 4096, S = 16 and 64, F = 1024 and 4096, f64 and f32.  Beside them the only other route
to a draw, hbegp_sample_posterior at m = 1600 with the same S.

    python tools/paths_bench.py [--reps 3] [--quick] [--out FILE]

Prints one JSON object per measurement (wall-clock medians of synchronous calls, milliseconds)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hbetune_rs_amd import _lib  # noqa: E402
from hbetune_rs_amd import estimator as E  # noqa: E402
from hbetune_rs_amd import gpr, synth  # noqa: E402


def _model(n, dtype):
    w = synth.make_workload("C2", n=n)
    X, y = w["X"].astype(dtype), w["y"].astype(dtype)
    d = X.shape[1]
    theta = np.log(np.concatenate([[1e-2, 1.0], np.full(d, 0.5)]))
    return gpr.FittedKernel.extend(X, y, theta, nu=2.5), d


def _median_ms(fn, reps):
    fn()  # warm-up: scratch growth, first launches
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="n = 1024 and m <= 16k only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    rows = []
    phases = np.zeros(3)
    for dtype in (np.float64, np.float32):
        for n in ((1024,) if a.quick else (1024, 4096)):
            fk, d = _model(n, dtype)
            rng = np.random.default_rng(0)
            for S in (16, 64):
                xs1600 = rng.uniform(0, 1, (1600, d)).astype(dtype)
                z = rng.standard_normal((S, 1600)).astype(dtype)
                exact = _median_ms(lambda: fk.sample_posterior(xs1600, z, jitter=1e-6), a.reps)
                for F in (1024, 4096):
                    r = E.RNG(1)
                    om0, ph = gpr.draw_spectral(fk.nu, F, d, r)
                    w, eps = r.standard_normal((S, F)), r.standard_normal((S, n))
                    made = []

                    def create():
                        made.append(fk.sample_paths(om0, ph, w, eps))

                    lib.hbegp_debug_paths_phases(1, None)
                    prep = _median_ms(create, a.reps)
                    lib.hbegp_debug_paths_phases(0, _lib.dptr(phases))
                    paths = made.pop()
                    for p in made:
                        p.release()
                    row = {"dtype": np.dtype(dtype).name, "n": n, "S": S, "F": F, "prepare_ms": round(prep, 3),
                           "prepare_phases_ms": [round(float(v), 3) for v in phases], "exact_draw_m1600_ms": round(exact, 3)}
                    for m in ((1600, 16384) if a.quick else (1600, 16384, 131072)):
                        xs = rng.uniform(0, 1, (m, d)).astype(dtype)
                        row[f"eval_m{m}_ms"] = round(_median_ms(lambda: paths.evaluate(xs), 1 if m > 20000 else a.reps), 3)
                    starts = rng.uniform(0, 1, (S, 8, d)).astype(dtype)
                    nev = []
                    row["minimize_ms"] = round(_median_ms(lambda: nev.append(paths.minimize(starts, np.zeros(d), np.ones(d))[2].sum()), 1), 3)
                    row["minimize_evals"] = int(nev[-1])
                    paths.release()
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            fk.release()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
