#!/usr/bin/env python3
"""When do the optimiser runs of a fit end?  Fixed-work (or, with a fourth argument, early-stopping) fits of config M as
tools/fit_rate.py runs them, with the per-run clocks and launch counts of hbegp_last_fit_stats beside the wall time of every fit.
Usage: run_ends.py [fits [n [dtype [early]]]]   -> one line per fit, then the median / min / max ms per fit; env switches apply."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from hbetune_rs_amd import gpr, synth

nfit = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2] != "-" else None
dtype = sys.argv[3] if len(sys.argv) > 3 else "float64"
early = len(sys.argv) > 4
w = synth.make_workload("M", n=n, dtype=dtype)
starts = synth.restart_points("M", w["lo"], w["hi"], 2)
ctx = gpr.Context(device_ids=[0])
def fit():
    t0 = time.perf_counter()
    fk = gpr.FittedKernel.new(w["X"], w["y"], w["theta0"], w["lo"], w["hi"], starts, nu=2.5, ctx=ctx, maxeval=150, fixed_work=not early)
    ms = (time.perf_counter() - t0) * 1e3
    out = ms, fk.run_end_ms, fk.run_counts, fk.n_evals, fk.lml
    fk.release()
    return out
fit()
times = []
for i in range(nfit):
    ms, ends, c, ne, lml = fit()
    times.append(ms)
    runs = "  ".join(f"run {r}: {ends[r]:.1f} ms (fused {c['fused'][r]} lml-only {c['lml_only'][r]} two-phase {c['phase2'][r]} lead {c['lead'][r]} lag {c['lag'][r]})"
                     for r in range(len(ends)))
    print(f"fit {i}: {ms:.1f} ms, {ne} evaluations, last - first run end {ends.max() - ends.min():.1f} ms | {runs}", flush=True)
print(f"ms per fit: median {np.median(times):.1f}  min {min(times):.1f}  max {max(times):.1f}  ({nfit} fits)  lml={lml!r}", flush=True)
ctx.close()
