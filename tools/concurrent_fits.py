#!/usr/bin/env python3
"""k independent fixed-work fits side by side on ONE GPU, one host thread each, one context (replicas).
Usage: concurrent_fits.py n k [k ...]   -> aggregate fits/s per k, and whether every concurrent fit reproduced the solo fit's bits;
the last line is the same as JSON.  HIP maps streams onto a few hardware queues per device (4 by default) and streams that share
a queue run one after the other (one stream per optimiser run; up to 128 rows one per fit)."""
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hbetune_rs_amd import gpr, synth  # noqa: E402

n = int(sys.argv[1])
ks = [int(a) for a in sys.argv[2:]] or [1, 2, 4]
dtype = np.float32 if os.environ.get("FIT_F32") else np.float64
w = synth.make_workload("M", n=n)
X, y = w["X"].astype(dtype), w["y"].astype(dtype)
starts = synth.restart_points("M", w["lo"], w["hi"], 2)
ctx = gpr.Context(device_ids=[0])


phases = np.zeros(3)  # FIT_PHASES=1: seconds in new / predict / release, summed over all threads (racy adds: a diagnostic)


def fit():
    t0 = time.perf_counter()
    fk = gpr.FittedKernel.new(X, y, w["theta0"], w["lo"], w["hi"], starts, nu=2.5, ctx=ctx, maxeval=150, fixed_work=True)
    t1 = time.perf_counter()
    mean, var, _ = fk.predict(X[:8])  # (the whole K^-1 is a 134 MB copy at n = 4096: the predictions stand in for the model's bits)
    t2 = time.perf_counter()
    out = (fk.lml, fk.theta.copy(), np.concatenate([mean, var]))
    fk.release()
    t3 = time.perf_counter()
    phases[:] += (t1 - t0, t2 - t1, t3 - t2)
    return out


solo = fit()
summary = {"n": n, "dtype": np.dtype(dtype).name, "fits_per_s": {}, "bitwise_equal_to_solo": True}
for k in ks:
    reps = max(8, 24 // k) if n <= 256 else max(2, 8 // k)  # (small fits: rounds of several threads need a few rounds to fall into step)
    results = [[] for _ in range(k)]

    def work(i):
        for _ in range(reps):
            results[i].append(fit())

    for _ in range(1):  # warm-up round: every thread's pools
        ts = [threading.Thread(target=work, args=(i,)) for i in range(k)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    results = [[] for _ in range(k)]
    phases[:] = 0
    t0 = time.perf_counter()
    ts = [threading.Thread(target=work, args=(i,)) for i in range(k)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    dt = time.perf_counter() - t0
    if os.environ.get("FIT_PHASES"):
        print(f"  per fit: new {phases[0] / (k * reps) * 1e3:.2f} ms, predict {phases[1] / (k * reps) * 1e3:.2f} ms, release {phases[2] / (k * reps) * 1e3:.2f} ms")
    same = all(r[0] == solo[0] and np.array_equal(r[1], solo[1]) and np.array_equal(r[2], solo[2]) for rs in results for r in rs)
    print(f"n={n} {np.dtype(dtype).name} k={k}: {k * reps / dt:.2f} fits/s aggregate ({dt / reps * 1e3:.1f} ms per round of {k}); "
          f"every fit bit for bit the solo fit: {same}", flush=True)
    summary["fits_per_s"][str(k)] = k * reps / dt
    summary["bitwise_equal_to_solo"] = bool(summary["bitwise_equal_to_solo"] and same)
ctx.close()
print(json.dumps(summary), flush=True)
