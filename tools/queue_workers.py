#!/usr/bin/env python3
"""How many compute units does a task-queue launch of a fit really hold, and how long do its tasks take there?

Reads the task traces a fit keeps of its own launches (HBEGP_DAG_TRACE=<prefix> HBEGP_DAG_TRACE_EVALS=a:b: one file per launch,
<prefix>.s<slot>.e<evaluation>.p<part>, written when the fit's problem is released; csrc/hbegp.cpp keep_fit_trace).  A dag workgroup
takes a whole CU and stays on it from its first claim to its last publication, so the CUs a launch holds at time t are the CUs with
first claim <= t <= last publication.

Usage: queue_workers.py <prefix> [costs]
  per kind of queue (fused / phase 1 / K^-1 alone) and share (even / lead / lag): launches seen, workgroups launched, distinct CUs
  over the launch's life, CUs held at 2 % / 25 % / 50 % / 75 % / 98 % of its life, the time average, and when the 64th / 80th / 96th
  CU joined (medians over the launches; times in us)
  costs: per task class (kind, contraction depth, beta = 1, row-major contraction operand, K^-1 output) the median ready ->
  published time, a line fit "fixed + rate x depth / 128" per class group, and the hand-off between two tasks of one workgroup."""
import glob
import re
import sys

import numpy as np

prefix = sys.argv[1]
want_costs = len(sys.argv) > 2
PART = {0: "fused", 1: "phase 1", 2: "K^-1 alone"}
SHARE = {0: "even", 1: "lead", 2: "lag"}
KIND = {0: "128x64", 1: "64x64", 2: "leaf", 8: "32x64", 9: "128x128"}
AKM, BKM, ACC, CKINV = 8, 16, 64, 128  # DAGF_* of csrc/engine.hpp
groups, rows_all = {}, []
for name in sorted(glob.glob(prefix + ".s*.e*.p*")):
    head = open(name).readline()
    m = re.match(r"# slot (\d+) evaluation (\d+) part (\d+) variant (\d+) share (\d+) nwg (\d+) tasks (\d+)", head)
    if not m:
        continue
    slot, ev, part, variant, share, nwg, ntasks = map(int, m.groups())
    a = np.loadtxt(name, dtype=np.int64, ndmin=2)
    if len(a) == 0:
        continue
    pulled, ready, comp, pub = [a[:, c] * 0.01 for c in (6, 7, 8, 9)]  # us
    ok = (pub >= ready) & (ready >= pulled) & (pulled > pulled.max() - 50e3)  # (a launch lasts a few ms)
    if ok.sum() < len(a):
        print(f"{name}: {len(a) - ok.sum()} of {len(a)} tasks without a stamp of this launch -- skipped", file=sys.stderr)
        continue
    cu = a[:, 10] * (1 << 32) + (a[:, 11] & 0xFFFFFF00)
    t0, t1 = pulled.min(), pub.max()
    life = t1 - t0
    ids = np.unique(cu)
    first = np.array([pulled[cu == c].min() for c in ids]) - t0
    last = np.array([pub[cu == c].max() for c in ids]) - t0
    held = lambda f: int(((first <= f * life) & (last >= f * life)).sum())  # noqa: E731
    joined = np.sort(first)
    nth = lambda k: joined[k - 1] if len(joined) >= k else np.nan  # noqa: E731
    busy, wait = (pub - ready).sum(), (ready - pulled).sum()
    groups.setdefault((part, share, nwg), []).append(
        [len(ids), held(0.02), held(0.25), held(0.5), held(0.75), held(0.98), (last - first).sum() / life, nth(64), nth(80), nth(96), life,
         100 * wait / (busy + wait)])
    if want_costs:
        for i in range(len(a)):
            rows_all.append((part, share, int(a[i, 1]), int(a[i, 4]), int(a[i, 12]), pub[i] - ready[i], comp[i] - ready[i]))
        # hand-off: publication of a workgroup's task -> its next task running, where that task did not wait for counters long
        for c in ids:
            idx = np.nonzero(cu == c)[0]
            idx = idx[np.argsort(ready[idx])]
            for x, y in zip(idx[:-1], idx[1:]):
                rows_all.append((part, share, -1, 0, 0, ready[y] - pub[x], 0.0))

print(f"{'queue':12s} {'share':5s} {'wg':>4s} {'n':>4s} {'CUs':>5s} {'2 %':>5s} {'25 %':>5s} {'50 %':>5s} {'75 %':>5s} {'98 %':>5s} {'mean':>6s} "
      f"{'64th at':>8s} {'80th at':>8s} {'96th at':>8s} {'life us':>8s} {'wait %':>7s}")
for (part, share, nwg), v in sorted(groups.items()):
    v = np.array(v, dtype=float)
    med = np.array([np.median(c[~np.isnan(c)]) if (~np.isnan(c)).any() else np.nan for c in v.T])  # (nan: fewer CUs than that)
    print(f"{PART[part]:12s} {SHARE[share]:5s} {nwg:4d} {len(v):4d} {med[0]:5.0f} {med[1]:5.0f} {med[2]:5.0f} {med[3]:5.0f} {med[4]:5.0f} {med[5]:5.0f} {med[6]:6.1f} "
          f"{med[7]:8.0f} {med[8]:8.0f} {med[9]:8.0f} {med[10]:8.0f} {med[11]:7.1f}")

if want_costs:
    r = np.array(rows_all, dtype=float)
    ho = r[r[:, 2] < 0][:, 5]
    print(f"\nhand-off published(a) -> ready(b) on one workgroup: median {np.median(ho):.2f} us, 25 % {np.percentile(ho, 25):.2f}, 75 % {np.percentile(ho, 75):.2f} "
          f"(includes waits for counters; the quartile below the median is the claim itself)")
    r = r[r[:, 2] >= 0]
    kind, depth, flags, dur = r[:, 2].astype(int), r[:, 3].astype(int), r[:, 4].astype(int), r[:, 5]
    cls = {}
    for k, d, f, t in zip(kind, depth, flags, dur):
        key = (k, bool(f & ACC), bool(f & (AKM | BKM)), bool(f & CKINV), d)
        cls.setdefault(key, []).append(t)
    print(f"{'kind':8s} {'beta=1':>6s} {'row-major':>9s} {'K^-1':>5s} {'depth':>6s} {'n':>7s} {'median us':>10s} {'25 %':>8s} {'75 %':>8s}")
    for key in sorted(cls):
        t = np.array(cls[key])
        print(f"{KIND.get(key[0], key[0]):8s} {int(key[1]):6d} {int(key[2]):9d} {int(key[3]):5d} {key[4]:6d} {len(t):7d} {np.median(t):10.2f} {np.percentile(t, 25):8.2f} {np.percentile(t, 75):8.2f}")
    print("\nline fits over the class medians, weighted by task count: time = fixed + rate x depth / 128")
    fit_groups = {}
    for key, t in cls.items():
        if key[0] == 2:
            continue
        fit_groups.setdefault(key[:3], []).append((key[4], np.median(t), len(t)))
    for g in sorted(fit_groups):
        pts = np.array(fit_groups[g], dtype=float)
        name = f"{KIND.get(g[0], g[0])} beta=1:{int(g[1])} row-major:{int(g[2])}"
        if len(pts) < 2:
            print(f"  {name:40s} one depth ({pts[0, 0]:.0f}): {pts[0, 1]:.2f} us")
            continue
        A = np.stack([np.ones(len(pts)), pts[:, 0] / 128.0], axis=1) * np.sqrt(pts[:, 2:3])
        sol = np.linalg.lstsq(A, pts[:, 1] * np.sqrt(pts[:, 2]), rcond=None)[0]
        print(f"  {name:40s} fixed {sol[0]:6.2f} us  rate {sol[1]:6.2f} us per 128   ({len(pts)} depths, {int(pts[:, 2].sum())} tasks)")
    leaf = np.concatenate([np.array(v) for k, v in cls.items() if k[0] == 2])
    print(f"  diagonal block: median {np.median(leaf):.2f} us ({len(leaf)} tasks)")
