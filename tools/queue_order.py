#!/usr/bin/env python3
"""The in-order replay of a fit's task queues on the CPU (csrc/dag_plan.hpp: dag_plan_replay, through hbegp_debug_dag_replay): for
each queue of the flagship problem -- 32 blocks, f64, three slots: fused, phase 1, K^-1 alone -- the makespan and the share of the
CU time spent waiting on counters when a queue ordered for X workers is pulled by W workgroups, under the planner's task times.
No GPU.  Usage: queue_order.py [blocks [launch_wg]]   ->  one table per queue; rows: ordered for, columns: run on."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from hbetune_rs_amd import _lib

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 32
nwg = int(sys.argv[2]) if len(sys.argv) > 2 else 96
ORDERS = [48, 56, 64, 72, 80, 88, 96, 104, 112, 128, -1]
WORKERS = [48, 56, 64, 72, 80, 88, 96, 112, 128]
lib = _lib.load()
fine = 1 | 8 | (16 if nb <= 20 else 0) | 32
big128 = 2 if nb >= 32 else 0


def replay(order_wg, which, workers):
    nt, err, out = C.c_int(), C.create_string_buffer(400), np.zeros(6)
    rc = lib.hbegp_debug_dag_replay(nb, 16, 4, nwg, order_wg, fine, big128, which, workers, C.byref(nt), None, 0,
                                    out.ctypes.data_as(C.POINTER(C.c_double)), err, 400)
    assert rc == 0, err.value.decode()
    return nt.value, out


for which, name in ((0, "fused"), (1, "phase 1"), (2, "K^-1 alone")):
    nt, out = replay(0, which, nwg)
    print(f"== {name}: {nt} tasks, planner work {out[2] / 1e3:.1f} ms x CU (128x128 tasks with beta = 1: {out[5] / 1e3:.1f}), critical path {out[4]:.0f} us, "
          f"sim_us {out[3]:.0f} at {nwg} workers")
    print("ordered for \\ run on " + "".join(f"{w:>14d}" for w in WORKERS))
    for o in ORDERS:
        cells = []
        for w in WORKERS:
            _, r = replay(o, which, w)
            cells.append(f"{r[0]:7.0f} {100 * r[1] / (r[1] + r[2]):4.1f} %")
        print(f"{'by level' if o < 0 else o:>20} " + "".join(f"{c:>14s}" for c in cells))
    best = {w: min(ORDERS, key=lambda o: replay(o, which, w)[1][0]) for w in WORKERS}
    print("best order per worker count: " + "  ".join(f"{w}: {'by level' if o < 0 else o}" for w, o in best.items()))
