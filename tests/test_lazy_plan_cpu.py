"""CPU: the two queues of a line-search trial evaluated in two phases (csrc/dag_plan.hpp: the plan built without the K^-1 tiles,
and dag_plan_kinv_only of the full plan) for the shapes the engine builds: both pass the plan checker (topological order, full-count
waits, no unordered tile access -- so a launch of either cannot hang), the K^-1-only queue holds exactly the full plan's DAGF_CKINV
tasks (same tiles, same contraction ranges, same order among themselves: every element keeps its accumulation chain), and the
first-phase queue holds none of them and every other task of the full plan."""
import ctypes as C

import numpy as np
import pytest

from hbetune_rs_amd import _lib

DAGF_CKINV = 128
# workgroups per launch of the busy-slot variants on 256 CUs (1, 2, 3 busy slots) and of the crowded-device levels (6, 12, 24 runs)
NWG = (256, 144, 96, 48, 24, 8)


def queue(nb, bk, nwg, fine, big128, which):
    lib = _lib.load()
    nt = C.c_int()
    err = C.create_string_buffer(400)
    cap = 40000
    tasks = np.zeros((cap, 6), dtype=np.int32)
    rc = lib.hbegp_debug_dag_queues(nb, bk, 4, nwg, fine, big128, which, C.byref(nt), tasks.ctypes.data_as(C.POINTER(C.c_int)), cap, err, 400)
    assert nt.value <= cap
    return rc, tasks[: nt.value].copy(), err.value.decode()


@pytest.mark.parametrize("nb", [6, 7, 8, 32])
def test_two_phase_queues_are_sound_and_hold_the_full_plans_tasks(nb):
    # the engine's plan: right-looking, row-progressive up to 20 blocks; 128x128 tiles from 32 blocks on when slots share the chip
    base = 1 | 8 | (16 if nb <= 20 else 0)
    n_checked = 0
    for bk in (16, 32):  # stage depth of f64 / f32
        for nwg in NWG:
            for fine, big128 in [(base, 0), (base | 32, 2 if nb >= 32 else 0)]:  # one slot (split K^-1 sums) / a fit's slots
                rc0, full, e0 = queue(nb, bk, nwg, fine, big128, 0)
                rc1, p1, e1 = queue(nb, bk, nwg, fine, big128, 1)
                rc2, kv, e2 = queue(nb, bk, nwg, fine, big128, 2)
                assert (rc0, rc1, rc2) == (0, 0, 0), (nb, bk, nwg, fine, big128, e0, e1, e2)
                is_kinv = (full[:, 1] & DAGF_CKINV) != 0
                assert is_kinv.sum() > 0
                assert np.array_equal(kv, full[is_kinv]), (nb, bk, nwg, fine)  # same tiles, same k ranges, same order
                assert not np.any(p1[:, 1] & DAGF_CKINV)
                # the first phase is the rest of the full plan: the same tasks (its own order: a list schedule of its own)
                rest = full[~is_kinv]
                key = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
                assert np.array_equal(key(p1), key(rest)), (nb, bk, nwg, fine)
                n_checked += 1
    assert n_checked == 2 * len(NWG) * 2


def test_kinv_only_queue_keeps_the_order_gates_of_the_row_progressive_plan():
    # the row-progressive K^-1 adds range after range onto the same tiles: the continued sums (beta = 1) must come after the
    # tiles they continue in queue order, which the checker enforces through the kept gates
    rc, kv, err = queue(8, 16, 96, 1 | 8 | 16 | 32, 0, 2)
    assert rc == 0 and len(kv) > 0
    acc = (kv[:, 1] & 64) != 0  # DAGF_ACC
    assert acc.any() and not acc[0]
    first_write = {}
    for i, t in enumerate(kv):
        first_write.setdefault((int(t[2]) // 64, int(t[3]) // 64), i)
    for i, t in enumerate(kv):
        if acc[i]:
            assert first_write[(int(t[2]) // 64, int(t[3]) // 64)] < i
