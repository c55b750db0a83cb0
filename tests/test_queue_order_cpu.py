"""CPU: a task queue ordered for another worker count than it is launched with (csrc/dag_plan.hpp: DagBuilder's order_wg, the
in-order replay dag_plan_replay, the default dag_default_order_wg; through hbegp_debug_dag_replay / hbegp_debug_dag_order_wg).
For 6, 8 and 32 blocks, both stage depths and every order_wg the defaults can produce -- plus the measured candidates, one worker,
a count above every launch size and the count-independent order -- all three queues of an evaluation pass the plan checker, hold
exactly the tasks of the order_wg == nwg queue, the K^-1-only queue is the full plan's K^-1 tasks in its order, and the replay on
order_wg workers returns the planner's own makespan."""
import ctypes as C
import functools

import numpy as np
import pytest

from hbetune_rs_amd import _lib

DAGF_CKINV = 128
BY_LEVEL = -1  # DAG_ORDER_BY_LEVEL
EVEN, LEAD, LAG = 0, 1, 2
LAUNCH = {EVEN: 96, LEAD: 80, LAG: 128}  # three slots on 256 compute units (tests/test_slot_share_cpu.py::test_default_launch_sizes)
CAP = 8000


@functools.lru_cache(maxsize=None)
def queue(nb, bk, nwg, order_wg, which, workers=0):
    """(tasks [n, 18], (makespan, wait, busy, sim_us, crit_us, acc128)) of one validated queue; never changed by a caller."""
    lib = _lib.load()
    fine = 1 | 8 | (16 if nb <= 20 else 0) | 32  # a fit's slots: right-looking, row-progressive up to 20 blocks, no split K^-1 sums
    big128 = 2 if nb >= 32 else 0
    nt = C.c_int()
    err = C.create_string_buffer(400)
    tasks = np.zeros((CAP, 18), dtype=np.int32)
    out = np.zeros(6)
    rc = lib.hbegp_debug_dag_replay(nb, bk, 4, nwg, order_wg, fine, big128, which, workers, C.byref(nt),
                                    tasks.ctypes.data_as(C.POINTER(C.c_int)), CAP, out.ctypes.data_as(C.POINTER(C.c_double)), err, 400)
    assert rc == 0, (nb, bk, nwg, order_wg, which, err.value.decode())  # the plan checker's verdict
    assert 0 < nt.value <= CAP
    tasks = tasks[: nt.value].copy()
    tasks.setflags(write=False)
    return tasks, tuple(out)


def default_order(q, share, nwg, nb, n_slots=3):
    return _lib.load().hbegp_debug_dag_order_wg(q, share, nwg, LAUNCH[EVEN], nb, n_slots)


def orders_for(nb, share):
    """Every order_wg the defaults give a launch of this share at this size, and the candidates of profiles/queue_order_sweep.txt."""
    nwg = LAUNCH[share]
    out = {default_order(q, share, nwg, nb) for q in range(3)} | {default_order(q, share, nwg, 32) for q in range(3)}
    out |= {1, 64, 72, 80, 88, 96, 200, BY_LEVEL}
    return sorted(o for o in out if o != 0 and o != nwg)


def multiset(a):
    return a[np.lexsort(a.T[::-1])]


@pytest.mark.parametrize("share", [EVEN, LEAD, LAG])
@pytest.mark.parametrize("bk", [16, 32])
@pytest.mark.parametrize("nb", [6, 8, 32])
def test_reordered_queues_are_sound_hold_the_same_tasks_and_replay_to_the_planners_makespan(nb, bk, share):
    nwg = LAUNCH[share]
    base = [queue(nb, bk, nwg, 0, which)[0] for which in range(3)]
    for order_wg in orders_for(nb, share):
        full, (_, _, _, sim_full, _, _) = queue(nb, bk, nwg, order_wg, 0)
        p1, (_, _, _, sim_p1, _, _) = queue(nb, bk, nwg, order_wg, 1)
        kv, _ = queue(nb, bk, nwg, order_wg, 2)
        what = (nb, bk, nwg, order_wg)
        # the same tasks -- kind, flags, tile, contraction range, waits and bumps -- as the queue ordered for the launch's own count
        for got, want in zip((full, p1, kv), base):
            assert got.shape == want.shape and np.array_equal(multiset(got), multiset(want)), what
        # the K^-1-only queue: the full plan's K^-1 tasks in its order (their waits are renumbered: compare the tiles)
        is_kinv = (full[:, 1] & DAGF_CKINV) != 0
        assert is_kinv.sum() > 0 and np.array_equal(kv[:, :6], full[is_kinv][:, :6]), what
        assert not np.any(p1[:, 1] & DAGF_CKINV)
        # the replay on the count the queue was ordered for is the list schedule itself
        workers = nwg if order_wg == BY_LEVEL else order_wg  # (the count-independent order carries the replay on the launch's count)
        for which, sim in ((0, sim_full), (1, sim_p1)):
            makespan, wait, busy, sim_again, crit, _ = queue(nb, bk, nwg, order_wg, which, workers)[1]
            assert sim_again == sim and abs(makespan - sim) <= 1e-6 * sim, (what, which, makespan, sim)
            assert crit <= makespan + 1e-9 and wait >= 0 and busy > 0
            assert makespan * min(workers, len(full)) >= busy + wait - 1e-6 * busy, (what, which)


@pytest.mark.parametrize("nb,bk", [(6, 16), (8, 32), (32, 16), (32, 32)])
def test_replay_of_todays_queue_on_its_own_count_is_sim_us_and_fewer_workers_take_longer(nb, bk):
    for which in (0, 1):
        tasks, (makespan, _, busy, sim, crit, _) = queue(nb, bk, 96, 0, which, 96)
        assert abs(makespan - sim) <= 1e-6 * sim and sim >= crit * (1 - 1e-9) > 0
        one = queue(nb, bk, 96, 0, which, 1)[1]
        assert abs(one[0] - busy) <= 1e-6 * busy and one[1] == 0  # one worker in a topological order never waits
        many = queue(nb, bk, 96, 0, which, len(tasks))[1]
        assert crit - 1e-6 <= many[0] <= makespan + 1e-6
        if nb == 32:  # work-bound: 292.8 / 201.7 CU x ms of tasks on half the workers
            assert queue(nb, bk, 96, 0, which, 48)[1][0] > 1.5 * makespan


@pytest.mark.parametrize("nb", [6, 8, 32])
def test_unset_and_below_the_size_gate_the_queues_are_the_planners_own(nb):
    lib = _lib.load()
    fine = 1 | 8 | (16 if nb <= 20 else 0) | 32
    big128 = 2 if nb >= 32 else 0
    for share, nwg in LAUNCH.items():
        for q in range(3):
            # one slot, or fewer blocks than the gate: the default is the launch's own count
            assert default_order(q, share, nwg, nb, 1) == 0
            if nb < 32:
                assert default_order(q, share, nwg, nb, 3) == 0
            else:  # measured (profiles/queue_order_sweep.txt): only the lag launch gains, ordered for the even launch's count
                assert default_order(q, share, nwg, nb, 3) == (LAUNCH[EVEN] if share == LAG else 0)
        for bk in (16, 32):
            for which in range(3):
                nt = C.c_int()
                err = C.create_string_buffer(400)
                old = np.zeros((CAP, 6), dtype=np.int32)
                rc = lib.hbegp_debug_dag_queues(nb, bk, 4, nwg, fine, big128, which, C.byref(nt), old.ctypes.data_as(C.POINTER(C.c_int)), CAP, err, 400)
                assert rc == 0, err.value.decode()
                own = queue(nb, bk, nwg, 0, which)[0]
                assert np.array_equal(own[:, :6], old[: nt.value]), (nb, bk, nwg, which)  # byte for byte the queue without an order_wg
                assert np.array_equal(own, queue(nb, bk, nwg, nwg, which)[0]), (nb, bk, nwg, which)


def test_abi_declares_the_hooks():
    import os
    import re

    text = open(os.path.join(os.path.dirname(_lib.HERE), "include", "hbegp.h")).read()
    for name in ("hbegp_debug_dag_replay", "hbegp_debug_dag_order_wg"):
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert proto and name in _lib.SIGNATURES, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
