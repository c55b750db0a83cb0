"""CPU: the share policy of a fit's slots (csrc/slot_share.hpp through hbegp_debug_slot_shares: which slot's next task-queue launch
gets the lead, the even or the lag share of the compute units, from the runs' progress alone), and the queues of the lead and lag
launch sizes (hbegp_debug_dag_queues): for every size the defaults and the measured candidates give, all three queues of an
evaluation pass the plan checker, and the K^-1-only queue is still the full plan's K^-1 tasks in their order."""
import ctypes as C

import numpy as np
import pytest

from hbetune_rs_amd import _lib

EVEN, LEAD, LAG = 0, 1, 2
HYST = 2  # SLOT_SHARE_HYSTERESIS
DAGF_CKINV = 128


def shares(running, done, maxeval=150, hysteresis=-1):
    lib = _lib.load()
    k = len(running)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    r, d = np.array(running, dtype=np.int32), np.array(done, dtype=np.int32)
    m = np.full(k, maxeval, dtype=np.int32) if np.isscalar(maxeval) else np.array(maxeval, dtype=np.int32)
    out = np.full(k, -1, dtype=np.int32)
    _lib.check(lib.hbegp_debug_slot_shares(k, ip(r), ip(d), ip(m), hysteresis, ip(out), 96, 256, None, None))
    return out.tolist()


def test_equal_progress_is_even():
    assert shares([1, 1, 1], [0, 0, 0]) == [EVEN] * 3
    assert shares([1, 1, 1], [70, 70, 70]) == [EVEN] * 3


@pytest.mark.parametrize("behind", [0, 1, 2])
def test_one_slot_behind_by_more_than_the_hysteresis_is_lag_and_the_others_lead(behind):
    done = [60, 80, 70]
    done[behind] = min(d for i, d in enumerate(done) if i != behind) - HYST - 1  # just more than HYST behind the next one
    want = [LEAD] * 3
    want[behind] = LAG
    assert shares([1, 1, 1], done) == want


def test_progress_exactly_at_the_hysteresis_and_ties_stay_even():
    assert shares([1, 1, 1], [50, 50 + HYST, 90]) == [EVEN] * 3       # the nearest slot is exactly HYST ahead
    assert shares([1, 1, 1], [50, 50 + HYST + 1, 90]) == [LAG, LEAD, LEAD]
    assert shares([1, 1, 1], [50, 50, 90]) == [EVEN] * 3                # two slots share the last place
    assert shares([1, 1, 1], [50, 90, 90]) == [LAG, LEAD, LEAD]         # a tie among the leaders changes nothing
    # the threshold is the argument, not a constant in the rule
    assert shares([1, 1, 1], [50, 55, 90], hysteresis=4) == [LAG, LEAD, LEAD]
    assert shares([1, 1, 1], [50, 54, 90], hysteresis=4) == [EVEN] * 3
    assert shares([1, 1, 1], [50, 55, 90], hysteresis=8) == [EVEN] * 3
    assert shares([1, 1, 1], [50, 51, 90], hysteresis=0) == [LAG, LEAD, LEAD]


def test_finished_slots_are_ignored():
    # slot 0 is over (far behind on paper): the other two decide between themselves
    assert shares([0, 1, 1], [10, 40, 90]) == [EVEN, LAG, LEAD]
    assert shares([0, 1, 1], [10, 88, 90]) == [EVEN, EVEN, EVEN]
    # a run at its cap counts as finished whatever the flag says
    assert shares([1, 1, 1], [150, 40, 90]) == [EVEN, LAG, LEAD]
    assert shares([1, 1, 1], [30, 40, 90], maxeval=[30, 150, 150]) == [EVEN, LAG, LEAD]


def test_two_running_slots_behave_the_same_way():
    assert shares([1, 1], [10, 10 + HYST + 1]) == [LAG, LEAD]
    assert shares([1, 1], [10 + HYST + 1, 10]) == [LEAD, LAG]
    assert shares([1, 1], [10, 10 + HYST]) == [EVEN, EVEN]
    assert shares([1, 1], [10, 10]) == [EVEN, EVEN]


def test_one_running_slot_is_even():
    assert shares([1], [3]) == [EVEN]
    assert shares([0, 1, 0], [100, 3, 100]) == [EVEN] * 3
    assert shares([0, 0, 0], [1, 2, 3]) == [EVEN] * 3
    assert shares([1, 1, 1], [150, 3, 150]) == [EVEN] * 3


def test_the_policy_is_a_function_of_its_arguments():
    rng = np.random.default_rng(7)
    for _ in range(200):
        k = int(rng.integers(1, 7))
        running, done = rng.integers(0, 2, k).tolist(), rng.integers(0, 160, k).tolist()
        a = shares(running, done)
        assert a == shares(running, done)
        live = [i for i in range(k) if running[i] and done[i] < 150]
        assert all(a[i] == EVEN for i in range(k) if i not in live)
        assert a.count(LAG) <= 1
        if LAG in a:
            lag = a.index(LAG)
            assert len(live) >= 2 and all(a[i] == LEAD and done[i] - done[lag] > HYST for i in live if i != lag)
        else:
            assert LEAD not in a


def default_sizes(even_wg, n_slots, cus=256):
    lib = _lib.load()
    one = np.ones(n_slots, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    lead, lag = C.c_int(), C.c_int()
    _lib.check(lib.hbegp_debug_slot_shares(n_slots, ip(one), ip(one), ip(one), -1, ip(one.copy()), even_wg, cus, C.byref(lead), C.byref(lag)))
    return lead.value, lag.value


def test_default_launch_sizes():
    assert default_sizes(96, 3) == (80, 128)    # three slots on 256 compute units: 2 x 80 + 128 = 3 x 96
    assert default_sizes(144, 2) == (128, 160)  # two slots
    for even, k in ((96, 3), (144, 2), (72, 4)):
        lead, lag = default_sizes(even, k)
        assert lead % 8 == 0 and lag % 8 == 0 and (k - 1) * lead + lag == k * even and lead < even < lag
    assert default_sizes(8, 3) == (8, 40) and default_sizes(256, 2) == (240, 256)  # clipped to [8, compute units]


def queue(nb, bk, nwg, fine, big128, which):
    lib = _lib.load()
    nt = C.c_int()
    err = C.create_string_buffer(400)
    cap = 40000
    tasks = np.zeros((cap, 6), dtype=np.int32)
    rc = lib.hbegp_debug_dag_queues(nb, bk, 4, nwg, fine, big128, which, C.byref(nt), tasks.ctypes.data_as(C.POINTER(C.c_int)), cap, err, 400)
    assert nt.value <= cap
    return rc, tasks[: nt.value].copy(), err.value.decode()


# lead and lag sizes: the defaults for three and for two slots, and the measured candidates (profiles/run_balance_sweep.txt)
SHARE_NWG = sorted({*default_sizes(96, 3), *default_sizes(144, 2), 88, 104, 112, 80, 128, 72, 144})


@pytest.mark.parametrize("nb", [6, 8, 32])
def test_lead_and_lag_queues_are_sound_and_keep_the_kinv_order(nb):
    fine = 1 | 8 | (16 if nb <= 20 else 0) | 32  # a fit's slots: right-looking, row-progressive up to 20 blocks, no split K^-1 sums
    big128 = 2 if nb >= 32 else 0
    key = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
    for bk in (16, 32):  # stage depth of f64 / f32
        rc, even_full, e = queue(nb, bk, 96, fine, big128, 0)
        assert rc == 0, e
        for nwg in SHARE_NWG:
            rc0, full, e0 = queue(nb, bk, nwg, fine, big128, 0)
            rc1, p1, e1 = queue(nb, bk, nwg, fine, big128, 1)
            rc2, kv, e2 = queue(nb, bk, nwg, fine, big128, 2)
            assert (rc0, rc1, rc2) == (0, 0, 0), (nb, bk, nwg, e0, e1, e2)
            is_kinv = (full[:, 1] & DAGF_CKINV) != 0
            assert is_kinv.sum() > 0
            assert np.array_equal(kv, full[is_kinv]), (nb, bk, nwg)  # the full plan's K^-1 tasks, in its order
            assert not np.any(p1[:, 1] & DAGF_CKINV)
            assert np.array_equal(key(p1), key(full[~is_kinv])), (nb, bk, nwg)
            # the same task set as the even launch's: only the queue order and the workgroup count differ
            assert np.array_equal(key(full), key(even_full)), (nb, bk, nwg)


def test_abi_declares_the_hooks():
    import os
    import re

    text = open(os.path.join(os.path.dirname(_lib.HERE), "include", "hbegp.h")).read()
    for name in ("hbegp_debug_slot_shares", "hbegp_debug_fits_in_flight"):
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert proto and name in _lib.SIGNATURES, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"#define HBEGP_STATS_MAX_RUNS\s+(\d+)", text).group(1) == str(_lib.STATS_MAX_RUNS)
