"""CPU: the rule by which a 128x128 task-queue tile skips structurally zero operand halves (csrc/engine.hpp: dag_zero_halves, through
hbegp_debug_dag_zero_halves; HBEGP_DAG_ZERO_SKIP).

An operand that lives in W2 is read out of X = L^-1, whose strict upper triangle is zero in memory.  The rule names, per side (A, B)
and 64-wide half, the leading and the trailing stages of a task's contraction range in which that half lies wholly above the
diagonal; the waves that own the half drop their MFMAs there.  What the device cannot assert is that every element the rule lets a
wave skip is such a zero -- so every sub-block it names, in the forced queues of tests/big128_cases.py (6, 8, 9, 11, 12 and 17
blocks, both stage depths) and in the 32-block queues of the flagship fit, is walked element by element here.
"""
import ctypes as C

import numpy as np
import pytest

import big128_cases as BC
from hbetune_rs_amd import _lib

DAGF_ABUF, DAGF_BBUF, DAGF_CBUF, DAGF_A3, DAGF_B3, DAGF_C3 = 1, 2, 4, 256, 512, 1024
SIDES = ((DAGF_ABUF, DAGF_A3, BC.DAGF_AKM, 2), (DAGF_BBUF, DAGF_B3, BC.DAGF_BKM, 3))  # (in W2, in W3, read along rows, origin's column in a task row)


def queue(nb, bk, small_h, nwg, fine, big128, which):
    lib = _lib.load()
    nt, err, cap = C.c_int(), C.create_string_buffer(400), 40000
    tasks = np.zeros((cap, 6), dtype=np.int32)
    rc = lib.hbegp_debug_dag_queues(nb, bk, small_h, nwg, fine, big128, which, C.byref(nt), tasks.ctypes.data_as(C.POINTER(C.c_int)), cap, err, 400)
    assert rc == 0 and nt.value <= cap, err.value.decode()
    return tasks[: nt.value].copy()


def rule(flags, row0, col0, kbeg, kend, bk):
    """(lead, trail): arrays [side][half] of whole stages."""
    out = (C.c_int * 8)()
    assert _lib.load().hbegp_debug_dag_zero_halves(int(flags), int(row0), int(col0), int(kbeg), int(kend), int(bk), out) == 0
    v = np.array(list(out)).reshape(2, 2, 2)
    return v[0], v[1]


def above_diagonal(task, side, half, bk):
    """Brute force over element coordinates: per stage, every element that `half` of `side` reads lies strictly above the diagonal
    of the operand's matrix."""
    _, flags, _, _, kbeg, kend = (int(v) for v in task)
    origin = int(task[SIDES[side][3]]) + 64 * half
    outer, k = np.meshgrid(np.arange(origin, origin + 64), np.arange(kbeg, kend), indexing="ij")
    i, j = (k, outer) if flags & SIDES[side][2] else (outer, k)  # read along rows: the contraction index is the matrix row
    return (j > i).reshape(64, (kend - kbeg) // bk, bk).all(axis=(0, 2))


def check_queue(tasks, bk, what):
    """Walks every 128x128 task of a queue; returns its half-zero stages and the tasks that have any."""
    n_stages = n_tasks = 0
    sides = np.zeros((2, 2), dtype=int)  # [side][lead / trail]
    for task in tasks[tasks[:, 0] == BC.DAG_GEMM_128x128]:
        _, flags, row0, col0, kbeg, kend = (int(v) for v in task)
        nst = (kend - kbeg) // bk
        assert nst >= 1 and (kend - kbeg) % bk == 0, (what, task)
        lead, trail = rule(flags, row0, col0, kbeg, kend, bk)
        for side, (buf, three, _, _) in enumerate(SIDES):
            in_w2 = bool(flags & buf) and not flags & three
            if not in_w2:
                assert not lead[side].any() and not trail[side].any(), (what, task, side)
                continue
            zero = np.zeros((2, nst), dtype=bool)  # brute force: [half][stage] lies wholly, strictly above the diagonal
            for half in (0, 1):
                zero[half] = above_diagonal(task, side, half, bk)
                named = np.zeros(nst, dtype=bool)
                named[: lead[side][half]] = True
                named[nst - trail[side][half]:] = trail[side][half] > 0
                # every sub-block the rule names is zero, and the rule misses none that is
                assert np.array_equal(named, zero[half]), (what, task, side, half, lead[side][half], trail[side][half])
            assert not (zero[0] & zero[1]).any(), (what, task, side)  # never both halves of a side: somebody always has work
            sides[side] += [lead[side].sum(), trail[side].sum()]
        z = int(lead.sum() + trail.sum())
        n_stages += z
        n_tasks += z > 0
    return n_stages, n_tasks, sides


@pytest.mark.parametrize("case,several_slots", [pytest.param(c, m, id=f"{c[0][0]}-n{c[1]}-{'fit' if m else 'one'}") for c, m in BC.PLANNED])
def test_every_half_the_rule_names_lies_above_the_diagonal_in_the_forced_queues(case, several_slots):
    (name, _, small_h, _), n, dtypes, _ = case
    for dtype in dtypes:
        bk = BC.stage_depth(dtype)
        for which in (0, 1, 2):
            tasks = queue(BC.blocks(n), bk, small_h, 96, BC.fine_bits(case[0], several_slots), 2, which)
            n_stages, _, _ = check_queue(tasks, bk, (name, n, dtype, which))
            assert n_stages > 0, (name, n, dtype, which)  # (every forced queue has such stages: the check is not vacuous)


def test_the_flagship_queues_and_their_counts():
    # the three queues of a 32-block fit slot on 96 workgroups (right-looking plan, divide-and-conquer inverse, no split K^-1 sums,
    # 128x128 tiles also with beta = 1): phase 1, fused, K^-1 alone -- half-zero stages and the tasks that hold them, as counted when
    # the skip was proposed
    want = {1: (4804, 1201), 0: (6788, 1697), 2: (1984, 496)}
    for which, (stages, n_tasks) in want.items():
        tasks = queue(32, 16, 4, 96, 1 | 8 | 32, 2, which)
        got_stages, got_tasks, sides = check_queue(tasks, 16, ("flagship", which))
        assert (got_stages, got_tasks) == (stages, n_tasks), (which, got_stages, got_tasks, sides.tolist())


def test_only_operands_in_w2_are_triangular():
    # geometries in which a half WOULD be zero (rows 0.. against a range that ends far right; columns 512.. read along rows against
    # a range that starts at 0): the rule answers only for DAGF_ABUF / DAGF_BBUF without DAGF_A3 / DAGF_B3 -- W1, W3 and the K^-1
    # buffer (an output only: DAGF_CKINV names no operand) hold full matrices
    for bk in (16, 32):
        for out_flags in (0, DAGF_CBUF, DAGF_C3, BC.DAGF_CKINV, BC.DAGF_NEG | BC.DAGF_ACC):
            for km in (0, 1):
                geom = (512, 512, 0, 512) if km else (0, 0, 0, 512)
                for side, (buf, three, kmflag, _) in enumerate(SIDES):
                    for place, triangular in ((0, False), (buf, True), (three, False), (buf | three, False)):
                        lead, trail = rule(place | (kmflag if km else 0) | out_flags, *geom, bk)
                        assert not lead[1 - side].any() and not trail[1 - side].any()
                        if triangular:
                            assert (trail[side] if not km else lead[side]).all() and not (lead[side] if not km else trail[side]).any()
                        else:
                            assert not lead[side].any() and not trail[side].any(), (bk, out_flags, km, side, place)
    # an empty or negative range names nothing
    lead, trail = rule(DAGF_ABUF | DAGF_BBUF, 0, 0, 256, 256, 16)
    assert not lead.any() and not trail.any()
