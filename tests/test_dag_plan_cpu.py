"""CPU: the task queue of the device-scheduled factorisation (csrc/dag_plan.hpp) is sound for every shape the engine
builds -- queue order topological (so any number of resident workgroups makes progress: no deadlock by construction),
every wait for a full count, no unordered access to a tile of W1/W2 -- and the checker itself catches broken plans."""
import ctypes as C
import os

import numpy as np
import pytest

import big128_cases as BC
from hbetune_rs_amd import _lib


def plan(nb, bk=16, small_h=8, nwg=85, fine=1):
    lib = _lib.load()
    nt, nc, nl = C.c_int(), C.c_int(), C.c_int()
    gf, cr, sm = C.c_double(), C.c_double(), C.c_double()
    err = C.create_string_buffer(400)
    rc = lib.hbegp_debug_dag_plan(nb, bk, small_h, nwg, fine, C.byref(nt), C.byref(nc), C.byref(nl), C.byref(gf), C.byref(cr),
                                  C.byref(sm), err, 400)
    return rc, dict(ntasks=nt.value, ncounters=nc.value, nleaf=nl.value, gflop=gf.value, crit_us=cr.value, sim_us=sm.value,
                    err=err.value.decode())


@pytest.mark.parametrize("nb", list(range(1, 20)) + [24, 31, 32, 33, 48, 64])
def test_plans_are_sound_for_every_block_count(nb):
    ref = None
    for bk in (16, 32):
        for small_h, nwg, fine in [(8, 85, 1), (2, 256, 1), (0, 1, 1), (64, 7, 1), (8, 0, 1), (8, 85, 0), (2, 0, 0)]:
            rc, info = plan(nb, bk, small_h, nwg, fine)
            assert rc == 0, (nb, bk, small_h, nwg, fine, info["err"])
            assert info["nleaf"] == nb
            ref = ref or info["gflop"]
            assert info["gflop"] == pytest.approx(ref, rel=1e-12)  # the work does not depend on tiling, order or dependencies
            if nwg > 0 and nb > 1:
                assert info["crit_us"] > 0 and info["sim_us"] >= info["crit_us"] - 1e-6


def test_flops_match_potrf_plus_trtri():
    # n = 4096: the recursion carries n^3/3 (Cholesky) + n^3/3 (inverse of the factor) minus what the half-counted
    # triangles save; LAUUM (the last third, 22.9 GFLOP) is a separate launch.  DESIGN.md quotes 68.7 - 22.95 = 45.8.
    rc, info = plan(32)
    assert rc == 0 and info["gflop"] == pytest.approx(45.77, abs=0.02)


@pytest.mark.parametrize("nb", [1, 2, 3, 5, 8, 11, 16, 24, 32, 33, 64])
def test_plans_with_the_inverse_tiles_are_sound(nb):
    # fine bit 2: K^-1 = X^T X as tile tasks behind the recursion (the default form of an evaluation)
    for bk in (16, 32):
        for small_h, nwg in [(8, 85), (2, 256), (8, 0), (0, 3)]:
            rc, info = plan(nb, bk, small_h, nwg, fine=1 | 4)
            assert rc == 0, (nb, bk, small_h, nwg, info["err"])


def test_flops_with_the_inverse_tiles_are_potrf_plus_potri():
    # n^3 = 68.7 GFLOP at n = 4096, of which lauum 22.95 (as Problem::op_gflop counts the launch it replaces)
    rc, info = plan(32, fine=1 | 4)
    assert rc == 0 and info["gflop"] == pytest.approx(45.77 + 22.95, abs=0.03)


@pytest.mark.parametrize("nb", list(range(1, 14)) + [16, 17, 24, 31, 32, 33, 48, 64, 80])
def test_right_looking_plans_are_sound_for_every_block_count(nb):
    # fine bit 3: the default plan (right-looking tile Cholesky + divide-and-conquer inverse), with and without the K^-1 tiles
    ref = None
    for bk in (16, 32):
        for small_h, nwg, fine in [(4, 96, 1 | 4 | 8), (4, 256, 1 | 4 | 8), (8, 0, 1 | 8), (0, 3, 1 | 4 | 8), (4, 85, 4 | 8)]:
            rc, info = plan(nb, bk, small_h, nwg, fine)
            assert rc == 0, (nb, bk, small_h, nwg, fine, info["err"])
            assert info["nleaf"] == nb
            if fine & 4:
                ref = ref or info["gflop"]
                assert info["gflop"] == pytest.approx(ref, rel=1e-12)
    # same algorithmic work as the recursion plan, whatever the order of operations
    rc, rec = plan(nb, 16, 8, 85, 1 | 4)
    assert rc == 0 and (ref is None or rec["gflop"] == pytest.approx(ref, rel=1e-12))


@pytest.mark.parametrize("nb", list(range(1, 14)) + [16, 17, 20, 24, 31, 32, 33, 48])
def test_row_progressive_plans_are_sound_for_every_block_count(nb):
    # fine bit 4: right-looking plan whose inverse of the factor and K^-1 follow the diagonal chain row by row (round 4; the
    # default up to 20 blocks): same flops as the divide and conquer, sound for every ordering
    _, dc = plan(nb, 16, 4, 96, 1 | 4 | 8)
    for bk in (16, 32):
        for small_h, nwg, fine in [(4, 96, 1 | 4 | 8 | 16), (4, 256, 1 | 4 | 8 | 16), (8, 0, 1 | 8 | 16), (0, 3, 1 | 4 | 8 | 16), (4, 85, 4 | 8 | 16)]:
            rc, info = plan(nb, bk, small_h, nwg, fine)
            assert rc == 0, (nb, bk, small_h, nwg, fine, info["err"])
            assert info["nleaf"] == nb
            if fine & 4:
                assert info["gflop"] == pytest.approx(dc["gflop"], rel=1e-12)


def test_row_progressive_plan_leaves_little_behind_the_last_diagonal_block():
    # n = 2048 on 256 workgroups: with the divide-and-conquer inverse a third of the flops can only start when the chain of
    # diagonal blocks has ended; row by row the critical path and the simulated makespan are shorter
    _, dc = plan(16, small_h=4, nwg=256, fine=1 | 4 | 8)
    _, pr = plan(16, small_h=4, nwg=256, fine=1 | 4 | 8 | 16)
    assert pr["crit_us"] < 0.9 * dc["crit_us"] and pr["sim_us"] < 0.9 * dc["sim_us"]


@pytest.mark.parametrize("fault", ["drop:40", "drop:700", "drop:2000", "drop:2900", "move:2500:10", "move:900:100"])
def test_checker_rejects_broken_row_progressive_plans(fault, monkeypatch):
    monkeypatch.setenv("HBEGP_DAG_TEST_FAULT", fault)
    rc, info = plan(16, small_h=4, nwg=96, fine=1 | 4 | 8 | 16)
    assert rc == _lib.EINVAL and info["err"], fault


def test_right_looking_plan_shortens_the_critical_path():
    # n = 4096: between two diagonal blocks the recursion has a product as deep as the node is wide, the right-looking plan
    # two 128-deep tiles (2.83 -> 2.03 ms simulated, 2.89 -> 2.19 ms measured for one evaluation)
    _, rec = plan(32, nwg=256, fine=1 | 4)
    _, rl = plan(32, small_h=4, nwg=256, fine=1 | 4 | 8)
    assert rl["crit_us"] < 0.8 * rec["crit_us"] and rl["sim_us"] < 0.85 * rec["sim_us"]
    assert rl["gflop"] == pytest.approx(68.72, abs=0.02)


@pytest.mark.parametrize("fault", ["drop:40", "drop:700", "drop:3000", "drop:7000", "move:5000:10", "move:900:100"])
def test_checker_rejects_broken_right_looking_plans(fault, monkeypatch):
    monkeypatch.setenv("HBEGP_DAG_TEST_FAULT", fault)
    rc, info = plan(32, small_h=4, nwg=96, fine=1 | 4 | 8)
    assert rc == _lib.EINVAL and info["err"], fault


def test_look_ahead_shortens_the_simulated_schedule():
    _, fine = plan(32, nwg=85, fine=1)
    _, coarse = plan(32, nwg=85, fine=0)
    assert fine["sim_us"] < 0.85 * coarse["sim_us"]


@pytest.mark.parametrize("fault", ["drop:40", "drop:200", "drop:900", "drop:2500", "move:3000:10", "move:500:100"])
def test_checker_rejects_broken_plans(fault, monkeypatch):
    monkeypatch.setenv("HBEGP_DAG_TEST_FAULT", fault)
    rc, info = plan(32)
    assert rc == _lib.EINVAL and info["err"], fault


def test_plan_builder_and_optimiser_are_clean_under_sanitizers(tmp_path):
    # host code of the hot path (csrc/dag_plan.hpp: both plans, 1..40 blocks, validator; csrc/lbfgsb.hpp: gradmin.rs:75-101 KAT)
    # compiled with AddressSanitizer + UndefinedBehaviorSanitizer -- sanitizers run on the CPU build only
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "san_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", os.path.join(root, "csrc"),
                           "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", os.path.join(root, "tools", "san_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 problems" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("nb", [2, 3, 5, 8, 16, 24, 32, 33, 48])
def test_plans_with_128x128_tiles_are_sound(nb, monkeypatch):
    # HBEGP_DAG_BIG128 = 1: the deep products without beta = 1 as 128x128 tiles; 2 (the default for a fit's slots from 32 blocks on and
    # for any problem from 64): the beta = 1 products too, whose old values the tile fetches in its epilogue.  Fewer tasks, the same
    # flops, sound in every plan -- and never a 128x128 task that continues a sum (DAGF_CINIT: the checker rejects one)
    _, base = plan(nb, 16, 4, 96, 1 | 4 | 8)
    fewer = base["ntasks"]
    for big128 in (1, 2):
        monkeypatch.setenv("HBEGP_DAG_BIG128", str(big128))
        for bk in (16, 32):
            for small_h, nwg, fine in [(4, 96, 1 | 4 | 8), (4, 256, 1 | 4 | 8 | 16), (8, 85, 1 | 4), (0, 3, 1 | 4 | 8)]:
                rc, info = plan(nb, bk, small_h, nwg, fine)
                assert rc == 0, (nb, big128, bk, small_h, nwg, fine, info["err"])
                assert info["gflop"] == pytest.approx(base["gflop"], rel=1e-12)
        if nb >= 8:
            _, big = plan(nb, 16, 4, 96, 1 | 4 | 8)
            assert big["ntasks"] < fewer  # 1: fewer tasks than 128x64 tiles alone; 2: fewer again
            fewer = big["ntasks"]


def queue(nb, bk, small_h, nwg, fine, big128, which):
    lib = _lib.load()
    nt = C.c_int()
    err = C.create_string_buffer(400)
    cap = 40000
    tasks = np.zeros((cap, 6), dtype=np.int32)
    rc = lib.hbegp_debug_dag_queues(nb, bk, small_h, nwg, fine, big128, which, C.byref(nt), tasks.ctypes.data_as(C.POINTER(C.c_int)), cap, err, 400)
    assert nt.value <= cap
    return rc, tasks[: nt.value].copy(), err.value.decode()


@pytest.mark.parametrize("case,several_slots", [pytest.param(c, m, id=f"{c[0][0]}-n{c[1]}-{'fit' if m else 'one'}") for c, m in BC.PLANNED])
def test_the_forced_gpu_cases_hold_128x128_tiles_of_every_class_they_claim(case, several_slots):
    # What the device cannot assert: that the small problems tests/test_gpu_big128.py forces really run the tile.  Each of its
    # configurations with its own (blocks, stage depth, small_h, fine bits), at the launch sizes it uses (all workgroups of one slot,
    # a fit's even / lead / lag shares, the forced 3, 40 and 128): the full queue and the two queues of a trial evaluated in two
    # phases pass the checker and hold at least one 128x128 task of every claimed class; BIG128 = 1 has the same tasks without
    # beta = 1, and BIG128 = 0 none at all.
    (name, _, small_h, _), n, dtypes, want = case
    nb, fine = BC.blocks(n), BC.fine_bits(case[0], several_slots)
    for dtype in dtypes:
        bk = BC.stage_depth(dtype)
        sets = {}
        for nwg in (256, 96, 72, 128, 3, 40):
            for which in (0, 1, 2):
                rc, tasks, err = queue(nb, bk, small_h, nwg, fine, 2, which)
                assert rc == 0, (name, n, dtype, nwg, which, err)
                got = BC.classes(tasks)
                for cls in BC.claimed(want, which):
                    assert got[cls] > 0, (name, n, dtype, nwg, which, cls, got)
                # the launch size orders the queue, it does not choose the tiles
                assert sets.setdefault(which, got) == got, (name, n, dtype, nwg, which)
        for which in (0, 1, 2):
            rc, one, err = queue(nb, bk, small_h, 96, fine, 1, which)
            assert rc == 0, (name, n, dtype, which, err)
            got = BC.classes(one)
            assert got["ACC"] == 0 and got["all"] == sets[which]["all"] - sets[which]["ACC"], (name, n, dtype, which, got)
            rc, none, err = queue(nb, bk, small_h, 96, fine, 0, which)
            assert rc == 0 and BC.classes(none)["all"] == 0, (name, n, dtype, which, err)


def test_the_issue_table_of_128x128_task_counts():
    # the counts the cases were chosen by (f64, 96 workgroups, one slot): 128x128 tasks, then those with beta = 1, alpha = -1, an
    # operand read along rows, and the K^-1 tiles -- 6 blocks is the smallest size with every class, 17 the first at which the
    # recursion with small nodes of 8 blocks has such tiles outside K^-1
    table = [(BC.RL_DC, 4, (11, 2, 2, 6, 6)), (BC.RL_DC, 6, (38, 13, 13, 15, 15)), (BC.RL_DC, 9, (149, 49, 65, 72, 36)), (BC.RL_PROG, 6, (68, 13, 28, 45, 15)),
             (BC.REC_8, 16, (120, 0, 0, 120, 120)), (BC.REC_8, 17, (372, 36, 100, 272, 136)), (BC.REC_0, 6, (51, 5, 13, 38, 15))]
    for p, nb, want in table:
        rc, tasks, err = queue(nb, 16, p[2], 96, p[3], 2, 0)
        got = BC.classes(tasks)
        assert rc == 0 and (got["all"], got["ACC"], got["NEG"], got["KM"], got["CKINV"]) == want, (p[0], nb, got, err)
