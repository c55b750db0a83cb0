"""The forced task-queue configurations that reach the 128x128 tile (DAG_GEMM_128x128, csrc/dag_kernel.inc.hpp) at small n, shared
by tests/test_dag_plan_cpu.py (the queues really hold such tiles, in every class a case claims) and tests/test_gpu_big128.py
(what the tiles compute).

The engine reads the plan switches per problem, so forcing them builds the queues of the large problems -- HBEGP_DAG_BIG128
defaults to 2 for a fit's slots from 32 blocks on and for any problem from 64 -- at six to seventeen 128-blocks.  A plan is
  (name, environment that forces it, small_h, fine bits of hbegp_debug_dag_plan / _queues without bit 5).
A case is (plan, n, element types, classes of 128x128 task its full queue must hold).  The classes:
  plain  beta = 0, alpha = +1, no transposed operand, not a K^-1 tile
  ACC    beta = 1: the old values are fetched in the epilogue (HBEGP_DAG_BIG128 = 2 only)
  NEG    alpha = -1
  KM     an operand read with the contraction index along rows (DAGF_AKM / DAGF_BKM)
  CKINV  a tile of K^-1 = X^T X
"""
import numpy as np

DAG_GEMM_128x128 = 9
DAGF_AKM, DAGF_BKM, DAGF_NEG, DAGF_ACC, DAGF_CKINV = 8, 16, 32, 64, 128

# right-looking plan with the divide-and-conquer inverse: the default from 21 to 80 blocks (with BIG128 = 2 from 32 on for a fit)
RL_DC = ("rl-dc", dict(HBEGP_DAG="1", HBEGP_DAG_RL="1", HBEGP_DAG_PROG="0", HBEGP_DAG_SMALLH="4"), 4, 1 | 8)
# right-looking plan, inverse and K^-1 row by row: the default up to 20 blocks
RL_PROG = ("rl-prog", dict(HBEGP_DAG="1", HBEGP_DAG_RL="1", HBEGP_DAG_PROG="1", HBEGP_DAG_SMALLH="4"), 4, 1 | 8 | 16)
# the recursion that carries the inverse, every product in tiles / with the default 8-block small nodes (the default above 80 blocks)
REC_0 = ("rec-h0", dict(HBEGP_DAG="1", HBEGP_DAG_RL="0", HBEGP_DAG_SMALLH="0"), 0, 1)
REC_8 = ("rec-h8", dict(HBEGP_DAG="1", HBEGP_DAG_RL="0", HBEGP_DAG_SMALLH="8"), 8, 1)

F64, F32 = "float64", "float32"
ALL = ("plain", "ACC", "NEG", "KM", "CKINV")

# group A (and B at the sizes it names): one evaluation, one slot
EVAL_CASES = [
    (RL_DC, 700, (F64, F32), ALL),  # 6 blocks, ragged: the smallest size with every class
    (RL_DC, 768, (F64, F32), ALL),  # 6 whole blocks
    (RL_DC, 1100, (F64, F32), ALL),  # 9 blocks: an odd split
    (RL_DC, 1409, (F64, F32), ALL),  # 12 blocks, one row past a block edge
    (RL_PROG, 700, (F64, F32), ALL),
    (REC_0, 700, (F64, F32), ALL),
    (REC_8, 2100, (F64, F32), ALL),  # 17 blocks: the first size where small_h = 8 leaves 128x128 tiles outside K^-1
]
ORACLE_CASES = [(RL_DC, 700), (RL_DC, 1100), (REC_8, 2100)]  # group B
SOAK_CASE = (RL_DC, 1300, (F64, F32), ALL)  # group C: three slots, 11 blocks
FIT_CASE = (RL_DC, 768, (F64, F32), ALL)  # group D: a fit's three slots (no split K^-1 sums), fused and two-phase
# group E: 4 blocks, the plan this size gets by default (right-looking, row by row) with small nodes of two blocks
NOT_PD_CASE = (("rl-prog-h2", dict(HBEGP_DAG="1", HBEGP_DAG_MIN_BLOCKS="2", HBEGP_DAG_SMALLH="2"), 2, 1 | 8 | 16), 400, (F64, F32), ALL)
POOL_CASE = (RL_DC, 900, (F64, F32), ALL)  # group F: 8 blocks, one slot and three

# (case, several slots): every queue the GPU module launches
PLANNED = [(c, False) for c in EVAL_CASES] + [(SOAK_CASE, True), (FIT_CASE, True), (NOT_PD_CASE, False), (POOL_CASE, False), (POOL_CASE, True)]


def blocks(n):
    return (n + 127) // 128


def stage_depth(dtype):
    """Contraction elements per pipeline stage of the task-queue tiles (dag_stage_depth): task ranges are whole stages."""
    return 32 if np.dtype(dtype) == np.float32 else 16


def fine_bits(plan, several_slots):
    """Bit 5: no split K^-1 sums (HBEGP_DAG_LAUUM_SPLIT defaults to 0 for a problem with several slots)."""
    return plan[3] | (32 if several_slots else 0)


def env(plan, big128):
    """The environment of one forced problem: the plan, the tile shape, and the planner's own check of every queue it builds."""
    return dict(plan[1], HBEGP_DAG_BIG128=str(big128), HBEGP_DAG_VALIDATE="1")


def classes(tasks):
    """{class: number of 128x128 tasks in it} of an (ntasks, 6) array of (kind, flags, row0, col0, kbeg, kend)."""
    f = tasks[tasks[:, 0] == DAG_GEMM_128x128][:, 1]
    count = lambda mask: int(((f & mask) != 0).sum())  # noqa: E731
    return {"all": len(f), "plain": len(f) - count(DAGF_ACC | DAGF_NEG | DAGF_AKM | DAGF_BKM | DAGF_CKINV), "ACC": count(DAGF_ACC), "NEG": count(DAGF_NEG),
            "KM": count(DAGF_AKM | DAGF_BKM), "CKINV": count(DAGF_CKINV)}


def claimed(case_classes, which):
    """The classes a case's queue `which` must hold: 0 the full plan, 1 the plan without the K^-1 tiles (first phase of a line-search
    trial evaluated in two phases), 2 the K^-1 tiles alone, which all read both operands along rows."""
    keep = {0: ALL, 1: ("plain", "ACC", "NEG"), 2: ("KM", "CKINV")}[which]
    return tuple(c for c in case_classes if c in keep)
