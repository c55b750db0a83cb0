"""CPU: the guard of tests/test_gpu_paths_sizes.py ("The size-dependent splits under test").

Every row of tests/paths_size_cases.py must reach the split its name stands for -- asked of the library through
hbegp_debug_paths_eval_blocks and hbegp_debug_paths_project_chunks, which answer from the functions the engine itself calls -- so
that a constant that moves makes this module fail instead of silently turning a case into one more single-block, 64-feature-chunk
run.  The chunk rule is also swept for soundness: that is the only cover of cap = 1 (n >= 16384 at S = 1024), which no quick GPU
test can reach.  The restatement's matrix-product evaluation, which the GPU module is judged against, is held to its einsum form."""
import ctypes as C
import math

import numpy as np
import pytest

import paths_ref as PR
import paths_size_cases as PC
from hbetune_rs_amd import _lib

MIB = 1 << 20


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.name)
def test_every_case_reaches_its_split(case):
    assert PC.blocks_of(case) == case.blocks and sum(case.blocks) == case.m
    cap, nch, fch = PC.project_chunks(case.F, case.n, case.S)
    assert (cap, nch, fch) == (case.cap, case.nch, case.fch)
    assert case.F - (nch - 1) * fch == case.last and 1 <= case.last <= fch
    assert case.nu == PC.NUS[PC.CASES.index(case) % 4]


def test_the_table_covers_the_four_splits():
    by = PC.BY_NAME
    multi = [c for c in PC.CASES if len(c.blocks) > 1]
    assert {c.name for c in multi} == {"rows-shared", "rows-per-path", "part-cap"}
    for c in multi:  # at least three blocks, a last one that is shorter, and pieces that are single blocks off the block edges
        assert len(c.blocks) >= 3 and c.blocks[-1] < c.blocks[0]
        for a, b in PC.slices(c.m, c.blocks[0]):
            assert PC.blocks_of(c, b - a) == (b - a,)
    # which bound decides mb: the pairs (262144 / S) for the two rows cases, the partial sums (256 MiB) for part-cap
    for name in ("rows-shared", "rows-per-path"):
        c = by[name]
        assert c.blocks[0] == 262144 // c.S
    c = by["part-cap"]
    per_point = 8 * (math.ceil(c.n / 512) + math.ceil(c.F / 512)) * c.S * (c.d + 1)
    assert c.blocks[0] == (256 * MIB) // per_point < 262144 // c.S
    assert math.ceil(c.d / 8) == 3  # three gradient passes
    # the round of the minimiser on part-cap's handle
    assert PC.eval_blocks(c.n, c.d, c.F, c.S, PC.ROUND_STARTS) == PC.ROUND_BLOCKS
    # chunks: fch > 64 with a last tile of 4 features under a cap below 64; with a last chunk of 2 tiles + 1; cap = nch = 4
    c = by["fch96-capped"]
    assert c.cap < 64 and c.fch == 96 and c.last % PC.PP_FT == 4 and c.last > 2 * PC.PP_FT
    c = by["fch96"]
    assert c.cap == 64 and c.fch == 96 and c.last == 2 * PC.PP_FT + 1
    c = by["cap4"]
    assert c.cap == c.nch == 4 and c.fch == 256 and c.n > 128 * 8
    assert by["tiny-F1-S1"].last < PC.PP_FT and by["tiny-F33-S3"].last == PC.PP_FT + 1
    # more than 64 paths and several 128-row blocks of the [S_p][n_p] operand, in both element types (every case runs in both)
    assert sum(c.S > 128 for c in PC.CASES) >= 5
    assert by["rows-shared"].S == _lib.PATHS_MAX_PATHS and by["part-cap"].F == _lib.PATHS_MAX_FEATURES  # the limits are accepted


def _sweep_F():
    rng = np.random.default_rng(14)
    return sorted(set(range(1, 131)) | set(range(4095, 4201)) | {16384} | set(int(v) for v in rng.integers(1, 16385, 300)))


@pytest.mark.parametrize("n", [1, 100, 300, 4096, 20000])
@pytest.mark.parametrize("S", [1, 64, 65, 1000, 1024])
def test_the_chunk_rule_is_sound(S, n):
    per_chunk = 8 * S * n
    for F in _sweep_F():
        cap, nch, fch = PC.project_chunks(F, n, S)
        # the chunks [c fch, min(F, (c + 1) fch)) cover [0, F) exactly once: nch - 1 full ones and a last one that is not empty
        assert nch >= 1 and (nch - 1) * fch < F <= nch * fch, (F, n, S, cap, nch, fch)
        assert fch % PC.PP_FT == 0 and fch >= PC.PP_FT
        assert nch <= 64 and nch <= cap
        assert cap == max(1, min(64, (128 * MIB) // per_chunk))
        if per_chunk <= 128 * MIB:
            assert nch * per_chunk <= 128 * MIB
        else:
            assert cap == 1 and nch == 1 and fch >= F  # one chunk, whatever it takes
        for d in (1, 17, 64):
            for m in (0, 1, 9, 100000):
                mb = PC.eval_block(n, d, F, S, m)
                assert mb >= 1 and (mb <= m or m == 0) and mb * S <= max(262144, S)


def test_cap_one_is_reached_by_the_sweep_only():
    cap, nch, fch = PC.project_chunks(16384, 16384, 1024)
    assert (cap, nch, fch) == (1, 1, 16384)
    assert PC.project_chunks(16384, 16383, 1024)[0] == 1 and PC.project_chunks(16384, 8192, 1024)[0] == 2
    assert max(c.n for c in PC.CASES) < 16384


def test_the_queries_refuse_what_the_entry_points_refuse():
    lib = _lib.load()
    v = C.c_int(7)
    for args, what in (((0, 2, 8, 1, 4), "n must be"), ((10, 0, 8, 1, 4), "d must be"), ((10, 2, 0, 1, 4), "F must be in"),
                       ((10, 2, _lib.PATHS_MAX_FEATURES + 1, 1, 4), "F must be in"), ((10, 2, 8, 0, 4), "S must be in"),
                       ((10, 2, 8, _lib.PATHS_MAX_PATHS + 1, 4), "S must be in"), ((10, 2, 8, 1, -1), "m must be")):
        assert lib.hbegp_debug_paths_eval_blocks(*args, C.byref(v)) == _lib.EINVAL and what in _lib.last_error(), args
    assert lib.hbegp_debug_paths_eval_blocks(10, 2, 8, 1, 4, None) == _lib.EINVAL and "NULL" in _lib.last_error()
    for args, what in (((0, 10, 1), "F must be in"), ((8, 0, 1), "n must be"), ((8, 10, 0), "S must be in")):
        assert lib.hbegp_debug_paths_project_chunks(*args, C.byref(v), None, None) == _lib.EINVAL and what in _lib.last_error(), args
    assert v.value == 7  # nothing was written
    assert lib.hbegp_debug_paths_project_chunks(100, 10, 3, None, None, None) == _lib.OK


@pytest.mark.parametrize("nu", PC.NUS)
def test_matrix_product_evaluation_is_the_restatement(nu):
    """paths_ref.Paths.evaluate_by_matmul (one product per gradient component; the einsum of `evaluate` is cubic at S = 1000,
    F = 16384) against `evaluate`, shared points, and through `gather` per path."""
    rng = np.random.default_rng(3)
    n, d, F, S, m = 40, 5, 70, 6, 11
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1)
    ref = PR.Paths(X, y, 1.3, np.linspace(0.3, 0.9, d), nu, 0.05, rng.standard_normal((F, d)), rng.uniform(0, 6, F),
                   rng.standard_normal((S, F)), rng.standard_normal((S, n)))
    x = rng.uniform(-0.1, 1.1, (m, d))
    x[3] = X[7]  # r = 0 at a training point
    f, df = ref.evaluate(x)
    f2, df2 = ref.evaluate_by_matmul(x)
    assert np.abs(f2 - f).max() <= 1e-13 * max(1.0, np.abs(f).max())
    assert np.abs(df2 - df).max() <= 1e-13 * max(1.0, np.abs(df).max())
    idx = rng.integers(0, m, (S, 8))
    fp, dfp = ref.evaluate(x[idx])
    gf, gdf = PR.gather(f2, df2, idx)
    assert np.abs(gf - fp).max() <= 1e-13 * max(1.0, np.abs(f).max())
    assert np.abs(gdf - dfp).max() <= 1e-13 * max(1.0, np.abs(df).max())
