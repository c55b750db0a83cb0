"""The case table of tests/test_gpu_paths_sizes.py and of its guard tests/test_paths_sizes_cpu.py ("The
size-dependent splits under test"): the smallest (n, d, F, S, m) that reach each of the four splits of the sample-path entry
points.  Both modules take them from here, so the guard judges the shapes the device is run at.

  1. blocks of points (csrc/hbegp.cpp: paths_eval_locked):  mb = min(m, 262144 / S, 256 MiB / per_point), at least 1, with
     per_point = 8 (ceil(n / 512) + ceil(F / 512)) S (d + 1); a call with m > mb loops over blocks, and only there do the 2-D
     copies have a pitch that differs from their width.
  2. feature chunks of the projection (csrc/kernels.hip: paths_project_chunks):  cap = min(64, 128 MiB / (8 S n)), at least 1,
     nch = min(cap, ceil(F / 64)), fch = ceil(F / nch) rounded up to 32, nch = ceil(F / fch).  fch > 64 (three or more 32-feature
     tiles per chunk) needs F > 4096 or S n > 262144.
  3. more than 64 paths (blockIdx.z > 0 of paths_project_kernel) and an [S_p][n_p] GEMM operand of several 128-row blocks.
  4. a lockstep round of the minimiser whose [S][mr] evaluation spans blocks.

Neither rule is restated here: the expected numbers below were worked out by hand from the rules above, and the guard asks the
library (hbegp_debug_paths_eval_blocks, hbegp_debug_paths_project_chunks: the functions the engine itself calls) for each of them.
cap = 1 needs n >= 16384 at S = 1024: a model of that size is beyond a quick test, so cap = 1 is covered by the guard's sweep only.

Models are FittedKernel.extend on tests/test_gpu_paths.py's data recipe and noise regime (f64: 1e-2 of the amplitude; f32: the
amplitude); nu rotates over the four orders."""
import collections
import ctypes as C
import math

import numpy as np

from hbetune_rs_amd import _lib

NUS = (0.5, 1.5, 2.5, math.inf)
DTYPES = (np.float64, np.float32)
PP_FT = 32            # features per LDS tile of the projection
ROUND_STARTS = 60     # starts per path of the round-blocks case, on part-cap's handle

# blocks: the point blocks of an evaluation of m points; cap, nch, fch: the projection's split; last: features of its last chunk
Case = collections.namedtuple("Case", "name n d F S m blocks cap nch fch last nu")

_TABLE = [
    # name            n    d   F      S     m    blocks          cap nch fch  last
    ("rows-shared",   100, 2,  64,    1024, 600, (256, 256, 88), 64, 1,  64,  64),
    ("rows-per-path", 100, 3,  96,    600,  900, (436, 436, 28), 64, 2,  64,  32),
    ("part-cap",      100, 17, 16384, 1000, 130, (56, 56, 18),   64, 64, 256, 256),
    ("fch96-capped",  300, 4,  4100,  1000, 20,  (20,),          55, 43, 96,  68),
    ("fch96",         200, 4,  4097,  4,    20,  (20,),          64, 43, 96,  65),
    ("cap4",          4096, 4, 1024,  1024, 20,  (20,),          4,  4,  256, 256),
    ("tiny-F1-S1",    200, 4,  1,     1,    9,   (9,),           64, 1,  32,  1),
    ("tiny-F1-S3",    200, 4,  1,     3,    9,   (9,),           64, 1,  32,  1),
    ("tiny-F33-S1",   200, 4,  33,    1,    9,   (9,),           64, 1,  64,  33),
    ("tiny-F33-S3",   200, 4,  33,    3,    9,   (9,),           64, 1,  64,  33),
]
CASES = [Case(*row, nu=NUS[i % len(NUS)]) for i, row in enumerate(_TABLE)]
BY_NAME = {c.name: c for c in CASES}
ROUND_CASE = BY_NAME["part-cap"]
ROUND_BLOCKS = (56, 4)  # the first round's [S][60] evaluation
HYGIENE_CASE = BY_NAME["rows-per-path"]


def eval_block(n, d, F, S, m):
    """mb of an evaluation of m points, from the library."""
    mb = C.c_int(-1)
    _lib.check(_lib.load().hbegp_debug_paths_eval_blocks(n, d, F, S, m, C.byref(mb)))
    return mb.value


def eval_blocks(n, d, F, S, m):
    """The block lengths of an evaluation of m points, in order."""
    mb = eval_block(n, d, F, S, m)
    assert mb >= 1
    return tuple(min(mb, m - p0) for p0 in range(0, m, mb))


def project_chunks(F, n, S):
    """(cap, nch, fch) of the projection, from the library."""
    cap, nch, fch = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _lib.check(_lib.load().hbegp_debug_paths_project_chunks(F, n, S, C.byref(cap), C.byref(nch), C.byref(fch)))
    return cap.value, nch.value, fch.value


def blocks_of(case, m=None):
    return eval_blocks(case.n, case.d, case.F, case.S, case.m if m is None else m)


def slices(m, mb):
    """[a, b) pieces of [0, m), each shorter than a block and none but the first starting at a block edge: pieces of mb - 3
    points (mb > 3 in every multi-block case)."""
    step = mb - 3
    assert step >= 1
    cuts = [(a, min(m, a + step)) for a in range(0, m, step)]
    assert all(a % mb != 0 for a, _ in cuts[1:])
    return cuts


def case_id(case, dtype):
    return f"{case.name}-{np.dtype(dtype).name}"
