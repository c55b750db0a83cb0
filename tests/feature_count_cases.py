"""The case table of tests/test_gpu_feature_counts.py and of its input guard tests/test_feature_counts_cpu.py (DESIGN.md
section 17): which (d, n) every family runs at, and the data, theta, box, query points and draws of each case.  Both modules take
them from here, so the guard judges the inputs the device is judged on.

The feature counts sit on both sides of every d-dependent branch of the feature kernels (8|9: GT_CHUNK and PE_KB, 16|17 and
32|33: PG_KB, 32|33 also SMALL_EVAL_MAXD) plus the two ends of the ABI's range; the row counts on the tile edges of the
leave-one-out tail (256: no padding, 257: one live row in a 128-block, 320: a multiple of 64 but not of 128)."""
import math

import numpy as np

D_CLASSES = (1, 8, 9, 16, 17, 33, 64)
N_GENERAL = (257, 320)
NUS = [0.5, 1.5, 2.5, math.inf]
DTYPES = (np.float64, np.float32)
AMP = 1.3
GROUP_LOO = 8     # GT_CHUNK: length-scale parameters per register pass of gradtrace_tile
GROUP_DMEAN = 16  # PG_KB: features per pass of pred_grad_kernel


def nu_of(d):
    """The orders rotate over the d list: every NU2 instantiation meets a d > 8 (9 -> 5/2, 16 -> inf, 17 -> 1/2, 33 -> 3/2)."""
    return NUS[D_CLASSES.index(d) % 4]


# leave-one-out: the full grid, n = 256 (np == n) at two d > 8, and the general path at one block (d > SMALL_EVAL_MAXD, n = 90)
LOO_CASES = [(d, n) for d in D_CLASSES for n in N_GENERAL] + [(9, 256), (64, 256), (33, 90), (64, 90)]
# the posterior queries, q-EI and the paths: n = 320 at every d, n = 257 at three
QUERY_CASES = [(d, 320) for d in D_CLASSES] + [(d, 257) for d in (9, 17, 64)]
# (d, n, nu); at d = 64 also the nu = 1/2 draw, whose Student-t frequencies give the widest phases
PATH_CASES = [(d, n, nu_of(d)) for d, n in QUERY_CASES] + [(64, 320, 0.5)]

M_QUERY = (5, 70)  # 5: the handful path; 70 = 17 * 4 + 2: ragged over pred_grad_kernel's four rows and over the 64-tile
QEI_SHAPES = [(1, 3, 256), (5, 3, 256)]  # (q, B, S)
QEI_SEED_CAP = 40
PATHS_S, PATHS_F = 5, 512


def tol_of(dtype):
    import parity_rules as PR

    return PR.TOL64 if np.dtype(dtype) == np.float64 else PR.TOL32


# the data seed is n + d, except where that draw fails the input guard (tests/test_feature_counts_cpu.py): at (33, 90) in
# the f32 noise regime its best group of eight length-scale entries of the leave-one-out gradient reaches only 9.2e-4 of the
# gradient's scale, under the guard's 1e-2; seed 125 gives 1.5e-2
DATA_SEED = {(33, 90): 125}


def inputs(d, n, dtype, seed=None):
    """(X, y, theta) of a case -- tests/test_gpu_model_kinds.py::_extend's recipe: the same correlation range in every d; the
    noise is 1e-2 x the amplitude in f64 and the amplitude in f32 (cond(K) <= n + 1, the regime of every f32 posterior test).
    `seed`: another table's data seed (tests/small_regime_cases.py) in place of this one's."""
    rng = np.random.default_rng(DATA_SEED.get((d, n), n + d) if seed is None else seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    ratio = 1e-2 if np.dtype(dtype) == np.float64 else 1.0
    ell = np.linspace(0.3, 0.9, d) * math.sqrt(max(d, 4) / 4)
    return X.astype(dtype), y.astype(dtype), np.log(np.concatenate([[ratio * AMP, AMP], ell]))


def box_and_thetas(theta):
    """(lo, hi, [theta, clamped]): a box around theta, and theta with its last length scale at twice its value, beyond the
    bound of 1.25 x: evaluated at the bound (tests/test_gpu_loo.py::_thetas)."""
    v = np.exp(theta)
    lo = np.concatenate([[1e-4 * v[0], 0.1], v[2:] / 8])
    hi = np.concatenate([[1e2 * v[0], 10.0], v[2:] * 1.25])
    clamped = theta.copy()
    clamped[-1] = theta[-1] + math.log(2.0)
    return lo, hi, [theta, clamped]


def query_points(X, dtype):
    """70 points inside and slightly outside the unit box; rows 1 and 3 (so: of both the first 5 and all 70) are training rows,
    where the r = 0 convention of the gradient applies."""
    n, d = X.shape
    pool = np.random.default_rng(11 + n + d).uniform(-0.1, 1.1, (max(M_QUERY), d)).astype(dtype)
    pool[1], pool[3] = X[7], X[n - 1]
    return pool


def groups(p, size):
    """The slices of p entries in groups of `size` (the last one ragged)."""
    return [slice(a, min(a + size, p)) for a in range(0, p, size)]


def qei_batches(d, n, q, B, seed, dtype):
    return np.random.default_rng(100000 * q + 1000 * d + n + seed).uniform(-0.1, 1.1, (B, q, d)).astype(dtype)


def qei_normals(q, S, dtype):
    return np.random.default_rng(7 + q).standard_normal((S, q)).astype(dtype)


def qei_fmin(mins):
    """fmin from the restated minima [B, S] of every draw of a call: the middle of the widest gap between neighbouring minima
    (of all batches) inside [max_b of batch b's S/8-th smallest, max_b of its S/4-th smallest].  So every batch improves on at
    least an eighth of the draws (no batch with qEI = 0 and a zero gradient), and no draw lies at the fmin kink."""
    mins = np.sort(np.asarray(mins, np.float64), axis=1)
    S = mins.shape[1]
    lo, hi = mins[:, S // 8].max(), mins[:, S // 4].max()
    s = np.sort(mins.ravel())
    s = s[(s >= lo) & (s <= hi)]
    k = int(np.argmax(np.diff(s)))
    return float(0.5 * (s[k] + s[k + 1]))


# f32: the first batch seed of each (d, n, q) whose restated draws keep top_two_gap > 1e-3 sqrt(c), found on the CPU at
# exp(theta); the test starts its search there and keeps the cap of QEI_SEED_CAP seeds
QEI_SEED32 = {(33, 320, 5): 1}  # every other (d, n, q): 0
