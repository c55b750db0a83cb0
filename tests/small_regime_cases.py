"""The case tables of tests/test_gpu_small_regime.py and of its input guard tests/test_small_regime_cpu.py (DESIGN.md section
27): the (d, n, nu) at which one evaluation in one launch (small_eval_kernel) and the device-driven fit (small_fit_kernel) are
run, and the data, theta, boxes, start points and query points of each case.  Both modules take them from here, so the guard
judges the inputs the device is judged on.

small_eval_body stages features eight at a time: pass A walks the chunks upwards and leaves the last one staged, pass B walks
them backwards from it.  The feature counts sit on both sides of every chunk edge (8|9, 16|17, 24|25), at both ends of the
range (1, 32 = SMALL_EVAL_MAXD), at two ragged counts inside a chunk (13, 31), and one past the range as the control (33: the
general launches at n <= 128).  The row counts are the edges of the three lower 64x64 tiles of the 128-block."""
import math

import numpy as np

import feature_count_cases as FC

D_SMALL = (1, 8, 9, 13, 16, 17, 24, 25, 31, 32)
D_CONTROL = 33  # SMALL_EVAL_MAXD + 1
N_CONTROL = 90
N_SMALL = (1, 17, 63, 64, 65, 100, 127, 128)
RAGGED_D = (9, 13, 17, 25, 31)
FULL_D = (8, 16, 24, 32)
NUS = FC.NUS
DTYPES = FC.DTYPES
AMP = FC.AMP
GROUP = 8  # features per staging of small_eval_body
M_QUERY = 5


def is_f32(dtype):
    return np.dtype(dtype) == np.float32


def tol_of(dtype):
    return FC.tol_of(dtype)


def nu_of(d, j, dtype):
    """The orders rotate over the d list as feature_count_cases.nu_of does, two steps on for a d's second row count and one step
    on in f32: every (nu, element type) meets a ragged d and a full chunk (tests/test_small_regime_cpu.py checks it), and every
    d of the grid meets all four orders."""
    return NUS[(D_SMALL.index(d) + 2 * j + (1 if is_f32(dtype) else 0)) % 4]


def n_of(d, j):
    """Two row counts per d, rotating over N_SMALL: every d gets one n <= 64 (the first tile alone) and one n > 64."""
    return N_SMALL[(3 * D_SMALL.index(d) + 4 * j) % len(N_SMALL)]


def eval_cases(dtype):
    """(d, n, nu) of the single-launch evaluations of an element type."""
    return [(d, n_of(d, j), nu_of(d, j, dtype)) for d in D_SMALL for j in (0, 1)]


CONTROL_CASE = (D_CONTROL, N_CONTROL, 1.5)

# the data seed is n + d, except where that draw fails the input guard (tests/test_small_regime_cpu.py) or, for one fit case at
# the most, where the device's and the host's optimiser part at a rounding tie; each entry with its reason
DATA_SEED = {}


def inputs(d, n, dtype):
    """(X, y, theta): feature_count_cases.inputs' recipe with this table's seeds (that table's override at (33, 90) answers its
    leave-one-out gradient; the lml gradient passes the guard here at n + d = 123, and at 125 its last group reaches 9.0e-3)."""
    return FC.inputs(d, n, dtype, seed=DATA_SEED.get((d, n), n + d))


def grad_groups(d):
    """The lml gradient by what small_eval_body publishes together: the noise / amplitude lead, then each chunk of eight length
    scales (red[wave * 35 + 2 + kc + u])."""
    return [("noise, amplitude", slice(0, 2))] + [(f"ell[{s.start}:{s.stop}]", slice(2 + s.start, 2 + s.stop))
                                                 for s in FC.groups(d, GROUP)]


def query_points(X, dtype):
    """Five points inside and slightly outside the unit box; row 1 is a training row."""
    n, d = X.shape
    pts = np.random.default_rng(23 + n + d).uniform(-0.1, 1.1, (M_QUERY, d)).astype(dtype)
    pts[1] = X[n // 2]
    return pts


# ------------------------------------------------------------------------------------------------------------------- the fits
FIT_D = (1, 9, 17, 25, 32)
FIT_N = (65, 100, 128)
MAXEVAL = {np.dtype(np.float64): 30, np.dtype(np.float32): 20}
N_RESTARTS = {np.dtype(np.float64): 2, np.dtype(np.float32): 1}


def _fit_cases():
    """(d, n, nu, dtype, fixed_work): FIT_D x the four orders in f64 with n rotating over FIT_N, the half of them with
    (index of d + index of nu) even in f32 (every d and every order), one fixed-work fit at d = 17, and the control."""
    cases = []
    for i, d in enumerate(FIT_D):
        for k, nu in enumerate(NUS):
            n = FIT_N[(4 * i + k) % 3]
            cases.append((d, n, nu, np.float64, False))
            if (i + k) % 2 == 0:
                cases.append((d, n, nu, np.float32, False))
    cases.append((17, 100, 1.5, np.float64, True))
    return cases


FIT_CASES = _fit_cases()
FIT_CONTROL = CONTROL_CASE + (np.float64, False)  # d = 33: the host drives the optimiser over the general launches


# fits long enough for runs to stop by the pgtol / ftol tests at every width of the state machine (p = 11, 19, 27, 34); with the
# oracle as the objective on the CPU their runs take 39-45, 79-144, 109-140, 35-65, 58-79 and 39-45 evaluations
LONG_MAXEVAL = 150
LONG_FIT_CASES = [(9, 100, 0.5, np.float64, False), (17, 65, 1.5, np.float64, False), (25, 65, math.inf, np.float64, False),
                  (32, 65, 0.5, np.float64, False), (32, 65, 2.5, np.float32, False), (17, 65, 1.5, np.float32, False)]


def fit_box(theta, dtype):
    """(lo, hi) around exp(theta): amplitude in [0.1, 10] c, length scales in [1/8, 8] x their value, noise in [1e-4, 1e2] s2;
    in f32 the noise's lower bound is 1e-2 x the amplitude's UPPER bound, so cond(K) <= 1 + n c / s2 <= 1 + 128 * 100 = 12801
    everywhere in the box: the f32 oracle always has digits."""
    v = np.exp(theta)
    lo = np.concatenate([[1e-4 * v[0], 0.1 * v[1]], v[2:] / 8])
    hi = np.concatenate([[1e2 * v[0], 10 * v[1]], v[2:] * 8])
    if is_f32(dtype):
        lo[0] = 1e-2 * hi[1]
    return lo, hi


COND32_BOUND = 12801.0


def fit_starts(d, n, lo, hi, dtype):
    """The restart points: uniform in the log box."""
    k = N_RESTARTS[np.dtype(dtype)]
    u = np.random.default_rng(7000 + 100 * d + n).uniform(0, 1, (k, d + 2))
    return np.log(lo) + (np.log(hi) - np.log(lo)) * u


def fit_id(case):
    d, n, nu, dtype, fixed = case
    return f"d{d}-n{n}-nu{nu}-{np.dtype(dtype).name}" + ("-fixed" if fixed else "")
