"""The case table of tests/test_gpu_warp.py and of its input guard in tests/test_warp_cpu.py: both modules
take the data, theta, warp and row variances of every case from here, so the guard judges the inputs the device is judged on.

Rows: 5, 64, 128 sit in the single launch of at most 128 rows (at d = 33 > SMALL_EVAL_MAXD they take the general path), 129 is the
first row count of the general path, 257 has one live row in a padded 128-block, 320 ends on a 64-tile edge inside a 128-block.
Features: both sides of GT_CHUNK = 8 (8 | 9) and two and four chunks past it (17, 33); the orders are spread so that each of the
four meets a d > 8."""
import math

import numpy as np

import feature_count_cases as FC

INF = math.inf
# (n, d, nu)
SHAPES = [
    (5, 1, 0.5), (5, 8, 1.5),
    (64, 9, 2.5), (64, 33, INF),
    (128, 8, INF), (128, 17, 0.5), (128, 33, 1.5),
    (129, 1, 2.5), (129, 9, INF),
    (257, 8, 0.5), (257, 17, 1.5), (257, 33, 2.5),
    (320, 9, 0.5), (320, 17, 2.5),
]
F32_SHAPES = [(5, 8, 1.5), (64, 33, INF), (128, 17, 0.5), (129, 9, INF), (257, 33, 2.5), (320, 17, 2.5)]


class Case:
    def __init__(self, n, d, nu, dtype, kind="plain"):
        self.n, self.d, self.nu, self.dtype, self.kind = n, d, nu, np.dtype(dtype), kind
        self.id = f"n{n}-d{d}-nu{nu}-{self.dtype.name}" + ("" if kind == "plain" else f"-{kind}")

    @property
    def tol(self):
        return FC.tol_of(self.dtype)


CASES = ([Case(n, d, nu, np.float64) for n, d, nu in SHAPES] + [Case(n, d, nu, np.float32) for n, d, nu in F32_SHAPES] +
         [Case(257, 8, 2.5, np.float64, "rv"),      # known row variances on the diagonal
          Case(129, 9, 1.5, np.float64, "dup"),     # rows 3 and 100 are one point: r = 0 off the diagonal
          Case(320, 9, 2.5, np.float64, "queue")])  # HBEGP_DAG=1: the evaluation runs through the task queue

# the data seed is n + d (feature_count_cases.inputs) except where that draw fails the input guard of tests/test_warp_cpu.py
DATA_SEED = {}


def inputs(case):
    """(X, y, theta): the recipe of DESIGN section 17 -- X uniform in [0, 1], ell = linspace(0.3, 0.9, d) sqrt(max(d, 4) / 4), the
    noise 1e-2 c in f64 and c in f32."""
    X, y, theta = FC.inputs(case.d, case.n, case.dtype, seed=DATA_SEED.get(case.id, case.n + case.d))
    if case.kind == "dup":
        X[100] = X[3]
    return X, y, theta


def row_variance(case):
    if case.kind != "rv":
        return None
    return np.random.default_rng(5 + case.n).uniform(0.0, 0.05, case.n)


def warp_ab(case):
    """a, b drawn in [0.4, 2.5], log-uniformly."""
    return np.exp(np.random.default_rng(1000 + case.n + case.d).uniform(math.log(0.4), math.log(2.5), 2 * case.d))


# ---- the fit fixture: a response that is stationary only after a warp ---------------------------------------------------------
FIT_AB = np.array([0.3, 1.0, 1.0, 3.0])  # a = (0.3, 1), b = (1, 3)
FIT_SIZES = (96, 200)
FIT_SEED = {96: 96, 200: 200}


def fit_data(n, dtype=np.float64):
    """d = 2, X uniform in [0, 1]^2, y = sin(6 u_1) + cos(4 u_2) + N(0, 0.05^2) at u = w(X; FIT_AB), standardised."""
    rng = np.random.default_rng(FIT_SEED[n])
    X = rng.uniform(0, 1, (n, 2))
    U = 1.0 - (1.0 - X ** FIT_AB[:2]) ** FIT_AB[2:]
    y = np.sin(6 * U[:, 0]) + np.cos(4 * U[:, 1]) + 0.05 * rng.standard_normal(n)
    y = (y - y.mean()) / y.std()
    return X.astype(dtype), y.astype(dtype)


FIT_NU = 2.5
FIT_THETA0 = np.log(np.array([0.05, 1.0, 0.5, 0.5]))
FIT_LO = np.array([1e-4, 0.05, 0.05, 0.05])
FIT_HI = np.array([1.0, 20.0, 5.0, 5.0])
# The f32 fit: the noise floor of every f32 fit of the suite (tests/test_gpu_incremental.py: 1e-2 x the largest amplitude of the
# box), with the amplitude capped at 2.  In the f64 box above the optimum sits at c = 20, s2 = 4e-3 with cond(K) = 4.5e5, where an
# f32 kernel matrix alone (eps 6e-8 per entry) moves the lml by ~2e-2: no f32 evaluation has the digits for 1e-4 |lml| there
# (measured on the device: 2.4e-4).  In this box cond(K) = 7.0e3 at the optimum and LAPACK's own f32 lml is 1.5e-6 off.
FIT_HI32 = np.array([1.0, 2.0, 5.0, 5.0])
FIT_LO32 = np.array([1e-2 * FIT_HI32[1], 0.05, 0.05, 0.05])


def fit_box(dtype):
    return (FIT_LO32, FIT_HI32) if np.dtype(dtype) == np.float32 else (FIT_LO, FIT_HI)
