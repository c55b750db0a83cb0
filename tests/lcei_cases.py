"""The dead-zone search shared by tests/test_lcei_cpu.py (where its inputs are shown to work with the reference alone) and
tests/test_gpu_lcei.py (where the device maximiser runs on them): no feasible point is known (fmin = +inf), one constraint
g(x) ~ x_0 <= LIMIT modelled with little noise, and six starts well on the wrong side of it, where sigma is 3e-3 to 1e-2: every z lies
far beyond -38, so the plain-space probability of feasibility is exactly 0 with a zero gradient."""
import math

import numpy as np

D = 2
N = 120
NU = 2.5
LIMIT = 0.2
MAXEVAL = 60
BOUNDS = [(0.0, 1.0)] * D


def training_rows():
    return np.random.default_rng(2023).uniform(0, 1, (N, D))


def objective_targets(X):
    return np.sin(3 * X).sum(axis=1) / math.sqrt(D) * 2


def constraint_targets(X):
    return X[:, 0] + 0.05 * np.sin(2 * X[:, 1:]).sum(axis=1)


def thetas():
    """log(noise, amplitude, length scales) of the objective's and the constraint's model: a well-fitted, low-noise surrogate."""
    ell = np.full(D, 0.7)
    return np.log(np.concatenate([[1e-6, 1.3], ell])), np.log(np.concatenate([[1e-6, 0.5], ell]))


def starts():
    """Six starts with x_0 between 0.66 and 0.9."""
    s = np.random.default_rng(7).uniform(0.3, 0.7, (6, D))
    s[:, 0] = np.linspace(0.66, 0.9, 6)
    return s
