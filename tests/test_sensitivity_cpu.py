"""CPU: the restated sensitivity estimators (tests/sensitivity_ref.py) on a function whose indices are known in closed form, and
the input guard of the dead-dimension cases of tests/test_gpu_sensitivity.py.

A linear f(x) = a . x on the unit cube has first = total = a_k^2 / sum a^2 (no interactions) and main effects a_k x + const.
The guard computes the cases' posterior mean on the host (alpha by a dense solve at the cases' own theta) and checks that the
inputs can show what the GPU test asserts: a variance well above the value bar, live features well above the dead one."""
import numpy as np
import pytest

import sensitivity_ref as SR
from hbetune_rs_amd import estimator as E

A_LIN = np.array([1.0, 2.0, 3.0, 0.5])


def _linear(points):
    return np.asarray(points, np.float64) @ A_LIN


def test_estimators_recover_the_indices_of_a_linear_function():
    N = 16384
    rng = np.random.default_rng(20240)
    A, B = rng.uniform(0, 1, (N, 4)), rng.uniform(0, 1, (N, 4))
    first, total, f0, V = SR.sobol_estimators(*SR.sobol_values(_linear, A, B))
    want = A_LIN ** 2 / (A_LIN ** 2).sum()
    print(f"first - want {np.abs(first - want).max():.4f}  total - want {np.abs(total - want).max():.4f}  f0 {f0:.4f}  V {V:.4f}")
    assert np.abs(first - want).max() <= 0.03
    assert np.abs(total - want).max() <= 0.03
    assert abs(f0 - A_LIN.sum() / 2) <= 0.02 and abs(V - (A_LIN ** 2).sum() / 12) <= 0.02


def test_a_constant_function_has_zero_indices():
    rng = np.random.default_rng(3)
    A, B = rng.uniform(0, 1, (50, 3)), rng.uniform(0, 1, (50, 3))
    first, total, f0, V = SR.sobol_estimators(*SR.sobol_values(lambda p: np.full(len(p), 2.5), A, B))
    assert V == 0.0 and f0 == 2.5 and (first == 0).all() and (total == 0).all()


def test_main_effects_of_a_linear_function_are_its_slopes():
    N, G = 200, 8
    A = np.random.default_rng(5).uniform(0, 1, (N, 4))
    grid = np.broadcast_to((np.arange(G) + 0.5) / G, (4, G)).copy()
    effect = SR.main_effects(_linear, A, grid)
    for k in range(4):
        const = (A.mean(axis=0) * A_LIN).sum() - A[:, k].mean() * A_LIN[k]
        assert np.abs(effect[k] - (A_LIN[k] * grid[k] + const)).max() <= 1e-12
    curves = SR.row_curves(_linear, A[:1], grid)  # one row: its conditional curves
    assert np.abs(curves[0] - SR.main_effects(_linear, A[:1], grid)).max() == 0.0


def test_pick_freeze_takes_one_column_from_b():
    A, B = np.zeros((3, 4)), np.ones((3, 4))
    AB = SR.pick_freeze(A, B)
    assert AB.shape == (4, 3, 4)
    for k in range(4):
        assert (AB[k].sum(axis=1) == 1).all() and (AB[k][:, k] == 1).all()


def test_rank_parameters_orders_by_total_index_ties_to_the_lower_index():
    class Tied:
        def sobol_indices_a(self, n_samples, rng, bounds=None):
            return np.zeros(4), np.array([0.2, 0.5, 0.2, 0.5])
    order, first, total = E.rank_parameters(Tied(), 8, None)
    assert list(order) == [1, 3, 0, 2] and order.dtype == np.int64 and total[1] == 0.5


@pytest.mark.parametrize("nu", SR.NUS)
@pytest.mark.parametrize("d,n", SR.DEAD_CASES)
def test_dead_dimension_inputs_can_show_what_the_gpu_test_asserts(d, n, nu):
    X, y, theta, A, B = SR.dead_inputs(d, n)
    v = np.exp(theta)
    f = SR.posterior_mean(X, SR.solve_alpha(X, y, theta, nu), v[1], v[2:], nu)
    first, total, f0, V = SR.sobol_estimators(*SR.sobol_values(f, A, B))
    print(f"d={d} n={n} nu={nu}: V {V:.3f}  live totals >= {total[:-1].min():.3e}  dead total {total[-1]:.2e}  dead first {first[-1]:.2e}")
    assert V >= 1e-2
    assert total[:-1].min() >= 1e-2
    assert total[-1] <= 1e-9
