"""GPU: Sobol indices and main-effect curves of the posterior mean (hbegp_sobol_* / hbegp_main_effects_*).

The device's substituted-coordinate means against the NumPy restatement (tests/sensitivity_ref.py) on the engine's own alpha and
device_params() at every d class and on both sides of the kernel's own d branches (8 | 9 features per pass per row, 2 | 3 per
grid), and at n = 1100 with G = 19 over several chunks of training points and several passes of grid values, ragged last
ones included; the indices against the restated estimators on the device's own values; a substituted point that is a training row
(r = 0); predict on the materialised points; a dead dimension; bits (prefix, one row, slabs, threads, after a NaN); every kind of
model; arguments and the estimator's wrappers.

Bars: the project's plain bar on a mean, 1e-8 (f64) / 1e-4 (f32) times max(1, max |f|); 1e-8 absolute on the indices (fp64 sums
over identical inputs).  Measured deviations: DESIGN section 19."""
import ctypes as C
import functools
import math
import threading

import numpy as np
import pytest

import feature_count_cases as FC
import sensitivity_ref as SR
import test_gpu_model_kinds as MK
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

N_ROWS = 70  # ragged over the four rows of a workgroup
G_SMALL = 5
# every d class at n = 320, three at n = 257, and d = 2, 3: the other side of the two features per pass of the grid mode (d = 1 is
# a class; 8 | 9 and 16 | 17, the eight features per pass of the per-row mode, are classes too)
CASES = FC.QUERY_CASES + [(2, 320), (3, 320)]


def _nu(d):
    return FC.nu_of(d) if d in FC.D_CLASSES else FC.NUS[d % 4]


def _reference(fk, nu):
    alpha, _ = fk.arrays(want_kinv=False)
    _, amp, ell = fk.device_params()
    return SR.posterior_mean(fk.x_train, alpha, amp, ell, nu)


def _grid(d, G, dtype, seed=0):
    return np.random.default_rng(50 + d + seed).uniform(-0.1, 1.1, (d, G)).astype(dtype)


@functools.lru_cache(maxsize=None)
def _case(d, n, dtype):
    """One model per case: the device's outputs and the restatement's, shared by the tests below and left unchanged."""
    nu = _nu(d)
    X, y, theta = FC.inputs(d, n, dtype)
    fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    A, B = SR.samples(d, N_ROWS, 11 + n + d, dtype)
    grid = _grid(d, G_SMALL, dtype)
    f = _reference(fk, nu)
    out = dict(dev=fk.sobol_indices(A, B, want_values=True), eff=fk.main_effects(A, grid, want_base=True),
               ref=SR.sobol_values(f, A, B), ref_eff=SR.main_effects(f, A, grid))
    fk.release()
    return out


def _check_values(fk, nu, dtype, A, B, grid, what):
    """f_a, f_b, f_ab and the effects of one model against the restatement at the plain bar; returns the worst deviation."""
    f = _reference(fk, nu)
    first, total, f0, V, f_a, f_b, f_ab = fk.sobol_indices(A, B, want_values=True)
    ra, rb, rab = SR.sobol_values(f, A, B)
    eff, base = fk.main_effects(A, grid, want_base=True)
    reff = SR.main_effects(f, A, grid)
    bar = SR.bar(dtype, np.concatenate([ra, rb, rab.ravel()]))
    dev = max(np.abs(f_a - ra).max(), np.abs(f_b - rb).max(), np.abs(f_ab - rab).max(), np.abs(eff - reff).max())
    print(f"{what}: values {dev:.1e} (bar {bar:.1e})")
    assert dev <= bar, (what, dev, bar)
    assert base.tobytes() == f_a.tobytes()
    rf, rt, rf0, rV = SR.sobol_estimators(f_a, f_b, f_ab)
    assert max(np.abs(first - rf).max(), np.abs(total - rt).max(), abs(f0 - rf0), abs(V - rV)) <= 1e-8
    return dev


# ---------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("d,n", CASES)
def test_values_match_the_restatement(d, n, dtype):
    c = _case(d, n, dtype)
    first, total, f0, V, f_a, f_b, f_ab = c["dev"]
    eff, base = c["eff"]
    ra, rb, rab = c["ref"]
    assert f_a.dtype == dtype and f_b.dtype == dtype and f_ab.dtype == dtype and f_ab.shape == (d, N_ROWS)
    assert eff.dtype == np.float64 and eff.shape == (d, G_SMALL) and first.dtype == np.float64
    bar = SR.bar(dtype, np.concatenate([ra, rb, rab.ravel()]))
    devs = dict(f_a=np.abs(f_a - ra).max(), f_b=np.abs(f_b - rb).max(), f_ab=np.abs(f_ab - rab).max(),
                effect=np.abs(eff - c["ref_eff"]).max())
    print(f"d={d} n={n} {np.dtype(dtype).name} nu={_nu(d)}: " + " ".join(f"{k} {v:.1e}" for k, v in devs.items()) + f" (bar {bar:.1e})")
    assert max(devs.values()) <= bar, devs
    assert base.tobytes() == f_a.tobytes()


@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("d,n", CASES)
def test_indices_are_the_estimators_of_the_device_values(d, n, dtype):
    first, total, f0, V, f_a, f_b, f_ab = _case(d, n, dtype)["dev"]
    rf, rt, rf0, rV = SR.sobol_estimators(f_a, f_b, f_ab)
    devs = (np.abs(first - rf).max(), np.abs(total - rt).max(), abs(f0 - rf0), abs(V - rV))
    print(f"d={d} n={n} {np.dtype(dtype).name}: first {devs[0]:.1e} total {devs[1]:.1e} f0 {devs[2]:.1e} V {devs[3]:.1e}")
    assert max(devs) <= 1e-8


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("nu", FC.NUS)
def test_a_substituted_point_that_is_a_training_row(nu, dtype):
    d, n = 4, 100
    X, y, theta = FC.inputs(d, n, dtype)
    fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    A, B = SR.samples(d, N_ROWS, 3, dtype)
    grid = _grid(d, G_SMALL, dtype)
    for k in range(d):  # row 1 + k of A is training row 7 except in feature k, where B and one grid value restore it
        A[1 + k] = X[7]
        A[1 + k, k] = dtype(0.5) * (X[7, k] + dtype(0.37))
        B[1 + k, k] = X[7, k]
        grid[k, 2] = X[7, k]
    f = _reference(fk, nu)
    _, _, _, _, f_a, f_b, f_ab = fk.sobol_indices(A, B, want_values=True)
    ra, rb, rab = SR.sobol_values(f, A, B)
    bar = SR.bar(dtype, np.concatenate([ra, rb, rab.ravel()]))
    dev = np.abs(f_ab - rab)
    hit = np.array([dev[k, 1 + k] for k in range(d)])
    ordinary = dev.copy()
    for k in range(d):
        ordinary[k, 1 + k] = 0.0
    print(f"nu={nu} {np.dtype(dtype).name}: at the training row {hit.max():.1e}, ordinary rows {ordinary.max():.1e} (bar {bar:.1e})")
    assert dev.max() <= bar
    # the conditional curve of each such row: the grid value that restores the training row
    cur_hit, cur_all = 0.0, 0.0
    for k in range(d):
        eff = fk.main_effects(A[1 + k:2 + k], grid)
        dv = np.abs(eff - SR.main_effects(f, A[1 + k:2 + k], grid))
        assert dv.max() <= bar
        cur_hit = max(cur_hit, dv[k, 2])
        dv[k, 2] = 0.0
        cur_all = max(cur_all, dv.max())
    print(f"    curves: at the training row {cur_hit:.1e}, elsewhere {cur_all:.1e}")
    if nu == 0.5:  # the kink at r = 0: a cancellation residue in r^2 would show here (3e-9 of the amplitude per training row)
        assert hit.max() <= ordinary.max()
        assert cur_hit <= cur_all
    fk.release()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("dtype", FC.DTYPES)
def test_values_match_predict_on_the_materialised_points(dtype):
    d, n = 4, 300
    X, y, theta = FC.inputs(d, n, dtype)
    fk = gpr.FittedKernel.extend(X, y, theta, nu=2.5)
    A, B = SR.samples(d, N_ROWS, 4, dtype)
    grid = _grid(d, G_SMALL, dtype)
    _, _, _, _, f_a, f_b, f_ab = fk.sobol_indices(A, B, want_values=True)
    AB = SR.pick_freeze(A, B).reshape(d * N_ROWS, d)
    big, _, _ = fk.predict(AB, want_variance=False)  # m > 16: the batched path
    bar = SR.bar(dtype, big)
    assert np.abs(f_ab.ravel().astype(np.float64) - big).max() <= bar
    small = np.concatenate([fk.predict(AB[a:a + 16], want_variance=False)[0] for a in range(0, 48, 16)])  # m <= 16: the handful path
    assert np.abs(f_ab.ravel()[:48].astype(np.float64) - small).max() <= bar
    pa, _, _ = fk.predict(A, want_variance=False)
    pb, _, _ = fk.predict(B[:16], want_variance=False)
    assert np.abs(f_a.astype(np.float64) - pa).max() <= bar and np.abs(f_b[:16].astype(np.float64) - pb).max() <= bar
    eff = fk.main_effects(A, grid)
    want = np.empty((d, G_SMALL))
    for k in range(d):
        pts = SR.effect_points(A, grid, k).reshape(G_SMALL * N_ROWS, d)
        pm, _, _ = fk.predict(pts, want_variance=False)
        want[k] = pm.astype(np.float64).reshape(G_SMALL, N_ROWS).mean(axis=1)
    one = fk.main_effects(A[:1], grid)  # one row, d G = 20 points, in handfuls
    pts = np.concatenate([SR.effect_points(A[:1], grid, k).reshape(G_SMALL, d) for k in range(d)])
    pm = np.concatenate([fk.predict(pts[a:a + 10], want_variance=False)[0] for a in (0, 10)])
    print(f"{np.dtype(dtype).name}: f_ab - predict {np.abs(f_ab.ravel() - big).max():.1e}, effect - predict {np.abs(eff - want).max():.1e}")
    assert np.abs(eff - want).max() <= bar
    assert np.abs(one.ravel() - pm.astype(np.float64)).max() <= bar
    fk.release()


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("nu", FC.NUS)
@pytest.mark.parametrize("d,n", SR.DEAD_CASES)
def test_a_dead_dimension_has_no_index(d, n, nu):
    X, y, theta, A, B = SR.dead_inputs(d, n)
    fk = gpr.FittedKernel.extend(X, y, theta, nu=nu)
    first, total, f0, V = fk.sobol_indices(A, B)
    print(f"d={d} n={n} nu={nu}: V {V:.3f} dead total {total[-1]:.2e} dead first {first[-1]:.2e} live totals >= {total[:-1].min():.3e}")
    assert total[-1] <= 1e-9
    assert abs(first[-1]) <= 2.0 * math.sqrt(2.0 * total[-1]) + 1e-8  # Cauchy-Schwarz on the estimator
    assert total[:-1].min() >= 1e-2
    model = E.SurrogateModelGPR(fk, None, None, None, E.YNormalize(1.0, 0.0, "linear"), np.float64)
    order, rf, rt = E.rank_parameters(model, SR.DEAD_N, E.RNG.new_with_seed(5))
    assert order.dtype == np.int64 and sorted(order) == list(range(d))
    assert order[-1] == d - 1 and (np.diff(rt[order]) <= 0).all()
    fk.release()


# ---------------------------------------------------------------------------------------------------------------- 6
def _bits_model(dtype=np.float64, d=9, n=320):
    X, y, theta = FC.inputs(d, n, dtype)
    return gpr.FittedKernel.extend(X, y, theta, nu=_nu(d)), d


def _all_bytes(out):
    return [np.asarray(v).tobytes() for v in out]


def test_a_prefix_of_the_rows_gives_the_same_bits():
    fk, d = _bits_model()
    A, B = SR.samples(d, N_ROWS, 6, np.float64)
    _, _, _, _, f_a, f_b, f_ab = fk.sobol_indices(A, B, want_values=True)
    _, _, _, _, p_a, p_b, p_ab = fk.sobol_indices(A[:5], B[:5], want_values=True)
    assert p_a.tobytes() == f_a[:5].tobytes() and p_b.tobytes() == f_b[:5].tobytes()
    assert p_ab.tobytes() == np.ascontiguousarray(f_ab[:, :5]).tobytes()
    fk.release()


@pytest.mark.parametrize("dtype", FC.DTYPES)
def test_one_rows_curve_has_the_same_bits_alone_and_inside_a_larger_call(dtype, monkeypatch):
    fk, d = _bits_model(dtype)
    A, _ = SR.samples(d, 11, 7, dtype)
    grid = _grid(d, G_SMALL, dtype)
    eff, base = fk.main_effects(A, grid, want_base=True)
    monkeypatch.setenv("HBEGP_SENS_SLAB_ROWS", "1")
    eff1, base1 = fk.main_effects(A, grid, want_base=True)  # one-row slabs
    monkeypatch.delenv("HBEGP_SENS_SLAB_ROWS")
    assert eff1.tobytes() == eff.tobytes() and base1.tobytes() == base.tobytes()
    acc = np.zeros((d, G_SMALL))
    for i in range(len(A)):  # the larger call adds the rows' curves in ascending order and divides once
        cur, b = fk.main_effects(A[i:i + 1], grid, want_base=True)
        assert b.tobytes() == base[i:i + 1].tobytes()
        acc = acc + cur
    assert (acc / len(A)).tobytes() == eff.tobytes()
    fk.release()


@pytest.mark.parametrize("dtype", FC.DTYPES)
def test_the_slab_size_never_shows(dtype, monkeypatch):
    fk, d = _bits_model(dtype)
    A, B = SR.samples(d, 300, 8, dtype)
    grid = _grid(d, G_SMALL, dtype)
    want_s = _all_bytes(fk.sobol_indices(A, B, want_values=True))
    want_m = _all_bytes(fk.main_effects(A, grid, want_base=True))
    for rows in ("1", "7", "64"):  # 600 and 300 rows: whole slabs of one row; 85 x 7 + 5 and 42 x 7 + 6; 9 x 64 + 24 and 4 x 64 + 44
        monkeypatch.setenv("HBEGP_SENS_SLAB_ROWS", rows)
        assert _all_bytes(fk.sobol_indices(A, B, want_values=True)) == want_s, rows
        assert _all_bytes(fk.main_effects(A, grid, want_base=True)) == want_m, rows
    fk.release()


# Several n-chunks and several value passes: n = 1100 is three chunks of sens_kernel's 512 training points, the last one ragged
# (76, itself a 64-tile and a ragged one); G = 19 is three passes of the grid mode's eight values, the last one ragged; d = 2 | 3
# on both sides of its two features per pass, d = 9 on the far side of the per-row mode's eight.
N_CHUNKED, G_PASSES = 1100, 19
CHUNKED_D = (2, 3, 9)


def _chunked_model(d, dtype):
    X, y, theta = FC.inputs(d, N_CHUNKED, dtype)
    return gpr.FittedKernel.extend(X, y, theta, nu=_nu(d))


@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("d", CHUNKED_D)
def test_values_over_several_chunks_and_value_passes(d, dtype):
    fk = _chunked_model(d, dtype)
    A, B = SR.samples(d, N_ROWS, 21 + d, dtype)
    _check_values(fk, _nu(d), dtype, A, B, _grid(d, G_PASSES, dtype), f"n={N_CHUNKED} d={d} G={G_PASSES} {np.dtype(dtype).name}")
    # every chunk carries weight: the restated means without the training points of the later chunks are off by more than ten bars
    alpha, _ = fk.arrays(want_kinv=False)
    _, amp, ell = fk.device_params()
    full = _reference(fk, _nu(d))(A)
    for cut in (512, 1024):
        part = SR.posterior_mean(fk.x_train[:cut], alpha[:cut], amp, ell, _nu(d))(A)
        assert np.abs(part - full).max() > 10 * SR.bar(dtype, full), cut
    fk.release()


@pytest.mark.parametrize("dtype", FC.DTYPES)
@pytest.mark.parametrize("d", CHUNKED_D)
def test_bits_over_several_chunks_and_value_passes(d, dtype, monkeypatch):
    fk = _chunked_model(d, dtype)
    A, B = SR.samples(d, 150, 22 + d, dtype)
    grid = _grid(d, G_PASSES, dtype)
    want_s = fk.sobol_indices(A, B, want_values=True)
    want_m = fk.main_effects(A, grid, want_base=True)
    # a prefix of the rows
    _, _, _, _, p_a, p_b, p_ab = fk.sobol_indices(A[:5], B[:5], want_values=True)
    assert p_a.tobytes() == want_s[4][:5].tobytes() and p_b.tobytes() == want_s[5][:5].tobytes()
    assert p_ab.tobytes() == np.ascontiguousarray(want_s[6][:, :5]).tobytes()
    # one row's curves alone and inside the larger call: the rows in ascending order, one division
    acc = np.zeros((d, G_PASSES))
    for i in range(12):
        cur, b = fk.main_effects(A[i:i + 1], grid, want_base=True)
        assert b.tobytes() == want_m[1][i:i + 1].tobytes()
        acc = acc + cur
    assert (acc / 12).tobytes() == fk.main_effects(A[:12], grid).tobytes()
    # slabs: 300 and 150 rows in whole slabs of one row; 42 x 7 + 6 and 21 x 7 + 3; 4 x 64 + 44 and 2 x 64 + 22
    for rows in ("1", "7", "64"):
        monkeypatch.setenv("HBEGP_SENS_SLAB_ROWS", rows)
        assert _all_bytes(fk.sobol_indices(A, B, want_values=True)) == _all_bytes(want_s), rows
        assert _all_bytes(fk.main_effects(A, grid, want_base=True)) == _all_bytes(want_m), rows
    fk.release()


def test_two_threads_on_one_model_give_the_same_bits():
    fk, d = _bits_model()
    A, B = SR.samples(d, N_ROWS, 9, np.float64)
    grid = _grid(d, G_SMALL, np.float64)
    want = _all_bytes(fk.sobol_indices(A, B, want_values=True)) + _all_bytes(fk.main_effects(A, grid, want_base=True))
    got = [None, None]

    def work(i):
        for _ in range(3):
            got[i] = _all_bytes(fk.sobol_indices(A, B, want_values=True)) + _all_bytes(fk.main_effects(A, grid, want_base=True))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got[0] == want and got[1] == want
    fk.release()


def test_a_nan_row_stays_in_its_row_and_leaves_nothing_behind():
    fk, d = _bits_model()
    A, B = SR.samples(d, N_ROWS, 10, np.float64)
    grid = _grid(d, G_SMALL, np.float64)
    clean_s = fk.sobol_indices(A, B, want_values=True)
    clean_m = fk.main_effects(A, grid, want_base=True)
    An = A.copy()
    An[3, 2] = np.nan
    first, total, f0, V, f_a, f_b, f_ab = fk.sobol_indices(An, B, want_values=True)
    assert np.isnan(f_a[3]) and np.isnan(np.delete(f_ab[:, 3], 2)).all()
    assert f_ab[2, 3].tobytes() == clean_s[6][2, 3].tobytes()  # feature 2 of row 3 is the substituted one: B's value, no NaN
    keep = np.arange(N_ROWS) != 3
    assert f_a[keep].tobytes() == clean_s[4][keep].tobytes() and f_b.tobytes() == clean_s[5].tobytes()
    assert np.ascontiguousarray(f_ab[:, keep]).tobytes() == np.ascontiguousarray(clean_s[6][:, keep]).tobytes()
    assert np.isnan(first).all() and np.isnan(f0)
    eff, base = fk.main_effects(An, grid, want_base=True)
    assert np.isnan(base[3]) and base[keep].tobytes() == clean_m[1][keep].tobytes() and np.isnan(np.delete(eff, 2, axis=0)).all()
    assert _all_bytes(fk.sobol_indices(A, B, want_values=True)) == _all_bytes(clean_s)
    assert _all_bytes(fk.main_effects(A, grid, want_base=True)) == _all_bytes(clean_m)
    fk.release()


# ---------------------------------------------------------------------------------------------------------------- 7
MODEL_KINDS = {
    "extend-lds-n100-d4": (MK.make_extend_lds(100, 4, np.float64, 2.5), 2.5),
    "extend-general-n90-d33": (MK.make_extend_general(33), 2.5),
    "small-fit-device-driven": (MK.make_small_fit(0, np.float64), 2.5),
    "incremental-256-300": (MK.make_incremental((256, 300)), 2.5),
}


@pytest.mark.parametrize("kind", sorted(MODEL_KINDS))
def test_every_kind_of_model(kind, monkeypatch):
    make, nu = MODEL_KINDS[kind]
    fk, X, y = make(monkeypatch)
    assert fk.nu == nu
    lo, hi = X.min(axis=0), X.max(axis=0)
    rng = np.random.default_rng(12)
    A = (lo + (hi - lo) * rng.uniform(-0.1, 1.1, (N_ROWS, fk.d))).astype(fk.dtype)
    B = (lo + (hi - lo) * rng.uniform(-0.1, 1.1, (N_ROWS, fk.d))).astype(fk.dtype)
    grid = (lo[:, None] + (hi - lo)[:, None] * rng.uniform(-0.1, 1.1, (fk.d, G_SMALL))).astype(fk.dtype)
    _check_values(fk, nu, fk.dtype, A, B, grid, kind)
    fk.release()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_arguments():
    lib = _lib.load()
    fk, d = _bits_model()
    fk32, _ = _bits_model(np.float32)
    A, B = SR.samples(d, 6, 13, np.float64)
    grid = _grid(d, 3, np.float64)
    first, total, eff = np.zeros(d), np.zeros(d), np.zeros((d, 3))
    p = _lib.dptr
    sob, me = lib.hbegp_sobol_f64, lib.hbegp_main_effects_f64
    bad_sobol = [
        (None, p(A), p(B), 6, p(first), p(total)), (fk._h, None, p(B), 6, p(first), p(total)), (fk._h, p(A), None, 6, p(first), p(total)),
        (fk._h, p(A), p(B), 6, None, p(total)), (fk._h, p(A), p(B), 6, p(first), None), (fk._h, p(A), p(B), 1, p(first), p(total)),
        (fk._h, p(A), p(B), 0, p(first), p(total)), (fk._h, p(A), p(B), -3, p(first), p(total)), (fk32._h, p(A), p(B), 6, p(first), p(total)),
    ]
    for a in bad_sobol:
        assert sob(*a, None, None, None, None, None) == _lib.EINVAL, a
        assert _lib.last_error()
    bad_me = [
        (None, p(A), 6, p(grid), 3, p(eff)), (fk._h, None, 6, p(grid), 3, p(eff)), (fk._h, p(A), 6, None, 3, p(eff)),
        (fk._h, p(A), 6, p(grid), 3, None), (fk._h, p(A), 0, p(grid), 3, p(eff)), (fk._h, p(A), -1, p(grid), 3, p(eff)),
        (fk._h, p(A), 6, p(grid), 0, p(eff)), (fk._h, p(A), 6, p(grid), -2, p(eff)), (fk32._h, p(A), 6, p(grid), 3, p(eff)),
    ]
    for a in bad_me:
        assert me(*a, None) == _lib.EINVAL, a
    assert first.any() == 0 and eff.any() == 0  # a refused call writes nothing
    # NULL optional outputs; the smallest N
    assert sob(fk._h, p(A), p(B), 2, p(first), p(total), None, None, None, None, None) == _lib.OK
    f0, V = C.c_double(), C.c_double()
    f_b = np.zeros(6)
    assert sob(fk._h, p(A), p(B), 6, p(first), p(total), C.byref(f0), C.byref(V), None, p(f_b), None) == _lib.OK
    w = fk.sobol_indices(A, B, want_values=True)
    assert first.tobytes() == w[0].tobytes() and f0.value == w[2] and V.value == w[3] and f_b.tobytes() == w[5].tobytes()
    assert me(fk._h, p(A), 1, p(grid), 3, p(eff), None) == _lib.OK
    assert eff.tobytes() == fk.main_effects(A[:1], grid).tobytes()
    assert fk.main_effects(A, grid[0]).tobytes() == fk.main_effects(A, np.broadcast_to(grid[0], (d, 3))).tobytes()  # a 1-D grid
    phases = np.zeros(4)
    lib.hbegp_debug_sens_phases(1, None)
    fk.sobol_indices(A, B)
    lib.hbegp_debug_sens_phases(0, p(phases))
    assert (phases >= 0).all() and phases[1] > 0
    fk.release()
    fk32.release()


def _surrogate(X, y, theta, nu=2.5):
    yn, y_norm = E.YNormalize.new_project_into_normalized(y, "linear")
    fk = gpr.FittedKernel.extend(X, yn, theta, nu=nu)
    return E.SurrogateModelGPR(fk, None, None, None, y_norm, np.float64)


def test_estimator_indices_are_those_of_y_and_effects_are_in_y_units():
    d, n = 4, 100
    X, y, theta = FC.inputs(d, n, np.float64)
    y = y + 3.0  # positive: the linear projection's amplitude is the mean of y - min y
    m1 = _surrogate(X, y, theta)
    m2 = _surrogate(X, 40.0 * y - 7.0, theta)  # an affine change of y, refitted at the same theta
    bounds = [(0.0, 1.0)] * (d - 1) + [(0.2, 0.8)]
    for b in (None, bounds):
        f1, t1 = m1.sobol_indices_a(256, E.RNG.new_with_seed(2), bounds=b)
        f2, t2 = m2.sobol_indices_a(256, E.RNG.new_with_seed(2), bounds=b)
        assert max(np.abs(f1 - f2).max(), np.abs(t1 - t2).max()) <= 1e-6
        assert t1.min() >= 1e-2
    order, rf, rt = E.rank_parameters(m1, 256, E.RNG.new_with_seed(2))
    assert rt.tobytes() == m1.sobol_indices_a(256, E.RNG.new_with_seed(2))[1].tobytes()
    assert list(order) == list(np.argsort(-rt, kind="stable"))
    # main effects: y units, the grid in the caller's coordinates
    grid, eff = m1.main_effects_a(64, 6, E.RNG.new_with_seed(3), bounds=bounds)
    assert grid.shape == (d, 6) and eff.shape == (d, 6)
    assert np.allclose(grid[-1], 0.2 + 0.6 * (np.arange(6) + 0.5) / 6) and np.allclose(grid[0], (np.arange(6) + 0.5) / 6)
    A = m1._uniform_rows(64, E.RNG.new_with_seed(3), bounds)
    want = np.empty((d, 6))
    for k in range(d):
        pts = SR.effect_points(A, grid, k).reshape(6 * 64, d)
        want[k] = m1.predict_mean_a(pts).reshape(6, 64).mean(axis=1)
    assert np.abs(eff - want).max() <= 1e-8 * max(1.0, np.abs(want).max())
    grid2, eff2 = m2.main_effects_a(64, 6, E.RNG.new_with_seed(3), bounds=bounds)
    assert np.abs(eff2 - (40.0 * eff - 7.0)).max() <= 1e-6 * np.abs(eff2).max()
    m1.fitted.release()
    m2.fitted.release()
