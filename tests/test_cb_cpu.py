"""CPU checks of the confidence bound (hbegp_confidence_bound_* / hbegp_minimize_confidence_bound_*): the new symbols against the
header, the refusals that need no model, the NumPy restatement (tests/cb_ref.py) -- its gradient on the fp64 oracle's posterior
against central differences of its value, its sigma = 0 and kappa = 0 branches, argmin_first -- and the estimator's host-side pieces
(predict_statistics_a, acquire_by_confidence_bound, suggest_optimum's bookkeeping) on stub models."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import cb_ref as R
import predict_grad_ref as PG
from hbetune_rs_amd import _lib
from hbetune_rs_amd import estimator as E
from oracle import gpr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hbegp_confidence_bound_f64", "hbegp_confidence_bound_f32", "hbegp_minimize_confidence_bound_f64",
       "hbegp_minimize_confidence_bound_f32", "hbegp_debug_cb_phases")


def test_cb_symbols_are_exported_with_the_headers_argument_counts():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "hbegp.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert len(_lib.SIGNATURES["hbegp_confidence_bound_f64"][1]) == 9 and len(_lib.SIGNATURES["hbegp_minimize_confidence_bound_f32"][1]) == 10
    assert lib.hbegp_version() == 200


def test_cb_calls_are_refused_before_any_device_call():
    lib = _lib.load()
    for sfx, dt in (("f64", np.float64), ("f32", np.float32)):
        fn = getattr(lib, "hbegp_confidence_bound_" + sfx)
        x, val, grad, best = np.zeros((1, 2), dt), np.full(1, 7.0), np.full((1, 2), 7.0, dt), C.c_int(5)
        mean, var = np.full(1, 7.0, dt), np.full(1, 7.0, dt)

        def call(kappa=1.0, m=1, xs=x, out=val):
            return fn(None, _lib.aptr(xs), m, kappa, _lib.dptr(out), _lib.aptr(grad), C.byref(best), _lib.aptr(mean), _lib.aptr(var))

        for kw, what in ((dict(), "NULL model"), (dict(kappa=math.nan), "kappa is not finite"), (dict(kappa=math.inf), "kappa is not finite"),
                         (dict(kappa=-math.inf), "kappa is not finite"), (dict(m=-1), "m must be >= 0"), (dict(xs=None), "Xs/cb is NULL"),
                         (dict(out=None), "Xs/cb is NULL"), (dict(m=0), "NULL model")):
            assert call(**kw) == _lib.EINVAL and what in _lib.last_error(), (kw, _lib.last_error())
        assert val[0] == 7.0 and (grad == 7).all() and best.value == 5 and mean[0] == 7 and var[0] == 7  # a refused call writes nothing

        fn = getattr(lib, "hbegp_minimize_confidence_bound_" + sfx)
        lo, hi, xo, vo, ne = np.zeros(2), np.ones(2), np.full((1, 2), 7.0, dt), np.full(1, 7.0), np.full(1, 7, np.int32)

        def minimize(starts=x, S=1, lo=lo, hi=hi, kappa=1.0, maxeval=10, x_out=xo, v_out=vo):
            return fn(None, _lib.aptr(starts), S, _lib.dptr(lo), _lib.dptr(hi), kappa, maxeval, _lib.aptr(x_out), _lib.dptr(v_out),
                      ne.ctypes.data_as(C.POINTER(C.c_int)))

        for kw, what in ((dict(), "NULL model"), (dict(S=0), "S must be >= 1"), (dict(kappa=math.nan), "kappa is not finite"),
                         (dict(kappa=math.inf), "kappa is not finite"), (dict(starts=None), "starts/lo/hi/x_out/cb_out is NULL"),
                         (dict(lo=None), "starts/lo/hi/x_out/cb_out is NULL"), (dict(hi=None), "starts/lo/hi/x_out/cb_out is NULL"),
                         (dict(x_out=None), "starts/lo/hi/x_out/cb_out is NULL"), (dict(v_out=None), "starts/lo/hi/x_out/cb_out is NULL"),
                         (dict(maxeval=0), "maxeval must be >= 1"),
                         # lo > hi and a start outside the box are checked against the model's d: without a model the call stops at
                         # the model (tests/test_gpu_cb.py checks both messages on a real one)
                         (dict(lo=hi, hi=lo), "NULL model"), (dict(starts=np.full((1, 2), 1.5, dt)), "NULL model")):
            assert minimize(**kw) == _lib.EINVAL and what in _lib.last_error(), (kw, _lib.last_error())
        assert (xo == 7).all() and vo[0] == 7.0 and ne[0] == 7
    ph = np.full(3, -1.0)
    assert lib.hbegp_debug_cb_phases(0, _lib.dptr(ph)) == _lib.OK
    assert ph[2] == -1.0 and np.isfinite(ph[:2]).all()  # two phases, nothing past them
    assert lib.hbegp_debug_cb_phases(0, None) == _lib.OK


def _problem(nu, n=30, d=3, seed=0):
    """tests/test_predict_grad_cpu.py's problem: the oracle's alpha and K^-1, query points away from the training points."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    amp, noise = 1.7, 1e-2
    ell = np.array([0.3, 0.5, 0.8][:d])
    res = O.lml_with_gradient(X, y, noise, amp, ell, nu)
    Xs = rng.uniform(0, 1, (40, d))
    dist = np.sqrt((((Xs / ell)[:, None, :] - (X / ell)[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
    return X, res["alpha"], res["k_inv"], amp, ell, Xs[dist > 0.05][:12], noise


@pytest.mark.parametrize("kappa", [-2.0, 1.0, 3.0])
@pytest.mark.parametrize("nu", [0.5, 1.5, 2.5, math.inf])
def test_restated_gradient_matches_central_differences_of_the_restated_value(nu, kappa):
    """The restatement's gradient on the oracle's posterior (predict_grad_ref's dmean and dvar) against central differences of
    the restatement's value on the oracle's predict: the step (1e-5 ell_k) and the row bar (1e-6) of
    tests/test_predict_grad_cpu.py, at points whose variance stays above 1e-6."""
    X, alpha, kinv, amp, ell, Xs, noise = _problem(nu)
    m, d = Xs.shape
    mean, var, _ = O.predict(Xs, X, alpha, kinv, amp, ell, nu)
    assert (var > 1e-6).all()  # no clamped variance, and sigma far above the sigma = 0 branch
    _, grad, _ = R.cb_grad(mean, var, PG.dmean_ref(Xs, X, alpha, amp, ell, nu), PG.dvar_ref(Xs, X, amp, ell, nu, noise), kappa)
    fd = np.zeros((m, d))
    zeros = np.zeros((m, d))
    for k in range(d):
        h = 1e-5 * ell[k]
        xp, xm = Xs.copy(), Xs.copy()
        xp[:, k] += h
        xm[:, k] -= h
        mp, vp, _ = O.predict(xp, X, alpha, kinv, amp, ell, nu)
        mm, vm, _ = O.predict(xm, X, alpha, kinv, amp, ell, nu)
        assert (vp > 1e-6).all() and (vm > 1e-6).all()
        fd[:, k] = (R.cb_grad(mp, vp, zeros, zeros, kappa)[0] - R.cb_grad(mm, vm, zeros, zeros, kappa)[0]) / (2 * h)
    dev = PG.row_dev(grad, fd)
    print(f"nu={nu} kappa={kappa}: gradient against central differences {dev:.1e}")
    assert dev < 1e-6, dev


def test_restatement_branches():
    mean, var = np.array([0.3, -1.2, 0.5, math.nan, 0.1, 2.0]), np.array([0.04, 0.0, 1e-40, 0.2, math.nan, 0.25])
    dmean, dvar = np.arange(12.0).reshape(6, 2) - 3.0, np.arange(12.0).reshape(6, 2)[::-1] * 0.1
    cb, grad, scale = R.cb_grad(mean, var, dmean, dvar, 2.0)
    assert cb[0] == 0.3 + 2.0 * 0.2 and np.array_equal(grad[0], dmean[0] + 2.0 * (dvar[0] / 0.4))
    for j in (1, 2):  # sigma = 0 and sigma = 1e-20 <= eps: the sigma term is dropped, never divided
        assert cb[j] == mean[j] and np.array_equal(grad[j], dmean[j])
    for j in (3, 4):
        assert math.isnan(cb[j]) and np.isnan(grad[j]).all()
    assert cb[5] == 3.0 and np.isfinite(scale[[0, 1, 2, 5]]).all()
    cb0, grad0, _ = R.cb_grad(mean, var, dmean, dvar, 0.0)
    keep = [0, 1, 2, 5]
    assert np.array_equal(cb0[keep], mean[keep]) and np.array_equal(grad0[keep], dmean[keep])
    cbn, _, _ = R.cb_grad(mean, var, dmean, dvar, -2.0)
    assert cbn[0] == 0.3 - 2.0 * 0.2
    assert R.value_bar(np.float64, [0.5, -30.0, math.nan]).tolist() == [1e-8, 3e-7, 0.0]
    assert R.grad_bar(np.float32, [0.5, -30.0], [0.1, 4.0]).tolist() == [1e-4, 1e-4 * 30.0 * 4.0]


def test_argmin_first():
    nan = math.nan
    assert R.argmin_first([3.0]) == 0 and R.argmin_first([]) == -1
    assert R.argmin_first([2.0, 1.0, 1.0, 5.0, 1.0]) == 1  # ties: the first
    assert R.argmin_first([nan, 4.0, nan, 4.0, 7.0]) == 1  # a NaN never wins
    assert R.argmin_first([nan, nan]) == -1 and R.argmin_first([nan]) == -1
    assert R.argmin_first([nan, nan, -math.inf, -math.inf]) == 2 and R.argmin_first([math.inf, nan]) == 0
    assert R.argmin_first([0.0, -0.0]) == 0  # equal values


class _StubFitted:
    """FittedKernel.predict of a fixed posterior: mean and variance are functions of the row (no GPU needed)."""

    def __init__(self, dtype, d=2):
        self.dtype, self.d, self.calls = np.dtype(dtype), d, 0

    def predict(self, x, want_variance=True):
        self.calls += 1
        x = np.asarray(x, dtype=self.dtype)
        mean = (np.sin(3.0 * x[:, 0]) + x[:, 1]).astype(self.dtype)
        var = np.where(x[:, 0] < 0.2, 0.0, 0.05 + 0.3 * x[:, 1] ** 2).astype(self.dtype)  # rows with x_0 < 0.2: sigma = 0
        return mean, var, 0


@pytest.mark.parametrize("projection", ["linear", "logarithmic"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=lambda t: np.dtype(t).name)
def test_predict_statistics_a_matches_the_scalar_method_row_by_row(dtype, projection):
    fitted = _StubFitted(dtype)
    fitted.lml = 0.0
    model = E.SurrogateModelGPR(fitted, None, None, None, E.YNormalize(1.3, 0.4, projection), dtype)
    x = np.random.default_rng(5).uniform(0, 1, (9, 2)).astype(dtype)
    assert (x[:, 0] < 0.2).any() and (x[:, 0] >= 0.2).any()
    stats = model.predict_statistics_a(x)
    assert fitted.calls == 1 and len(stats) == 9  # one predict for all rows
    for i in range(9):
        s = model.predict_statistics(x[i])
        for a, b in ((stats[i].mean(), s.mean()), (stats[i].std(), s.std()), (stats[i].cv(), s.cv()), (stats[i].q1, s.q1),
                     (stats[i].q2, s.q2), (stats[i].q3, s.q3), (stats[i].median(), s.median()), (stats[i].iqr(), s.iqr())):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (i, a, b)
        assert stats[i].q1 <= stats[i].q2 <= stats[i].q3


class _StubModel:
    """Stands in for SurrogateModelGPR: the bound is a coarse function of the first feature, so that there are plenty of ties."""

    dtype = np.dtype(np.float64)

    def __init__(self):
        self.minimised = None

    def predict_confidence_bound_a(self, x, cb):
        x = np.asarray(x)
        return np.round(np.sin(7.0 * x[:, 0]), 1) + cb * 0.0

    def predict_mean(self, x):
        return float(np.asarray(x).sum())

    def predict_mean_ei(self, x, fmin):
        return float(np.asarray(x).sum()), float(fmin) + 100.0

    def minimize_confidence_bound(self, starts, bounds, cb, maxeval=150):
        self.minimised = np.array(starts)
        bound = self.predict_confidence_bound_a(starts, cb) - np.array([0.0, 0.5, 0.5, 0.2][:len(starts)])  # runs 1 and 2 end equal
        return starts * 0.5, bound, np.full(len(starts), 3, np.int32)


def test_acquire_by_confidence_bound_orders_by_a_stable_sort():
    cand = np.random.default_rng(3).random((40, 3))
    model = _StubModel()
    bound = model.predict_confidence_bound_a(cand, 1.0)
    assert len(np.unique(bound)) < 25  # ties
    idx, val = E.acquire_by_confidence_bound(cand, model, 12, 1.0)
    want = sorted(range(40), key=lambda i: (bound[i], i))[:12]
    assert idx.tolist() == want and idx.dtype == np.int64 and np.array_equal(val, bound[want])
    assert E.acquire_by_confidence_bound(cand, model, 0, -2.0)[0].shape == (0,)
    assert E.acquire_by_confidence_bound(cand, model, 40, -2.0)[0].tolist() == sorted(range(40), key=lambda i: (bound[i], i))
    with pytest.raises(ValueError):
        E.acquire_by_confidence_bound(cand, model, 41, 1.0)
    with pytest.raises(ValueError):
        E.acquire_by_confidence_bound(cand[0], model, 1, 1.0)

    class Bad(_StubModel):
        def predict_confidence_bound_a(self, x, cb):
            b = super().predict_confidence_bound_a(x, cb)
            b[3] = math.nan
            return b

    with pytest.raises(ValueError, match="comparable"):
        E.acquire_by_confidence_bound(cand, Bad(), 2, 1.0)


def test_suggest_optimum_bookkeeping_on_a_stub():
    """The scan's winner starts run 0, the next-lowest DISTINCT individuals the further runs; the lowest run wins, ties to the lower
    run index; EI is taken against the scan winner's predicted mean."""
    feats = np.random.default_rng(8).random((30, 3))
    feats[11] = feats[4]  # a duplicate point: it must not start a second run
    model = _StubModel()
    bound = model.predict_confidence_bound_a(feats, 1.0)
    order = sorted(range(30), key=lambda i: (bound[i], i))
    start, sy = E.find_best_individual_by_confidence_bound(feats, model, 1.0)
    assert start == order[0]
    x, b, mean, ei, idx = E.suggest_optimum(feats, model, confidence_bound=1.0)
    assert idx == start and model.minimised.shape == (1, 3) and np.array_equal(model.minimised[0], feats[start])
    assert np.array_equal(x, feats[start] * 0.5) and b == bound[start] and mean == x.sum() and ei == sy + 100.0
    x4, b4, _, ei4, idx4 = E.suggest_optimum(feats, model, confidence_bound=1.0, n_starts=4)
    rows = []
    for i in order:
        if len(rows) < 4 and not any((feats[i] == feats[r]).all() for r in rows):
            rows.append(i)
    assert np.array_equal(model.minimised, feats[rows]) and idx4 == start and ei4 == sy + 100.0
    ends = bound[rows] - np.array([0.0, 0.5, 0.5, 0.2])
    run = min(range(4), key=lambda r: (ends[r], r))
    assert b4 == ends[run] and np.array_equal(x4, feats[rows[run]] * 0.5) and b4 <= b
    assert E.suggest_optimum(feats[:2], model, n_starts=5)[4] in (0, 1) and len(model.minimised) == 2  # fewer individuals than runs
