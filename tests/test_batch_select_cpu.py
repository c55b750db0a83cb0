"""CPU checks of the greedy batch selection by EI (hbegp_select_batch_*): the symbols and their signatures, register use of the
new kernel, argument checks that refuse before any device call, the NumPy restatement (tests/batch_select_ref.py) against the
oracle's closed-form predict on the training set augmented with the fantasies, k = 1 against find_best_candidate_by_ei, and
the estimator's projection of fmin and the lie on a model stand-in."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import batch_select_ref as BS
import posterior_cov_ref as PC
from hbetune_rs_amd import _lib
from hbetune_rs_amd import estimator as E
from oracle import gpr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ("hbegp_select_batch_f64", "hbegp_select_batch_f32")
NUS = [0.5, 1.5, 2.5, math.inf]


def test_select_symbols_are_exported_with_signatures():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def _kernel_notes(isa):
    """name -> {key: int} from the amdhsa metadata (one YAML block per kernel)."""
    out = {}
    meta = isa[isa.index("amdhsa.kernels:"):]
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+_count|private_segment_fixed_size):\s+(\d+)", block)}
    return out


def test_batch_select_kernel_does_not_spill():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", ROOT, "build/kernels.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "build", "kernels.s")) as f:
        notes = _kernel_notes(f.read())
    found = [k for k in notes if "batch_select_kernel" in k]
    assert len(found) == 2, found  # f64 and f32
    for sym in found:
        assert notes[sym]["vgpr_spill_count"] == 0 and notes[sym]["sgpr_spill_count"] == 0, (sym, notes[sym])
        assert notes[sym]["private_segment_fixed_size"] == 0, (sym, notes[sym])
        assert notes[sym]["vgpr_count"] <= 128, (sym, notes[sym])  # 1024 threads: 16 waves on one CU


def _einval(rc, what):
    assert rc == _lib.EINVAL
    assert what in _lib.last_error(), _lib.last_error()


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    d, f = _lib.dptr, _lib.fptr
    x, out = np.zeros(8), np.zeros(8)
    xf, outf = np.zeros(8, np.float32), np.zeros(8, np.float32)
    idx = np.zeros(4, np.int32)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int))
    ei = np.zeros(4)
    good, nan, inf = C.c_double(0.5), C.c_double(math.nan), C.c_double(-math.inf)
    for fn, xp, op in ((lib.hbegp_select_batch_f64, d(x), d(out)), (lib.hbegp_select_batch_f32, f(xf), f(outf))):
        _einval(fn(None, xp, 2, 1, 0.0, None, ip, d(ei), op, op), "NULL model")
        _einval(fn(None, xp, 2, 1, 0.0, C.byref(good), ip, None, None, None), "NULL model")
        _einval(fn(None, xp, -1, 0, 0.0, None, ip, d(ei), op, op), "m must be >= 0")
        _einval(fn(None, xp, 2, -1, 0.0, None, ip, d(ei), op, op), "k must be >= 0")
        _einval(fn(None, xp, 2, 3, 0.0, None, ip, d(ei), op, op), "k must be <= m")
        _einval(fn(None, xp, 0, 1, 0.0, None, ip, d(ei), op, op), "k must be <= m")
        _einval(fn(None, xp, 2, 1, 0.0, None, None, d(ei), op, op), "idx is NULL")
        for bad in (math.nan, math.inf, -math.inf):
            _einval(fn(None, xp, 2, 1, bad, None, ip, d(ei), op, op), "fmin must be finite")
        _einval(fn(None, xp, 2, 1, 0.0, C.byref(nan), ip, d(ei), op, op), "lie must be finite")
        _einval(fn(None, xp, 2, 1, 0.0, C.byref(inf), ip, d(ei), op, op), "lie must be finite")
    # k = 0 with a NULL idx is allowed by the checks; it still needs a model
    _einval(lib.hbegp_select_batch_f64(None, d(x), 2, 0, 0.0, None, None, None, None, None), "NULL model")
    # (the element type and a non-finite query coordinate need a model: tests/test_gpu_batch_select.py)


def _problem(n=40, d=3, m=30, seed=0, noise=1e-2):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    amp = 1.7
    ell = np.array([0.3, 0.5, 0.8][:d])
    Xs = rng.uniform(-0.1, 1.1, (m, d))
    return X, y, amp, noise, ell, Xs


def _posterior(X, y, amp, noise, ell, nu, Xs):
    res = O.lml_with_gradient(X, y, noise, amp, ell, nu)
    mean, _, _ = O.predict(Xs, X, res["alpha"], res["k_inv"], amp, ell, nu)
    return mean, PC.sigma_ref(Xs, X, amp, ell, nu, noise)


@pytest.mark.parametrize("lie", [None, "low", "high"])
@pytest.mark.parametrize("nu", NUS)
def test_restatement_is_closed_form_conditioning(nu, lie):
    X, y, amp, noise, ell, Xs = _problem(seed=int(nu) if math.isfinite(nu) else 7)
    mean, S = _posterior(X, y, amp, noise, ell, nu, Xs)
    fmin = float(y.min())
    L = None if lie is None else (fmin - 0.3 if lie == "low" else float(y.max()))
    k = 8
    r = BS.select(mean, S, noise, fmin, k, lie=L)
    assert len(set(r["idx"].tolist())) == k
    for t in range(1, k + 1):
        Xa = np.vstack([X, Xs[r["idx"][:t]]])
        ya = np.concatenate([y, r["fantasy"][:t]])
        res = O.lml_with_gradient(Xa, ya, noise, amp, ell, nu)
        om, ov, _ = O.predict(Xs, Xa, res["alpha"], res["k_inv"], amp, ell, nu)
        mu_t, v_t = r["history"][t - 1]
        dm = float(np.abs(mu_t - om).max())
        dv = float(np.abs(np.maximum(v_t, 0.0) - ov).max())
        assert dm <= 1e-10 * amp and dv <= 1e-10 * amp, (t, dm, dv)
    if lie is None:
        assert np.array_equal(r["mean"], mean)  # the kriging believer never moves the mean
        assert np.array_equal(r["fantasy"], mean[r["idx"]])


def test_restatement_ei_is_the_estimators():
    X, y, amp, noise, ell, Xs = _problem(m=60, seed=2)
    mean, S = _posterior(X, y, amp, noise, ell, 2.5, Xs)
    var = np.diag(S).copy()
    var[:3] = [0.0, -1e-9, 1e-40]  # the std <= EPSILON branch, on both sides of fmin
    mean[:3] = [y.min() - 1, y.min() + 1, y.min() - 0.5]
    e = BS.expected_improvement(mean, var, float(y.min()))
    for i in range(len(mean)):
        want = E.expected_improvement(float(mean[i]), math.sqrt(max(var[i], 0.0)), float(y.min()))
        assert abs(e[i] - want) <= 1e-15 * max(1.0, want), (i, e[i], want)


class _EIModel:
    """A stand-in for SurrogateModelGPR with fixed (mean, var) per candidate row (looked up by row index)."""

    def __init__(self, mean, var):
        self.mean, self.var = mean, var

    def predict_mean_ei_a(self, x, fmin):
        rows = np.asarray(x)[:, 0].astype(int)
        m, v = self.mean[rows], self.var[rows]
        return m, np.array([E.expected_improvement(float(a), math.sqrt(max(b, 0.0)), fmin) for a, b in zip(m, v)])


def test_k1_is_find_best_candidate_by_ei_and_ties_go_to_the_last_index():
    X, y, amp, noise, ell, Xs = _problem(m=25, seed=3)
    mean, S = _posterior(X, y, amp, noise, ell, 1.5, Xs)
    fmin = float(y.min())
    rows = np.arange(25, dtype=float)[:, None]
    model = _EIModel(mean, np.diag(S))
    i, _, ei = E.find_best_candidate_by_ei(rows, model, fmin)
    r = BS.select(mean, S, noise, fmin, 1)
    assert r["idx"][0] == i and abs(r["ei"][0] - ei) <= 1e-15 * max(1.0, ei)
    # a tie: the best row duplicated at a later index (same mean, same row and column of Sigma)
    order = list(range(25)) + [i]
    mean2, S2 = mean[order], S[np.ix_(order, order)]
    r2 = BS.select(mean2, S2, noise, fmin, 2)
    assert r2["idx"][0] == 25  # the last of the two maxima
    i2, _, _ = E.find_best_candidate_by_ei(np.arange(26, dtype=float)[:, None], _EIModel(mean2, np.diag(S2)), fmin)
    assert i2 == 25
    # after the fantasy at row 25 its twin keeps (almost) no variance: the second pick is another row
    assert r2["idx"][1] != i


@pytest.mark.parametrize("lie", [None, 0.0])
def test_picks_are_distinct_and_prefixes_agree(lie):
    X, y, amp, noise, ell, Xs = _problem(m=40, seed=4)
    mean, S = _posterior(X, y, amp, noise, ell, 2.5, Xs)
    full = BS.select(mean, S, noise, float(y.min()), 40, lie=lie)
    assert sorted(full["idx"].tolist()) == list(range(40))  # k = m: a permutation
    for t in (1, 5, 17):
        part = BS.select(mean, S, noise, float(y.min()), t, lie=lie)
        assert np.array_equal(part["idx"], full["idx"][:t]) and np.array_equal(part["ei"], full["ei"][:t])
    # the EI of each pick is that step's maximum
    assert np.array_equal(full["ei"], full["best"])


class _FakeFitted:
    """A stand-in for gpr.FittedKernel: select_batch through the restatement on a fixed (mean, Sigma), predict from the mean."""

    def __init__(self, mean, sigma, s2):
        self.mean, self.sigma, self.s2 = mean, sigma, s2
        self.lml = 0.0
        self.calls = []

    def select_batch(self, x, k, fmin_normalized, lie=None):
        self.calls.append((np.array(x), k, fmin_normalized, lie))
        r = BS.select(self.mean, self.sigma, self.s2, fmin_normalized, k, lie=lie)
        return r["idx"], r["ei"], r["mean"], r["var"]

    def predict(self, x, want_variance=True):
        rows = np.asarray(x)[:, 0].astype(int)
        return self.mean[rows], None, 0


@pytest.mark.parametrize("projection", ["linear", "logarithmic"])
def test_estimator_projects_fmin_and_the_lie(projection):
    X, y, amp, noise, ell, Xs = _problem(m=30, seed=5)
    mean, S = _posterior(X, y, amp, noise, ell, 2.5, Xs)
    y_obs = np.exp(y) + 3.0  # positive, for the logarithmic projection
    _, yn = E.YNormalize.new_project_into_normalized(y_obs, projection)
    fake = _FakeFitted(mean, S, noise)
    model = E.SurrogateModelGPR(fake, (1e-5, 1e5), (1e-3, 1e3), [(1e-3, 1e3)] * 3, yn, np.float64)
    rows = np.arange(30, dtype=float)[:, None]
    fmin = float(y_obs.min())
    lie = float(np.median(y_obs))
    for L in (None, lie):
        idx, means, ei = E.acquire_by_batch_ei(rows, model, 6, fmin, lie=L)
        _, k, fmin_n, lie_n = fake.calls[-1]
        assert k == 6
        assert fmin_n == float(yn.project_into_normalized(np.array([fmin]))[0])
        assert lie_n == (None if L is None else float(yn.project_into_normalized(np.array([L]))[0]))
        r = BS.select(mean, S, noise, fmin_n, 6, lie=lie_n)
        assert np.array_equal(idx, r["idx"]) and np.array_equal(ei, r["ei"])
        assert np.array_equal(means, yn.project_location_from_normalized(mean[r["idx"]]))
        assert (idx, means, ei)[0].dtype == np.int64
    with pytest.raises(ValueError):
        E.acquire_by_batch_ei(rows[:, 0], model, 2, fmin)
