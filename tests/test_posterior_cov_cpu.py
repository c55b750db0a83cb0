"""CPU checks of the joint-posterior feature (hbegp_predict_cov_*, hbegp_sample_posterior_*): the symbols and their signatures,
register use of the new kernels, argument checks that refuse before any device call, the NumPy restatement of Sigma
(tests/posterior_cov_ref.py) against the oracle's predict and against scikit-learn, the caller-side normals
(RNG.standard_normal) and the Thompson selection on a model stand-in."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import posterior_cov_ref as PC
from hbetune_rs_amd import _lib
from hbetune_rs_amd import estimator as E
from oracle import gpr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ("hbegp_predict_cov_f64", "hbegp_predict_cov_f32", "hbegp_sample_posterior_f64", "hbegp_sample_posterior_f32")
NUS = [0.5, 1.5, 2.5, math.inf]


def test_posterior_symbols_are_exported_with_signatures():
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


def test_new_kernels_do_not_spill():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", ROOT, "build/kernels.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "build", "kernels.s")) as f:
        notes = _kernel_notes(f.read())
    found = [k for k in notes if "leaf_keep_kernel" in k or "sample_epilogue_kernel" in k]
    assert len(found) == 4, found  # two element types each
    for sym in found:
        assert notes[sym]["vgpr_spill_count"] == 0 and notes[sym]["sgpr_spill_count"] == 0, (sym, notes[sym])
        assert notes[sym]["private_segment_fixed_size"] == 0, (sym, notes[sym])
        assert notes[sym]["vgpr_count"] <= 128, (sym, notes[sym])  # leaf_keep_kernel: 512 threads, 2 workgroups per CU


def _einval(rc, what):
    assert rc == _lib.EINVAL
    assert what in _lib.last_error(), _lib.last_error()


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    d, f = _lib.dptr, _lib.fptr
    x, z, out = np.zeros(8), np.zeros(8), np.zeros(8)
    xf, zf, outf = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.float32)
    amin = np.zeros(4, np.int32)
    ip = amin.ctypes.data_as(_lib.SIGNATURES["hbegp_sample_posterior_f64"][1][7])
    # predict_cov
    _einval(lib.hbegp_predict_cov_f64(None, d(x), 2, 0.0, d(out), d(out)), "NULL model")
    _einval(lib.hbegp_predict_cov_f32(None, f(xf), 2, 0.0, f(outf), f(outf)), "NULL model")
    _einval(lib.hbegp_predict_cov_f64(None, d(x), -1, 0.0, d(out), d(out)), "m must be >= 0")
    _einval(lib.hbegp_predict_cov_f32(None, f(xf), -2, 0.0, f(outf), f(outf)), "m must be >= 0")
    for bad in (-1e-3, math.nan, math.inf):
        _einval(lib.hbegp_predict_cov_f64(None, d(x), 2, bad, d(out), d(out)), "jitter")
        _einval(lib.hbegp_predict_cov_f32(None, f(xf), 2, bad, f(outf), f(outf)), "jitter")
    # sample_posterior
    _einval(lib.hbegp_sample_posterior_f64(None, d(x), 2, d(z), 1, 0.0, d(out), ip, None), "NULL model")
    _einval(lib.hbegp_sample_posterior_f32(None, f(xf), 2, f(zf), 1, 0.0, f(outf), ip, None), "NULL model")
    _einval(lib.hbegp_sample_posterior_f64(None, d(x), -1, d(z), 1, 0.0, d(out), ip, None), "m must be >= 0")
    _einval(lib.hbegp_sample_posterior_f64(None, d(x), 2, d(z), 0, 0.0, d(out), ip, None), "S must be >= 1")
    _einval(lib.hbegp_sample_posterior_f32(None, f(xf), 2, f(zf), -3, 0.0, f(outf), ip, None), "S must be >= 1")
    _einval(lib.hbegp_sample_posterior_f64(None, d(x), 2, None, 1, 0.0, d(out), ip, None), "z is NULL")
    _einval(lib.hbegp_sample_posterior_f32(None, f(xf), 2, None, 1, 0.0, f(outf), ip, None), "z is NULL")
    _einval(lib.hbegp_sample_posterior_f64(None, d(x), 2, d(z), 1, 0.0, None, None, None), "both NULL")
    _einval(lib.hbegp_sample_posterior_f32(None, f(xf), 2, f(zf), 1, 0.0, None, None, None), "both NULL")
    for bad in (-1.0, math.nan, -math.inf):
        _einval(lib.hbegp_sample_posterior_f64(None, d(x), 2, d(z), 1, bad, d(out), ip, None), "jitter")
        _einval(lib.hbegp_sample_posterior_f32(None, f(xf), 2, f(zf), 1, bad, None, ip, None), "jitter")
    # (the element type and a non-finite query coordinate need a model: tests/test_gpu_posterior_cov.py)


def _problem(nu, n=40, d=3, m=25, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    amp, noise = 1.7, 1e-2
    ell = np.array([0.3, 0.5, 0.8][:d])
    Xs = rng.uniform(-0.1, 1.1, (m, d))
    return X, y, amp, noise, ell, Xs


@pytest.mark.parametrize("nu", NUS)
def test_restatement_diagonal_is_the_oracles_variance(nu):
    X, y, amp, noise, ell, Xs = _problem(nu)
    res = O.lml_with_gradient(X, y, noise, amp, ell, nu)
    _, var, below = O.predict(Xs, X, res["alpha"], res["k_inv"], amp, ell, nu)
    assert not below and (var > 0).all()  # nothing clamped: the oracle's variance is the raw one
    S = PC.sigma_ref(Xs, X, amp, ell, nu, noise)
    assert np.abs(np.diag(S) - var).max() <= 1e-12 * amp
    assert np.array_equal(S, S) and np.abs(S - S.T).max() <= 1e-13 * amp
    Sk = PC.sigma_ref_kinv(Xs, X, res["k_inv"], amp, ell, nu)
    assert np.abs(Sk - S).max() <= 1e-10 * amp
    # jitter moves the diagonal only
    Sj = PC.sigma_ref(Xs, X, amp, ell, nu, noise, jitter=0.25)
    off = ~np.eye(len(S), dtype=bool)
    assert np.array_equal(Sj[off], S[off]) and np.allclose(np.diag(Sj) - np.diag(S), 0.25, rtol=0, atol=1e-14)


@pytest.mark.parametrize("nu", NUS)
def test_restatement_matches_sklearn_return_cov(nu):
    gp = pytest.importorskip("sklearn.gaussian_process")
    kernels = pytest.importorskip("sklearn.gaussian_process.kernels")
    X, y, amp, noise, ell, Xs = _problem(nu, seed=3)
    kern = kernels.ConstantKernel(amp, constant_value_bounds="fixed") * kernels.Matern(length_scale=ell, length_scale_bounds="fixed",
                                                                                      nu=nu)
    reg = gp.GaussianProcessRegressor(kernel=kern, alpha=noise, optimizer=None, normalize_y=False).fit(X, y)
    _, cov = reg.predict(Xs, return_cov=True)
    S = PC.sigma_ref(Xs, X, amp, ell, nu, noise)
    assert np.abs((S - O.MIN_NOISE * np.eye(len(S))) - cov).max() <= 1e-10 * amp


def test_draws_restatement_has_the_covariance():
    X, y, amp, noise, ell, Xs = _problem(2.5, m=6)
    S = PC.sigma_ref(Xs, X, amp, ell, 2.5, noise)
    z = E.RNG(11).standard_normal((40000, 6))
    draws = PC.draws_ref(np.zeros(6), S, z)
    C = np.cov(draws.T)
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S * S) / len(z))
    assert (np.abs(C - S) <= 5 * se).all()


def test_standard_normal_is_deterministic_finite_and_normal():
    a = E.RNG(42).standard_normal((300, 7))
    b = E.RNG(42).standard_normal((300, 7))
    assert a.shape == (300, 7) and a.tobytes() == b.tobytes()
    r = E.RNG(42)
    first, second = r.standard_normal(1000), r.standard_normal(1000)
    assert not np.array_equal(first, second)  # successive calls advance the stream
    assert E.RNG(5).standard_normal(3).shape == (3,)
    z = E.RNG(7).standard_normal(200001)  # odd count: the last pair is cut
    assert z.shape == (200001,) and np.isfinite(z).all()
    n = len(z)
    assert abs(z.mean()) < 5 / math.sqrt(n)
    assert abs(z.var() - 1) < 5 * math.sqrt(2 / n)
    assert abs((z ** 3).mean()) < 5 * math.sqrt(15 / n)
    assert abs((z ** 4).mean() - 3) < 5 * math.sqrt(96 / n)
    assert abs((np.abs(z) > 1.959964).mean() - 0.05) < 5 * math.sqrt(0.05 * 0.95 / n)


def test_standard_normal_maps_a_zero_uniform_away(monkeypatch):
    # a stream that starts with u = 0 (the smallest value SplitMix64 can give) still gives finite normals
    monkeypatch.setattr(E, "splitmix64_uniform_fast", lambda seed, count: np.zeros(count))
    z = E.RNG(1).standard_normal(6)
    assert np.isfinite(z).all() and (z == 0).all()


class _FakeFitted:
    """A stand-in for gpr.FittedKernel: draws mean + L z from a fixed Sigma on the host."""

    def __init__(self, mean, sigma):
        self.mean, self.sigma = mean, sigma
        self.calls = []

    def sample_posterior(self, x, z, jitter=0.0, want_samples=True):
        self.calls.append((np.array(x), np.array(z), jitter, want_samples))
        s = PC.draws_ref(self.mean, self.sigma, z)
        return (s if want_samples else None), np.argmin(s, axis=1).astype(np.int32)


class _FakeModel:
    def __init__(self, fitted):
        self.fitted = fitted
        self.dtype = np.dtype(np.float64)


def test_acquire_by_thompson_is_a_numpy_argmin_on_a_fake_model():
    X, y, amp, noise, ell, Xs = _problem(1.5, m=30, seed=5)
    S = PC.sigma_ref(Xs, X, amp, ell, 1.5, noise)
    mean = np.linspace(0.5, -0.5, 30)
    fake = _FakeFitted(mean, S)
    idx = E.acquire_by_thompson(Xs, _FakeModel(fake), 9, E.RNG(3))
    assert idx.shape == (9,)
    z = E.RNG(3).standard_normal((9, 30))
    assert np.array_equal(idx, np.argmin(PC.draws_ref(mean, S, z), axis=1))
    x_seen, z_seen, _, want = fake.calls[0]
    assert np.array_equal(x_seen, Xs) and np.array_equal(z_seen, z) and want is False
    with pytest.raises(ValueError):
        E.acquire_by_thompson(Xs[0], _FakeModel(fake), 2, E.RNG(3))
