"""CPU checks of noisy expected improvement over a candidate set (hbegp_noisy_ei_*): the symbols and their signatures against the
header, argument checks that refuse before any device call, register use of the new kernels, the NumPy restatement
(tests/nei_ref.py) against plain Monte Carlo over joint draws of its meaning, the restatement's own properties, and the
estimator's methods on a model stand-in."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kg_ref as KG
import nei_ref as NEI
import posterior_cov_ref as PC
from hbetune_rs_amd import _lib
from hbetune_rs_amd import estimator as E
from oracle import gpr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ("hbegp_noisy_ei_f64", "hbegp_noisy_ei_f32", "hbegp_debug_nei_phases")


def test_nei_symbols_are_exported_with_the_headers_argument_counts():
    lib = _lib.load()
    assert lib.hbegp_version() == 200
    with open(os.path.join(ROOT, "include", "hbegp.h")) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def _einval(rc, what):
    assert rc == _lib.EINVAL
    assert what in _lib.last_error(), _lib.last_error()


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    d, f = _lib.dptr, _lib.fptr
    x, xf = np.zeros(8), np.zeros(8, np.float32)
    z, zf = np.zeros(8), np.zeros(8, np.float32)
    nei, fm, rho = np.full(4, 7.0), np.full(4, 7.0), np.full(4, 7.0)
    best, info = C.c_int(7), C.c_int(7)
    bp, ip = C.byref(best), C.byref(info)
    for fn, xp, zp in ((lib.hbegp_noisy_ei_f64, d(x), d(z)), (lib.hbegp_noisy_ei_f32, f(xf), f(zf))):
        out = (d(nei), bp, d(fm), d(rho), ip)
        _einval(fn(None, xp, 2, 1, zp, 3, 0.0, *out), "NULL model")
        _einval(fn(None, xp, 2, 2, zp, 3, 0.0, None, None, None, None, None), "NULL model")  # mc = 0 needs no nei
        _einval(fn(None, xp, 0, 0, zp, 3, 0.0, *out), "m must be >= 1")
        _einval(fn(None, xp, -1, 1, zp, 3, 0.0, *out), "m must be >= 1")
        _einval(fn(None, xp, 2, 0, zp, 3, 0.0, *out), "mb must be >= 1")
        _einval(fn(None, xp, 2, 3, zp, 3, 0.0, *out), "mb must be <= m")
        _einval(fn(None, xp, 2, 1, zp, 0, 0.0, *out), "S must be >= 1")
        _einval(fn(None, xp, 2, 1, None, 3, 0.0, *out), "z is NULL")
        _einval(fn(None, xp, 2, 1, zp, 3, 0.0, None, bp, d(fm), d(rho), ip), "nei is NULL")
        _einval(fn(None, xp, 2, 1, zp, 3, -1e-9, *out), "jitter must be finite and >= 0")
        _einval(fn(None, xp, 2, 1, zp, 3, math.nan, *out), "jitter must be finite and >= 0")
        _einval(fn(None, xp, 2, 1, zp, 3, math.inf, *out), "jitter must be finite and >= 0")
    # a refused call writes nothing
    assert best.value == 7 and info.value == 7
    assert (nei == 7.0).all() and (fm == 7.0).all() and (rho == 7.0).all()
    assert lib.hbegp_debug_nei_phases(0, None) == _lib.OK
    # (the element type and a non-finite coordinate need a model: tests/test_gpu_nei.py)


def _kernel_notes(isa):
    """name -> {key: int} from the amdhsa metadata (one YAML block per kernel)."""
    out = {}
    meta = isa[isa.index("amdhsa.kernels:"):]
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+_count|private_segment_fixed_size):\s+(\d+)", block)}
    return out


def test_nei_kernels_do_not_spill():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", ROOT, "build/kernels.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "build", "kernels.s")) as f:
        notes = _kernel_notes(f.read())
    for stem, count in (("nei_pad_kernel", 2), ("nei_fmin_kernel", 2), ("nei_rho_kernel", 2), ("nei_kernel", 2), ("nei_best_kernel", 1)):
        found = [k for k in notes if stem in k]
        assert len(found) == count, (stem, found)  # f64 and f32; the epilogue has no element type
        for sym in found:
            assert notes[sym]["vgpr_spill_count"] == 0 and notes[sym]["sgpr_spill_count"] == 0, (sym, notes[sym])
            assert notes[sym]["private_segment_fixed_size"] == 0, (sym, notes[sym])


def test_ei_over_arrays_is_the_estimators_expected_improvement():
    rng = np.random.default_rng(1)
    mean, fmin = rng.standard_normal(200), rng.standard_normal(200)
    std = np.abs(rng.standard_normal(200)) * rng.choice([0.0, 1e-17, 1e-3, 1.0], 200)
    got = NEI.ei(mean, std, fmin)
    for i in range(200):
        ref = E.expected_improvement(float(mean[i]), float(std[i]), float(fmin[i]))
        assert abs(got[i] - ref) <= 4 * np.finfo(float).eps * max(1.0, abs(ref)), (i, got[i], ref)


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    return X, y


def _posterior(X, y, amp, noise, ell, nu, Xs):
    res = O.lml_with_gradient(X, y, noise, amp, ell, nu)
    mean, _, _ = O.predict(Xs, X, res["alpha"], res["k_inv"], amp, ell, nu)
    return np.asarray(mean, np.float64), PC.sigma_ref(Xs, X, amp, ell, nu, noise)


def test_restatement_is_the_expected_improvement_over_joint_draws():
    """nei_ref against plain Monte Carlo of E[max(0, min_i f(b_i) - f(x_j))] over 20 000 joint draws of all 52 rows, the
    restatement fed the same draws' baseline normals (the leading block of the joint factor is L_b).  Bar: 5 standard errors of
    the plain estimator + 1e-5."""
    n, d, amp, noise, nu = 300, 4, 1.3, 0.013, 2.5
    ell = np.linspace(0.3, 0.9, d)
    X, y = _data(n, d, 21)
    res = O.lml_with_gradient(X, y, noise, amp, ell, nu)
    mean_train, _, _ = O.predict(X, X, res["alpha"], res["k_inv"], amp, ell, nu)
    base = X[np.argsort(np.asarray(mean_train), kind="stable")[:40]]
    cand = base[:12] + 0.05 * np.random.default_rng(22).standard_normal((12, d))
    mu, S = _posterior(X, y, amp, noise, ell, nu, np.vstack([base, cand]))
    zj = np.random.default_rng(23).standard_normal((20000, 52))
    f = mu[None, :] + zj @ np.linalg.cholesky(S).T
    imp = np.maximum(0.0, f[:, :40].min(axis=1)[:, None] - f[:, 40:])
    plain, se = imp.mean(axis=0), imp.std(axis=0, ddof=1) / math.sqrt(len(zj))
    nei, rho, fmin_s = NEI.nei(mu, S, 40, zj[:, :40])
    assert np.abs(fmin_s - f[:, :40].min(axis=1)).max() <= 1e-12
    ratio = np.abs(plain - nei) / (5.0 * se + 1e-5)
    print(f"nei_ref against 20000 joint draws: worst ratio {ratio.max():.2f}, {int((nei > 1e-3).sum())} of 12 above 1e-3")
    assert (ratio <= 1.0).all(), ratio
    assert (nei > 1e-3).sum() >= 4, nei  # not vacuous


def test_restatement_properties():
    n, d, amp, noise, nu = 60, 3, 1.7, 0.02, 1.5
    ell = np.array([0.3, 0.5, 0.8])
    X, y = _data(n, d, 4)
    rng = np.random.default_rng(5)
    base = X[:25]
    cand = rng.uniform(-0.1, 1.1, (9, d))
    cand = np.vstack([cand, cand[:4], X[:2]])  # duplicates, and rows on the baseline
    mu, S = _posterior(X, y, amp, noise, ell, nu, np.vstack([base, cand]))
    mb, mc = 25, len(cand)
    # z = 0: exactly EI(mu_j, sqrt(rho_j), min mu_b)
    nei0, rho, fmin0 = NEI.nei(mu, S, mb, np.zeros((1, mb)))
    assert (fmin0 == mu[:mb].min()).all()
    assert np.array_equal(nei0, NEI.ei(mu[mb:], np.sqrt(rho), mu[:mb].min()))
    for j in range(mc):  # and that is the estimator's function, to the rounding of erfc
        ref = E.expected_improvement(float(mu[mb + j]), math.sqrt(rho[j]), float(mu[:mb].min()))
        assert abs(nei0[j] - ref) <= 4 * np.finfo(float).eps * max(1.0, abs(ref)), (j, nei0[j], ref)
    # rho is the conditional variance by a solve
    cond = np.diag(S)[mb:] - np.einsum("jb,bj->j", S[mb:, :mb], np.linalg.solve(S[:mb, :mb], S[:mb, mb:]))
    assert np.abs(rho - np.maximum(cond, 0.0)).max() <= 1e-10 * amp
    assert (rho[-2:] <= 2e-5).all()  # a candidate on a baseline row is known up to predict's 1e-5
    # duplicate candidates get equal values; best is the last index of the maximum
    z = rng.standard_normal((64, mb))
    nei, rho, fmin_s = NEI.nei(mu, S, mb, z)
    assert (nei >= 0).all() and np.isfinite(nei).all() and nei.max() > 0
    assert np.abs(nei[:4] - nei[9:13]).max() <= 1e-14 and np.abs(rho[:4] - rho[9:13]).max() <= 1e-14
    assert NEI.argmax_last([0.0, 2.0, 1.0, 2.0, 0.5]) == 3 and NEI.argmax_last([1.0]) == 0
    # mc = 0: the draws' minima only
    nei_e, rho_e, fm_e = NEI.nei(mu[:mb], S[:mb, :mb], mb, z)
    assert nei_e.shape == (0,) and rho_e.shape == (0,) and np.array_equal(fm_e, fmin_s)


class _FakeFitted:
    """A stand-in for gpr.FittedKernel on a fixed (mean, Sigma): rows are looked up by the index in their first feature;
    noisy_ei through the restatement, extend_with by conditioning on the appended row (kg_ref.sigma_tilde)."""

    released = 0

    def __init__(self, mean, sigma, s2, x_train, y_train):
        self.mean, self.sigma, self.s2 = mean, sigma, s2
        self.x_train, self.y_train = x_train, y_train
        self.lml = 0.0
        self.calls = []

    def predict(self, x, want_variance=True):
        rows = np.asarray(x)[:, 0].astype(int)
        return self.mean[rows], (np.maximum(np.diag(self.sigma)[rows], 0.0) if want_variance else None), 0

    def noisy_ei(self, baseline, candidates, z, jitter=0.0, want_details=False):
        b = np.asarray(baseline)[:, 0].astype(int)
        c = np.asarray(candidates).reshape(-1, 1)[:, 0].astype(int)
        self.calls.append((b, c, np.array(z)))
        rows = np.concatenate([b, c])
        S = self.sigma[np.ix_(rows, rows)] + jitter * np.eye(len(rows))
        nei, rho, fm = NEI.nei(self.mean[rows], S, len(b), z)
        best = NEI.argmax_last(nei) if len(c) else -1
        return (nei, best, fm, rho) if want_details else (nei, best)

    def extend_with(self, x, y, ctx=None):
        assert np.array_equal(x[:-1], self.x_train) and np.array_equal(y[:-1], self.y_train)
        j = int(x[-1, 0])
        st, sd = KG.sigma_tilde(self.sigma, j, self.s2)
        mean = self.mean + st * (y[-1] - self.mean[j]) / sd
        return _FakeFitted(mean, self.sigma - np.outer(st, st), self.s2, x, y)

    def release(self):
        _FakeFitted.released += 1


class _CountingRng:
    def __init__(self, seed):
        self.rng, self.shapes = np.random.default_rng(seed), []

    def standard_normal(self, shape):
        self.shapes.append(tuple(shape))
        return self.rng.standard_normal(shape)


@pytest.mark.parametrize("projection", ["linear", "logarithmic"])
def test_estimator_methods_on_a_stand_in(projection):
    n, d, amp, noise, nu = 40, 3, 1.7, 1e-2, 2.5
    ell = np.array([0.3, 0.5, 0.8])
    X, y = _data(n, d, 5)
    Xs = np.vstack([X[:20], np.random.default_rng(6).uniform(-0.1, 1.1, (30, d))])  # rows 0..19: "training rows", 20..49: candidates
    mean, S = _posterior(X, y, amp, noise, ell, nu, Xs)
    _, yn = E.YNormalize.new_project_into_normalized(np.exp(y) + 3.0, projection)
    train = np.arange(20, dtype=float)[:, None]
    fake = _FakeFitted(mean, S, noise, train, mean[:20].copy())
    model = E.SurrogateModelGPR(fake, (1e-5, 1e5), (1e-3, 1e3), [(1e-3, 1e3)] * 3, yn, np.float64)
    cand = np.arange(20, 50, dtype=float)[:, None]
    # the default baseline: the training rows; z from the rng; normalised units (no projection)
    nei, best = model.noisy_ei_a(cand, 64, np.random.default_rng(7))
    z = np.random.default_rng(7).standard_normal((64, 20))
    ref, _, _ = NEI.nei(mean, S, 20, z)
    assert np.array_equal(fake.calls[-1][0], np.arange(20)) and np.array_equal(fake.calls[-1][2], z)
    assert np.array_equal(nei, ref) and best == NEI.argmax_last(ref) and (nei >= 0).all() and nei.max() > 0
    # an explicit baseline
    model.noisy_ei_a(cand, 8, np.random.default_rng(7), baseline=np.array([[3.0], [1.0]]))
    assert fake.calls[-1][0].tolist() == [3, 1] and fake.calls[-1][2].shape == (8, 2)
    # max_baseline: the rows of lowest posterior mean, in their order, without random numbers
    keep = np.sort(np.argsort(mean[:20], kind="stable")[:7])
    nei7, best7 = model.noisy_ei_a(cand, 64, np.random.default_rng(8), max_baseline=7, jitter=1e-6)
    assert np.array_equal(fake.calls[-1][0], keep)
    rows = np.concatenate([keep, np.arange(20, 50)])
    ref7, _, _ = NEI.nei(mean[rows], S[np.ix_(rows, rows)] + 1e-6 * np.eye(37), 7, np.random.default_rng(8).standard_normal((64, 7)))
    assert np.array_equal(nei7, ref7) and best7 == NEI.argmax_last(ref7)
    model.noisy_ei_a(cand, 4, np.random.default_rng(8), max_baseline=50)  # more than there are: all of them
    assert np.array_equal(fake.calls[-1][0], np.arange(20))
    # k = 1 is best
    idx, means, neis = E.acquire_by_noisy_ei(cand, model, 1, np.random.default_rng(7), n_samples=64)
    assert idx.dtype == np.int64 and idx.tolist() == [best] and neis[0] == ref[best]
    assert means[0] == yn.project_location_from_normalized(mean[20 + best:21 + best])[0]
    # k > 1: distinct rows; the pick joins the baseline, whose growth makes the normals be drawn again
    _FakeFitted.released = 0
    rng = _CountingRng(9)
    idx, means, neis = E.acquire_by_noisy_ei(cand, model, 4, rng, n_samples=32)
    assert len(set(idx.tolist())) == 4 and (neis >= 0).all() and np.isfinite(means).all()
    assert _FakeFitted.released == 3  # every fantasy model, never the caller's
    assert rng.shapes == [(32, 20), (32, 21), (32, 22), (32, 23)]
    # the second pick is the best of the model conditioned on the first fantasy, with the first pick in the baseline
    z0 = np.random.default_rng(9).standard_normal((32, 20))
    r0, _, _ = NEI.nei(mean, S, 20, z0)
    assert idx[0] == NEI.argmax_last(r0) and neis[0] == r0[idx[0]]
    cond = fake.extend_with(np.vstack([train, [[20.0 + idx[0]]]]), np.concatenate([fake.y_train, mean[20 + idx[0]:21 + idx[0]]]))
    rest = [i for i in range(30) if i != idx[0]]
    rows = np.concatenate([np.arange(20), [20 + idx[0]], 20 + np.array(rest)])
    rng2 = np.random.default_rng(9)
    rng2.standard_normal((32, 20))
    r1, _, _ = NEI.nei(cond.mean[rows], cond.sigma[np.ix_(rows, rows)], 21, rng2.standard_normal((32, 21)))
    assert idx[1] == rest[NEI.argmax_last(r1)] and neis[1] == r1[NEI.argmax_last(r1)]
    # with max_baseline the baseline keeps its size and the same normals serve every pick
    rng = _CountingRng(10)
    idx, _, _ = E.acquire_by_noisy_ei(cand, model, 3, rng, n_samples=16, max_baseline=10)
    assert len(set(idx.tolist())) == 3 and rng.shapes == [(16, 10)]
    for bad in (dict(k=31), dict(k=-1)):
        with pytest.raises(ValueError):
            E.acquire_by_noisy_ei(cand, model, rng=np.random.default_rng(0), **bad)
    with pytest.raises(ValueError):
        E.acquire_by_noisy_ei(cand[:, 0], model, 2, np.random.default_rng(0))
