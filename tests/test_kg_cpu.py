"""CPU checks of the knowledge gradient over a candidate set (hbegp_knowledge_gradient_*): the symbols and their signatures against
the header, argument checks that refuse before any device call, register use of the new kernels, the NumPy restatement
(tests/kg_ref.py) against quadrature of its definition, the meaning of sigma-tilde against the oracle's closed-form predict on
the training set augmented with one noisy sample, and the estimator's methods on a model stand-in."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kg_ref as KG
import posterior_cov_ref as PC
from hbetune_rs_amd import _lib
from hbetune_rs_amd import estimator as E
from oracle import gpr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ("hbegp_knowledge_gradient_f64", "hbegp_knowledge_gradient_f32", "hbegp_debug_kg_phases")
NUS = [0.5, 1.5, 2.5, math.inf]


def test_kg_symbols_are_exported_with_the_headers_argument_counts():
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


def _kernel_notes(isa):
    """name -> {key: int} from the amdhsa metadata (one YAML block per kernel)."""
    out = {}
    meta = isa[isa.index("amdhsa.kernels:"):]
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+_count|private_segment_fixed_size):\s+(\d+)", block)}
    return out


def test_kg_kernels_do_not_spill():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", ROOT, "build/kernels.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "build", "kernels.s")) as f:
        notes = _kernel_notes(f.read())
    found = [k for k in notes if "kg_kernel" in k]
    assert len(found) == 2, found  # f64 and f32
    others = [k for k in notes if "kg_global_kernel" in k or "kg_epilogue_kernel" in k]
    assert len(others) == 4, others
    for sym in found + others:
        assert notes[sym]["vgpr_spill_count"] == 0 and notes[sym]["sgpr_spill_count"] == 0, (sym, notes[sym])
        assert notes[sym]["private_segment_fixed_size"] == 0, (sym, notes[sym])
    for sym in found:
        # 256 threads = one wave per SIMD per workgroup; the LDS lets 160 KiB / (16 P + 2 KiB) workgroups share a CU, and
        # 128 registers keep 4 waves per SIMD resident, which covers every P >= 2048
        assert notes[sym]["vgpr_count"] <= 128, (sym, notes[sym])


def _einval(rc, what):
    assert rc == _lib.EINVAL
    assert what in _lib.last_error(), _lib.last_error()


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    d, f = _lib.dptr, _lib.fptr
    x, out = np.zeros(8), np.zeros(8)
    xf, outf = np.zeros(8, np.float32), np.zeros(8, np.float32)
    kg = np.zeros(4)
    best, imin = C.c_int(7), C.c_int(7)
    bp, ip = C.byref(best), C.byref(imin)
    for fn, xp, op in ((lib.hbegp_knowledge_gradient_f64, d(x), d(out)), (lib.hbegp_knowledge_gradient_f32, f(xf), f(outf))):
        _einval(fn(None, xp, 2, 1, d(kg), bp, ip, op, op), "NULL model")
        _einval(fn(None, xp, 2, 2, d(kg), None, None, None, None), "NULL model")
        _einval(fn(None, xp, 2, 0, None, None, None, None, None), "NULL model")  # mc = 0 with a NULL kg passes the checks before it
        _einval(fn(None, xp, -1, 0, d(kg), bp, ip, op, op), "m must be >= 0")
        _einval(fn(None, xp, 2, -1, d(kg), bp, ip, op, op), "mc must be >= 0")
        _einval(fn(None, xp, 2, 3, d(kg), bp, ip, op, op), "mc must be <= m")
        _einval(fn(None, xp, 0, 1, d(kg), bp, ip, op, op), "mc must be <= m")
        _einval(fn(None, xp, 2, 1, None, bp, ip, op, op), "kg is NULL")
    assert best.value == 7 and imin.value == 7  # a refused call writes nothing
    assert lib.hbegp_debug_kg_phases(0, None) == _lib.OK
    # (the element type and a non-finite query coordinate need a model: tests/test_gpu_kg.py)


def _random_lines(rng, m, kind):
    a = rng.standard_normal(m)
    b = rng.standard_normal(m) * rng.choice([0.05, 0.5, 2.0])
    if kind == "tied slopes" and m > 1:
        b = np.round(b, 1)
    if kind == "tied pairs" and m > 1:
        src = rng.integers(0, m, m // 2)
        a[: m // 2], b[: m // 2] = a[src], b[src]
    if kind == "flat":
        b[:] = b[0]
    return a, b


def test_restatement_is_the_definition_by_quadrature():
    rng = np.random.default_rng(0)
    cases = [(1, "plain")]
    for kind in ("plain", "tied slopes", "tied pairs", "flat"):
        cases += [(int(m), kind) for m in rng.integers(2, 61, 12)]
    worst = 0.0
    for m, kind in cases:
        a, b = _random_lines(rng, m, kind)
        got = KG.h(a, b)  # E[max (a + b Z)] - max a = min mu - E[min (mu + st Z)] with mu = -a, st = -b
        assert got >= 0.0
        step = 1.0 / 1024
        q = [float(np.min(-a)) - KG.expected_min_quadrature(-a, -b, s) for s in (step, step / 2, step / 4)]
        # the trapezoid rule's error at the kinks of min_i(.) falls by 4 per halving, so the finest value is within a third of the
        # last change when the kinks sit alike on both grids; four times the larger of the two changes covers the case where they
        # do not, and the sum of 24 / (step / 4) terms of size <= max|a| + 12 max|b| carries its own rounding
        tol = 4.0 * max(abs(q[0] - q[1]), abs(q[1] - q[2])) + (96 / step) * np.finfo(float).eps * (np.abs(a).max() + 12 * np.abs(b).max())
        assert abs(got - q[2]) <= tol, (m, kind, got, q, tol)
        worst = max(worst, abs(got - q[2]))
        if m == 1 or kind == "flat":
            assert got == 0.0, (m, kind, got)
    print(f"restatement against quadrature: worst deviation {worst:.1e} over {len(cases)} cases")


def test_single_surviving_line_gives_exactly_zero():
    assert KG.h([0.3], [1.7]) == 0.0
    assert KG.h([0.3, 0.1, 0.2], [0.5, 0.5, 0.5]) == 0.0  # all slopes equal: the largest a survives
    assert KG.h([0.3, 0.3], [-0.0, 0.0]) == 0.0  # the two zeros are one slope
    ea, eb = KG.envelope([0.0, 5.0, 0.0], [-1.0, 0.0, 1.0])
    assert len(ea) == 3
    ea, eb = KG.envelope([0.0, -5.0, 0.0], [-1.0, 0.0, 1.0])  # the middle line lies below the crossing of the outer two
    assert list(eb) == [-1.0, 1.0]
    # r = 0 off the diagonal and no latent variance: d_j = s2 and every slope is 0
    S = np.eye(4) * KG.MIN_NOISE
    assert np.array_equal(KG.kg(np.array([0.1, -0.4, 0.0, 2.0]), S, 0.3), np.zeros(4))


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


@pytest.mark.parametrize("nu", NUS)
def test_sigma_tilde_is_the_mean_after_one_noisy_sample(nu):
    X, y, amp, noise, ell, Xs = _problem(seed=int(nu) if math.isfinite(nu) else 7)
    mean, S = _posterior(X, y, amp, noise, ell, nu, Xs)
    for j in (0, 11, 29):
        st, sd = KG.sigma_tilde(S, j, noise)
        for z in (-2.0, -0.5, 0.0, 1.0, 3.0):
            Xa = np.vstack([X, Xs[j:j + 1]])
            ya = np.concatenate([y, [mean[j] + sd * z]])
            res = O.lml_with_gradient(Xa, ya, noise, amp, ell, nu)
            om, _, _ = O.predict(Xs, Xa, res["alpha"], res["k_inv"], amp, ell, nu)
            dm = float(np.abs(mean + st * z - om).max())
            assert dm <= 1e-10 * amp, (j, z, dm)  # tests/test_batch_select_cpu.py's bar for the same augmented-set comparison


@pytest.mark.parametrize("nu", NUS)
def test_kg_is_nonnegative_and_does_not_depend_on_mc(nu):
    X, y, amp, noise, ell, Xs = _problem(m=50, seed=3)
    Xs[40:] = Xs[:10]  # duplicate rows
    Xs[30:35] = X[:5]  # rows on training points
    mean, S = _posterior(X, y, amp, noise, ell, nu, Xs)
    full = KG.kg(mean, S, noise)
    assert (full >= 0.0).all() and np.isfinite(full).all() and full.max() > 0.0
    assert np.array_equal(KG.kg(mean, S, noise, mc=7), full[:7])
    assert KG.kg(mean[:1], S[:1, :1], noise)[0] == 0.0  # m = 1


class _FakeFitted:
    """A stand-in for gpr.FittedKernel on a fixed (mean, Sigma): rows are looked up by the index in their first feature;
    knowledge_gradient through the restatement, extend_with by conditioning on the appended row."""

    released = 0

    def __init__(self, mean, sigma, s2, x_train, y_train):
        self.mean, self.sigma, self.s2 = mean, sigma, s2
        self.x_train, self.y_train = x_train, y_train
        self.lml = 0.0
        self.calls = []

    def knowledge_gradient(self, x, n_candidates=None, want_posterior=False):
        rows = np.asarray(x)[:, 0].astype(int)
        mc = len(rows) if n_candidates is None else n_candidates
        self.calls.append((rows, mc))
        mu, S = self.mean[rows], self.sigma[np.ix_(rows, rows)]
        kg = KG.kg(mu, S, self.s2, mc=mc)
        out = (kg, KG.argmax_last(kg) if mc else -1, int(np.argmin(mu)))
        return out + (mu, np.maximum(np.diag(S), 0.0)) if want_posterior else out

    def extend_with(self, x, y, ctx=None):
        assert np.array_equal(x[:-1], self.x_train) and np.array_equal(y[:-1], self.y_train)
        j = int(x[-1, 0])
        st, sd = KG.sigma_tilde(self.sigma, j, self.s2)
        mean = self.mean + st * (y[-1] - self.mean[j]) / sd
        return _FakeFitted(mean, self.sigma - np.outer(st, st), self.s2, x, y)

    def release(self):
        _FakeFitted.released += 1


@pytest.mark.parametrize("projection", ["linear", "logarithmic"])
def test_estimator_methods_on_a_stand_in(projection):
    X, y, amp, noise, ell, Xs = _problem(m=30, seed=5)
    mean, S = _posterior(X, y, amp, noise, ell, 2.5, Xs)
    _, yn = E.YNormalize.new_project_into_normalized(np.exp(y) + 3.0, projection)
    fake = _FakeFitted(mean, S, noise, np.zeros((0, 1)), np.zeros(0))
    model = E.SurrogateModelGPR(fake, (1e-5, 1e5), (1e-3, 1e3), [(1e-3, 1e3)] * 3, yn, np.float64)
    rows = np.arange(30, dtype=float)[:, None]
    ref = KG.kg(mean, S, noise)
    kg, best = model.knowledge_gradient_a(rows)
    assert np.array_equal(kg, ref) and best == KG.argmax_last(ref)  # normalised units: no projection
    kg12, best12 = model.knowledge_gradient_a(rows, n_candidates=12)
    assert np.array_equal(kg12, ref[:12]) and best12 == KG.argmax_last(ref[:12])
    imin, m_imin = model.best_by_mean_a(rows)
    assert imin == int(np.argmin(mean)) and fake.calls[-1][1] == 0
    assert m_imin == yn.project_location_from_normalized(mean[imin:imin + 1])[0]
    # k = 1 is best; k picks are distinct and stay among the places to sample
    idx, means, kgs = E.acquire_by_knowledge_gradient(rows, model, 1)
    assert idx.dtype == np.int64 and idx.tolist() == [best] and kgs[0] == ref[best]
    assert means[0] == yn.project_location_from_normalized(mean[best:best + 1])[0]
    _FakeFitted.released = 0
    idx, means, kgs = E.acquire_by_knowledge_gradient(rows, model, 6, n_candidates=12)
    assert len(set(idx.tolist())) == 6 and idx.max() < 12 and idx[0] == best12
    assert _FakeFitted.released == 5  # every fantasy model, never the caller's
    # the second pick is the best of the model conditioned on the first fantasy, the first pick no longer a place to sample
    cond = fake.extend_with(np.array([[float(idx[0])]]), mean[idx[0]:idx[0] + 1])
    order = [i for i in range(12) if i != idx[0]] + [int(idx[0])] + list(range(12, 30))
    kg2, b2, _ = cond.knowledge_gradient(rows[order], n_candidates=11)
    assert idx[1] == order[b2] and kgs[1] == kg2[b2]
    assert (kgs >= 0).all()
    for bad in (dict(k=13, n_candidates=12), dict(k=-1), dict(k=1, n_candidates=31)):
        with pytest.raises(ValueError):
            E.acquire_by_knowledge_gradient(rows, model, **bad)
    with pytest.raises(ValueError):
        E.acquire_by_knowledge_gradient(rows[:, 0], model, 2)
