"""CPU: posterior sample paths -- the NumPy restatement against itself (tests/paths_ref.py), gpr.draw_spectral, the ABI of
hbegp_paths_* (symbols, signatures, the argument checks that need no device) and the new kernels' register metadata."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import paths_ref as PR
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUS = [0.5, 1.5, 2.5, math.inf]


def _problem(nu, n=60, d=3, F=512, S=3, seed=0, noise_draw=True):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    amp, ell, noise = 1.3, np.linspace(0.3, 0.9, d), 1.3e-2
    om0, ph = gpr.draw_spectral(nu, F, d, E.RNG(seed + 11))
    w = rng.standard_normal((S, F))
    eps = rng.standard_normal((S, n)) if noise_draw else None
    return X, y, amp, ell, noise, om0, ph, w, eps


@pytest.mark.parametrize("nu", NUS)
def test_antithetic_pair_is_the_posterior_mean(nu):
    """f is linear in (w, eps): the mean of a path and its mirror image is k* alpha exactly, whatever the feature error."""
    X, y, amp, ell, noise, om0, ph, w, eps = _problem(nu, n=300, d=4, F=4096, S=4)
    xs = np.random.default_rng(5).uniform(-0.1, 1.1, (50, 4))
    a = PR.Paths(X, y, amp, ell, nu, noise, om0, ph, w, eps)
    b = PR.Paths(X, y, amp, ell, nu, noise, om0, ph, -w, -eps)
    mu = a.mean(xs)
    dev = np.abs(0.5 * (a.evaluate(xs, False)[0] + b.evaluate(xs, False)[0]) - mu[None, :]).max() / max(1.0, np.abs(mu).max())
    print(f"nu={nu}: antithetic deviation {dev:.2e}")
    assert dev <= 1e-12


@pytest.mark.parametrize("nu", NUS)
def test_gradient_is_the_central_difference_of_the_value(nu):
    X, y, amp, ell, noise, om0, ph, w, eps = _problem(nu, F=256)
    p = PR.Paths(X, y, amp, ell, nu, noise, om0, ph, w, eps)
    xs = np.random.default_rng(3).uniform(-0.1, 1.1, (7, 3))
    _, df = p.evaluate(xs)
    # per-path points take the same road
    f3, df3 = p.evaluate(np.broadcast_to(xs, (3,) + xs.shape))
    assert np.allclose(df3, df, rtol=0, atol=1e-10) and np.allclose(f3, p.evaluate(xs)[0], rtol=0, atol=1e-12)  # (BLAS shapes differ)
    h = 1e-6
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        num = (p.evaluate(xs + e, False)[0] - p.evaluate(xs - e, False)[0]) / (2 * h)
        scale = max(1.0, np.abs(df).max())
        # truncation h^2 f''' / 6 and rounding eps |f| / h of a central difference; nu = 1/2 has a kink only AT a training point
        assert np.abs(num - df[:, :, k]).max() <= 1e-5 * scale, (nu, k, np.abs(num - df[:, :, k]).max())


@pytest.mark.parametrize("noise_draw", [True, False])
@pytest.mark.parametrize("nu", NUS)
def test_closed_form_covariance_is_the_empirical_one(nu, noise_draw):
    """N paths that share (omega, b): every entry of the empirical covariance within 6 standard errors of the closed form, the
    standard error of a Gaussian sample covariance taken from the closed form itself, sqrt((S_ii S_jj + S_ij^2) / (N - 1))."""
    N = 4000
    X, y, amp, ell, noise, om0, ph, w, eps = _problem(nu, n=40, d=3, F=128, S=N, seed=7, noise_draw=noise_draw)
    p = PR.Paths(X, y, amp, ell, nu, noise, om0, ph, w, eps)
    xs = np.random.default_rng(9).uniform(-0.1, 1.1, (12, 3))
    cov = p.covariance(xs) if noise_draw else None
    if not noise_draw:  # without the noise draw the noise I term of the closed form is absent
        Ps, PX = p.features(xs), p.features(p.X)
        Am = np.linalg.solve(p.K, p.kstar(xs).T).T
        cov = Ps @ Ps.T - Am @ (PX @ Ps.T) - (Ps @ PX.T) @ Am.T + Am @ (PX @ PX.T) @ Am.T
    f = p.evaluate(xs, False)[0]
    emp = np.cov(f.T)
    se = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov**2) / (N - 1))
    worst = (np.abs(emp - cov) / se).max()
    print(f"nu={nu} noise_draw={noise_draw}: worst deviation {worst:.2f} standard errors")
    assert worst <= 6.0
    # ... and the empirical mean is the posterior mean (the features' mean is zero)
    sem = np.sqrt(np.diag(cov) / N)
    assert (np.abs(f.mean(axis=0) - p.mean(xs)) / sem).max() <= 6.0


@pytest.mark.parametrize("nu", NUS)
def test_draw_spectral_approaches_the_kernel(nu):
    """Phi(X) Phi(X)^T -> k(X, X) as F grows: the error at 16 F is below the error at F (no fixed size is asserted)."""
    rng = np.random.default_rng(2)
    X = rng.uniform(0, 1, (80, 4))
    ell, c = np.linspace(0.3, 0.9, 4), 1.3
    K = c * PR.matern(PR.scaled_dist(X, X, ell), nu)
    errs = []
    for F in (256, 4096):
        om0, ph = gpr.draw_spectral(nu, F, 4, E.RNG(17))
        assert om0.shape == (F, 4) and ph.shape == (F,) and (ph >= 0).all() and (ph < 2 * math.pi).all()
        P = math.sqrt(2 * c / F) * np.cos(X @ (om0 / ell).T + ph)
        errs.append(float(np.abs(P @ P.T - K).max()))
    print(f"nu={nu}: max |Phi Phi^T - K| = {errs[0]:.4f} at F = 256, {errs[1]:.4f} at F = 4096")
    assert errs[1] < errs[0]
    a, _ = gpr.draw_spectral(nu, 8, 2, E.RNG(3))
    b, _ = gpr.draw_spectral(nu, 8, 2, E.RNG(3))
    assert np.array_equal(a, b)


def test_draw_spectral_refuses_other_orders():
    with pytest.raises(ValueError):
        gpr.draw_spectral(1.0, 8, 2, E.RNG(1))


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_paths_symbols_are_exported_with_signatures():
    lib = _lib.load()
    names = ["hbegp_paths_create_f64", "hbegp_paths_create_f32", "hbegp_paths_eval_f64", "hbegp_paths_eval_f32",
             "hbegp_paths_minimize_f64", "hbegp_paths_minimize_f32", "hbegp_paths_info", "hbegp_paths_release", "hbegp_debug_paths_phases"]
    with open(os.path.join(ROOT, "include", "hbegp.h")) as f:
        header = f.read()
    for name in names:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        decl = re.search(r"\b(?:int|void)\s+" + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
    assert f"#define HBEGP_PATHS_MAX_FEATURES {_lib.PATHS_MAX_FEATURES}" in header
    assert f"#define HBEGP_PATHS_MAX_PATHS {_lib.PATHS_MAX_PATHS}" in header


def _einval(rc, what):
    assert rc == _lib.EINVAL
    assert what in _lib.last_error(), _lib.last_error()


def test_bad_arguments_are_refused_before_any_device_call():
    import ctypes as C

    lib = _lib.load()
    d, f = _lib.dptr, _lib.fptr
    a, af = np.zeros(16), np.zeros(16, np.float32)
    h = C.c_void_p()
    hp = C.byref(h)
    for fn, p, arr in ((lib.hbegp_paths_create_f64, d, a), (lib.hbegp_paths_create_f32, f, af)):
        _einval(fn(None, p(arr), p(arr), p(arr), None, 0, 1, hp), "F must be in")
        _einval(fn(None, p(arr), p(arr), p(arr), None, _lib.PATHS_MAX_FEATURES + 1, 1, hp), "F must be in")
        _einval(fn(None, p(arr), p(arr), p(arr), None, 4, 0, hp), "S must be in")
        _einval(fn(None, p(arr), p(arr), p(arr), None, 4, _lib.PATHS_MAX_PATHS + 1, hp), "S must be in")
        _einval(fn(None, p(arr), p(arr), p(arr), None, 4, 2, hp), "NULL model")
    for fn, p, arr in ((lib.hbegp_paths_eval_f64, d, a), (lib.hbegp_paths_eval_f32, f, af)):
        _einval(fn(None, p(arr), -1, 0, p(arr), None), "m must be >= 0")
        _einval(fn(None, p(arr), 2, 2, p(arr), None), "per_path must be 0 or 1")
        _einval(fn(None, p(arr), 2, 0, p(arr), None), "NULL paths handle")
    for fn, p, arr in ((lib.hbegp_paths_minimize_f64, d, a), (lib.hbegp_paths_minimize_f32, f, af)):
        _einval(fn(None, p(arr), 0, d(a), d(a), 10, p(arr), d(a), None), "R must be >= 1")
        _einval(fn(None, p(arr), 1, d(a), d(a), 0, p(arr), d(a), None), "maxeval must be >= 1")
        _einval(fn(None, p(arr), 1, d(a), d(a), 10, p(arr), d(a), None), "NULL paths handle")
    _einval(lib.hbegp_paths_info(None, None, None, None, None, None), "NULL paths handle")
    lib.hbegp_paths_release(None)  # a no-op
    assert lib.hbegp_debug_paths_phases(0, None) == _lib.OK
    # (NULL arrays, the other element type, lo > hi and starts outside the box need a model or a handle:
    # tests/test_gpu_paths.py::test_refusals_that_need_a_model_or_a_handle and ::test_minimiser_contract)


def test_cpp_wrapper_instantiates_for_both_element_types(tmp_path):
    """include/hbegp.hpp: PathsT<A> and FittedKernel<A>::sample_paths compile for double and float (host only, syntax check)."""
    import shutil

    src = tmp_path / "paths_hpp.cpp"
    src.write_text(
        '#include "hbegp.hpp"\n'
        "template class hbegp::PathsT<double>;\ntemplate class hbegp::PathsT<float>;\n"
        "template <typename A> void use(const hbegp::FittedKernel<A>& fk, const A* a, const double* b, A* o, double* f) {\n"
        "  hbegp::PathsT<A> p = fk.sample_paths(a, a, a, nullptr, 4, 2);\n"
        "  p.eval(a, 1, false, o, o);\n  p.eval(a, 1, true, o, nullptr);\n  p.minimize(a, 2, b, b, 10, o, f);\n"
        "  hbegp::PathsT<A> q(std::move(p));\n  p = std::move(q);\n}\n"
        "template void use<double>(const hbegp::FittedKernel<double>&, const double*, const double*, double*, double*);\n"
        "template void use<float>(const hbegp::FittedKernel<float>&, const float*, const double*, float*, double*);\n")
    cxx = shutil.which("g++") or shutil.which("c++") or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([cxx, "-std=c++17", "-x", "c++", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)])


# ------------------------------------------------------------------------------------------------------- kernel metadata
def _kernel_notes(isa):
    out = {}
    for block in isa.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+_count|private_segment_fixed_size):\s+(\d+)", block)}
    return out


def test_new_kernels_do_not_spill():
    subprocess.check_call(["make", "-C", ROOT, "build/kernels.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "build", "kernels.s")) as f:
        notes = _kernel_notes(f.read())
    mine = {k: v for k, v in notes.items() if re.search(r"paths_(project|project_finish|scale_omega|eval|eval_finish)_kernel", k)}
    # f64 and f32 of: scale_omega, project, project_finish, eval_finish, and eval<SB = 1 | PE_SB> x <data | features>
    assert len(mine) == 16, sorted(mine)
    for sym, n in mine.items():
        print(sym, n)
        assert n["vgpr_spill_count"] == 0 and n["sgpr_spill_count"] == 0, (sym, n)
        assert n["private_segment_fixed_size"] == 0, (sym, n)
