"""CPU: input warping without a GPU -- the library exports the new entry points, the host warp
(hbegp_warp_apply / _invert) agrees with 50-digit arithmetic, the NumPy restatement tests/warp_ref.py agrees with central
differences of its own lml in extended precision (the yardstick is checked before the device is judged by it), and the inputs of
tests/test_gpu_warp.py are such that a dropped feature chunk or a dead warp term cannot hide below the bars (the precedent of
tests/test_feature_counts_cpu.py)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import feature_count_cases as FC
import warp_cases as WC
import warp_ref as WR
from hbetune_rs_amd import _lib, gpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hbegp_warp_apply", "hbegp_warp_invert", "hbegp_problem_eval_xgrad", "hbegp_problem_eval_warped",
               "hbegp_fit_warped_f64", "hbegp_fit_warped_f32", "hbegp_model_warp", "hbegp_problem_debug_rows_f64",
               "hbegp_problem_debug_rows_f32"]
# what the C++ mirror wraps (it has no problem handle) and what the Rust binding declares
IN_HPP = ["hbegp_warp_apply", "hbegp_warp_invert", "hbegp_fit_warped_f64", "hbegp_fit_warped_f32", "hbegp_model_warp"]
IN_RUST = NEW_SYMBOLS[:7]


def test_library_exports_the_warp_entry_points():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hbegp.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        proto = re.search(name + r"\s*\(([^)]*)\)", text)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.hbegp_version() == 200
    for other, names in (("include/hbegp.hpp", IN_HPP), ("integration/gpr_gpu.rs", IN_RUST)):
        src = open(os.path.join(ROOT, other)).read()
        for name in names:
            assert name in src, (other, name)
    import ctypes as C
    assert C.sizeof(_lib.FitOptions) == 8 + 4 * 4 + 7 * 8  # the warped fit reads the options every fit reads: the struct keeps its size
    assert lib.hbegp_model_warp(None, None) == _lib.EINVAL


# ---- the host warp against mpmath ---------------------------------------------------------------------------------------------
GRID_X = [0.0, 2.0 ** -50, 1e-3, 0.5, 1.0 - 2.0 ** -50, 1.0]
GRID_AB = [0.2, 1.0, 5.0]


def _mp_warp(x, a, b):
    """u, du/dln a, du/dln b of one interior point at 50 digits, in forms that keep the digits of 1 - x^a near both ends."""
    import mpmath as mp

    X, A, B = mp.mpf(x), mp.mpf(a), mp.mpf(b)
    t = A * mp.log(X)
    L = mp.log(-mp.expm1(t)) if t > -1 else mp.log1p(-mp.exp(t))  # ln(1 - x^a)
    v = B * L
    return -mp.expm1(v), B * t * mp.exp((B - 1) * L + t), -v * mp.exp(v)


def test_host_warp_against_mpmath():
    import mpmath as mp

    mp.mp.dps = 50
    x = np.array(GRID_X)[:, None]
    worst = {}
    for a in GRID_AB:
        for b in GRID_AB:
            w = gpr.Warp([a, b])
            u, da, db = w.apply(x, want_param_gradients=True)
            back = w.invert(u)
            # the ends: exact values, exact zeros
            assert u[0, 0] == 0.0 and u[-1, 0] == 1.0 and back[0, 0] == 0.0 and back[-1, 0] == 1.0, (a, b)
            assert da[0, 0] == 0.0 and da[-1, 0] == 0.0 and db[0, 0] == 0.0 and db[-1, 0] == 0.0, (a, b)
            jac = w.jacobian(x)
            assert jac[0, 0] == (math.inf if a < 1 else (b if a == 1 else 0.0)), (a, b, jac[0, 0])
            assert jac[-1, 0] == (math.inf if b < 1 else (a if b == 1 else 0.0)), (a, b, jac[-1, 0])
            for i in range(1, len(GRID_X) - 1):
                ref = _mp_warp(GRID_X[i], a, b)
                for name, got, want in zip(("u", "du/dln a", "du/dln b"), (u[i, 0], da[i, 0], db[i, 0]), ref):
                    err = abs(mp.mpf(float(got)) - want)
                    rel = float(err / abs(want)) if want != 0 else float(err)
                    assert rel <= 1e-13 or float(err) <= 1e-300, (name, a, b, GRID_X[i], float(got), float(want), rel)
                    if rel > worst.get(name, (0.0,))[0]:
                        worst[name] = (rel, a, b, GRID_X[i])
                rt = abs(float(back[i, 0]) - GRID_X[i])
                assert rt <= 1e-12, ("round trip", a, b, GRID_X[i], float(back[i, 0]))
                if rt > worst.get("round trip", (0.0,))[0]:
                    worst["round trip"] = (rt, a, b, GRID_X[i])
    print("host warp vs mpmath, worst (deviation, a, b, x):", worst)


def test_host_warp_matches_the_restatement_and_its_shapes():
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 1, (4, 7, 3))
    ab = np.exp(rng.uniform(math.log(0.2), math.log(5.0), 6))
    w = gpr.Warp(ab)
    u, da, db = w.apply(x, want_param_gradients=True)
    ru, rda, rdb, rdx = WR.warp(x, ab)
    assert u.shape == x.shape
    for got, ref in ((u, ru), (da, rda), (db, rdb), (w.jacobian(x), rdx)):
        assert np.abs(got - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    assert np.abs(w.invert(u) - x).max() <= 1e-12 and np.abs(WR.unwarp(ru, ab) - x).max() <= 1e-12
    ident = gpr.Warp.identity(3)
    assert np.abs(ident.apply(x) - x).max() <= 2e-16 and np.abs(ident.jacobian(x) - 1).max() <= 1e-15


def test_host_warp_refuses_bad_input():
    lib = _lib.load()
    x = np.array([0.25, 0.5])
    out = np.full(2, 7.0)
    ok = np.array([1.0, 2.0, 1.0, 0.5])
    for bad_ab in ([0.0, 1, 1, 1], [1, -1.0, 1, 1], [1, 1, math.nan, 1], [1, 1, 1, math.inf]):
        ab = np.array(bad_ab, dtype=np.float64)
        assert lib.hbegp_warp_apply(_lib.dptr(ab), 2, _lib.dptr(x), 1, _lib.dptr(out), None, None, None) == _lib.EINVAL, bad_ab
        assert lib.hbegp_warp_invert(_lib.dptr(ab), 2, _lib.dptr(x), 1, _lib.dptr(out)) == _lib.EINVAL, bad_ab
    for bad_x in ([-1e-300, 0.5], [0.5, 1.0 + 2.0 ** -52], [math.nan, 0.5]):
        xb = np.array(bad_x)
        assert lib.hbegp_warp_apply(_lib.dptr(ok), 2, _lib.dptr(xb), 1, _lib.dptr(out), None, None, None) == _lib.EINVAL, bad_x
        assert lib.hbegp_warp_invert(_lib.dptr(ok), 2, _lib.dptr(xb), 1, _lib.dptr(out)) == _lib.EINVAL, bad_x
    assert lib.hbegp_warp_apply(None, 2, _lib.dptr(x), 1, _lib.dptr(out), None, None, None) == _lib.EINVAL
    assert lib.hbegp_warp_apply(_lib.dptr(ok), 0, _lib.dptr(x), 1, _lib.dptr(out), None, None, None) == _lib.EINVAL
    assert (out == 7.0).all()  # a refused call writes nothing
    assert lib.hbegp_warp_apply(_lib.dptr(ok), 2, _lib.dptr(x), 1, None, None, None, None) == _lib.OK  # every output may be NULL
    assert lib.hbegp_problem_eval_xgrad(None, 0, 0, None, None, None, None, None, None) == _lib.EINVAL
    assert lib.hbegp_problem_eval_warped(None, 0, 0, None, None, None, None, None, None) == _lib.EINVAL
    with pytest.raises(ValueError):
        gpr.Warp([1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        gpr.Warp([1.0, 0.0])


# ---- the restatement against central differences of its own lml -------------------------------------------------------------
FD_STEP = 1e-6
FD_BAR = 1e-6
FD_N, FD_D = 12, 3


def _fd_case(nu, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.05, 0.95, (FD_N, FD_D))
    if nu != 0.5:
        X[7] = X[2]  # a duplicate pair: r = 0 off the diagonal (at nu = 1/2 the kernel has a kink there, the convention is a choice)
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(FD_N)
    theta = np.log(np.concatenate([[0.05, 1.3], np.linspace(0.4, 0.9, FD_D)]))
    ab = np.exp(rng.uniform(math.log(0.4), math.log(2.5), 2 * FD_D))
    rv = rng.uniform(0, 0.05, FD_N) if seed % 2 else None
    return X, y, theta, ab, rv


@pytest.mark.parametrize("nu", [0.5, 1.5, 2.5, math.inf])
def test_restated_gradients_against_central_differences(nu):
    LD = np.longdouble
    h = LD(FD_STEP)
    X, y, theta, ab, rv = _fd_case(nu, 40 + int(min(nu, 9) * 2))
    noise, c, ell = WR.params_of(theta)
    ev = WR.evaluate(X, y, noise, c, ell, nu, rv)

    def lml_at(Xr):
        return WR.lml_ld(Xr, y, noise, c, ell, nu, rv)

    # G: every row and feature, moving a duplicate's two copies one at a time (the other keeps its place)
    fd = np.zeros_like(ev["G"])
    for i in range(FD_N):
        for k in range(FD_D):
            Xp, Xm = np.asarray(X, LD).copy(), np.asarray(X, LD).copy()
            Xp[i, k] += h
            Xm[i, k] -= h
            fd[i, k] = float((lml_at(Xp) - lml_at(Xm)) / (2 * h))
    dev_g = np.abs(ev["G"] - fd).max() / np.abs(fd).max()
    # the warped objective: p + 2 d log-space variables
    lml, grad, _ = WR.warped_objective(X, y, theta, ab, nu, rv=rv)
    v0 = np.concatenate([theta, np.log(ab)]).astype(LD)

    def warped_at(v):
        par = np.exp(v[:FD_D + 2])
        return WR.lml_ld(WR.warp_ld(X, np.exp(v[FD_D + 2:])), y, par[0], par[1], par[2:], nu, rv)

    assert abs(float(warped_at(v0)) - lml) <= 1e-10 * max(1.0, abs(lml))
    fdw = np.zeros_like(grad)
    for j in range(len(v0)):
        vp, vm = v0.copy(), v0.copy()
        vp[j] += h
        vm[j] -= h
        fdw[j] = float((warped_at(vp) - warped_at(vm)) / (2 * h))
    dev_w = np.abs(grad - fdw).max() / np.abs(fdw).max()
    print(f"nu={nu}: G vs central differences {dev_g:.2e}, warped gradient {dev_w:.2e} (bar {FD_BAR:g}; longdouble eps "
          f"{float(np.finfo(LD).eps):.1e})")
    assert np.abs(fd).max() > 0.1 and np.abs(fdw[FD_D + 2:]).min() > 0
    assert dev_g <= FD_BAR and dev_w <= FD_BAR, (dev_g, dev_w)


# ---- the inputs of the GPU module -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WC.CASES, ids=[c.id for c in WC.CASES])
def test_gpu_inputs_expose_every_chunk_and_every_warp_term(case):
    X, y, theta = WC.inputs(case)
    assert X.dtype == case.dtype and X.min() >= 0 and X.max() <= 1
    rv = WC.row_variance(case)
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    noise, c, ell = WR.params_of(theta)
    ev = WR.evaluate(X64, y64, noise, c, ell, case.nu, rv)
    f32 = case.dtype == np.float32
    cond_bar = case.n + 1 if f32 else 1e6
    assert np.linalg.cond(ev["K"]) <= cond_bar
    scale = max(1.0, float(np.abs(ev["G"]).max()))
    for sl in FC.groups(case.d, FC.GROUP_LOO):
        best = float(np.abs(ev["G"][:, sl]).max()) / scale
        assert best >= 100 * case.tol, f"{case.id}: columns {sl.start}:{sl.stop} of G reach {best:.2e} of its scale"
    ab = WC.warp_ab(case)
    assert ab.min() >= 0.4 and ab.max() <= 2.5
    lml, grad, evw = WR.warped_objective(X64, y64, theta, ab, case.nu, rv=rv)
    assert np.linalg.cond(evw["K"]) <= cond_bar
    gscale = max(1.0, float(np.abs(grad).max()))
    small = float(np.abs(grad[case.d + 2:]).min()) / gscale
    assert small > case.tol, f"{case.id}: a warp gradient entry is {small:.2e} of the gradient's scale"
    if case.kind == "dup":
        assert (X[100] == X[3]).all()
    # the warp moves the rows, and the lml by ten bars or more: a warp that was not applied cannot pass
    U = WR.warp(X64, ab)[0]
    assert np.abs(U - X64).max() > 0.05 and abs(lml - ev["lml"]) > 10 * case.tol * max(1.0, abs(lml))


# ---- the fit fixture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", WC.FIT_SIZES)
def test_fit_fixture_rewards_a_warp(n):
    """A condition on the inputs of the GPU module's fit tests: on the reference objective, from the plain optimum, the warp is
    worth more than 1 nat (seeds 96 / 200 of warp_cases.fit_data: 30.0 and 36.0 nats)."""
    X, y = WC.fit_data(n)
    assert X.min() >= 0 and X.max() <= 1 and abs(y.mean()) < 1e-12 and abs(y.std() - 1) < 1e-12
    r = WR.reference_fits(X, y, WC.FIT_THETA0, WC.FIT_LO, WC.FIT_HI, WC.FIT_NU)
    print(f"n={n}: reference lml plain {r['lml_plain']:.4f}, warped {r['lml_warped']:.4f}, gain {r['gain']:.4f} nats; "
          f"a, b = {np.exp(r['v_warped'][4:])}")
    assert r["gain"] > 1.0
    if n == 96:  # the f32 fit's box (warp_cases.fit_box): the same condition, and a kernel matrix f32 can factor to the bar
        lo, hi = WC.fit_box(np.float32)
        r32 = WR.reference_fits(X, y, WC.FIT_THETA0, lo, hi, WC.FIT_NU)
        ev = WR.warped_objective(X, y, r32["v_warped"][:4], np.exp(r32["v_warped"][4:]), WC.FIT_NU, lo, hi)[2]
        print(f"n={n}, f32 box: gain {r32['gain']:.4f} nats, cond(K) at the warped optimum {np.linalg.cond(ev['K']):.3g}")
        assert r32["gain"] > 1.0 and np.linalg.cond(ev["K"]) <= n * hi[1] / lo[0] + 1
