"""CPU checks of the Monte Carlo batch expected improvement (hbegp_qei_* / hbegp_maximize_qei_*): the symbols and their signatures,
register and LDS use of the new kernel, argument checks that refuse before any device call, the NumPy restatement (tests/qei_ref.py)
pinned against torch.autograd, central differences and the q = 1 closed form, the leading-block property of the factor, and the
host-side L-BFGS state that the maximiser runs on (tests/cpp/test_lbfgs_host_state.cpp)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import predict_grad_ref as PG
import qei_ref as QR
from hbetune_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ("hbegp_qei_f64", "hbegp_qei_f32", "hbegp_maximize_qei_f64", "hbegp_maximize_qei_f32", "hbegp_debug_qei_phases")
NUS = [0.5, 1.5, 2.5, math.inf]


def test_qei_symbols_are_exported_with_signatures():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def _kernel_notes(isa):
    out = {}
    meta = isa[isa.index("amdhsa.kernels:"):]
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+_count|\w+_segment_fixed_size):\s+(\d+)", block)}
    return out


def test_qei_kernel_does_not_spill_and_fits_the_lds():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", ROOT, "build/kernels.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "build", "kernels.s")) as f:
        notes = _kernel_notes(f.read())
    found = [k for k in notes if "qei_batch_kernel" in k]
    assert len(found) == 2, found  # f64 and f32
    for sym in found:
        assert notes[sym]["vgpr_spill_count"] == 0 and notes[sym]["sgpr_spill_count"] == 0, (sym, notes[sym])
        assert notes[sym]["private_segment_fixed_size"] == 0, (sym, notes[sym])
    assert notes[sym]["group_segment_fixed_size"] == 0, (sym, notes[sym])  # all of its LDS is the dynamic request below


def test_qei_lds_request_fits_one_cu(tmp_path):
    """The dynamic LDS the launcher requests (engine.hpp: qei_lds_bytes, also what the start-up raises the limit to) at the largest
    batch the call accepts, q = QEI_MAXQ and d = MAXD, read from the header itself."""
    src = tmp_path / "lds.cpp"
    src.write_text('#include <cstdio>\n#include "engine.hpp"\nint main() { std::printf("%zu %d %d\\n", '
                   "hbegp::qei_lds_bytes(hbegp::QEI_MAXQ, hbegp::MAXD), hbegp::QEI_MAXQ, hbegp::MAXD); }\n")
    exe = str(tmp_path / "lds")
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "csrc"),
                           str(src), "-o", exe])
    nbytes, maxq, maxd = map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert (maxq, maxd) == (64, 64)
    assert nbytes <= 160 * 1024, nbytes


def _einval(rc, what):
    assert rc == _lib.EINVAL
    assert what in _lib.last_error(), _lib.last_error()


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    d, f = _lib.dptr, _lib.fptr
    x, z, out, g = np.zeros(64), np.zeros(64), np.zeros(8), np.zeros(64)
    xf, zf, gf = np.zeros(64, np.float32), np.zeros(64, np.float32), np.zeros(64, np.float32)
    info = np.zeros(8, np.int32)
    ip = info.ctypes.data_as(C.POINTER(C.c_int))
    for fn, xp, zp, gp in ((lib.hbegp_qei_f64, d(x), d(z), d(g)), (lib.hbegp_qei_f32, f(xf), f(zf), f(gf))):
        _einval(fn(None, xp, 2, 2, zp, 4, 0.0, 0.0, d(out), gp, ip), "NULL model")
        _einval(fn(None, xp, 2, 0, zp, 4, 0.0, 0.0, d(out), gp, ip), "q must be in [1, 64]")
        _einval(fn(None, xp, 2, 65, zp, 4, 0.0, 0.0, d(out), gp, ip), "q must be in [1, 64]")
        _einval(fn(None, xp, -1, 2, zp, 4, 0.0, 0.0, d(out), gp, ip), "B must be >= 0")
        _einval(fn(None, xp, 2, 2, zp, 0, 0.0, 0.0, d(out), gp, ip), "S must be >= 1")
        _einval(fn(None, xp, 2, 2, None, 4, 0.0, 0.0, d(out), gp, ip), "z is NULL")
        for bad in (math.nan, math.inf, -math.inf):
            _einval(fn(None, xp, 2, 2, zp, 4, bad, 0.0, d(out), gp, ip), "fmin must be finite")
        for bad in (-1e-9, math.nan, math.inf):
            _einval(fn(None, xp, 2, 2, zp, 4, 0.0, bad, d(out), gp, ip), "jitter must be finite and >= 0")
        _einval(fn(None, xp, 0, 2, zp, 4, 0.0, 0.0, None, None, None), "NULL model")  # B = 0 still needs a model
    lo, hi, qo = np.zeros(4), np.ones(4), np.zeros(4)
    for fn, xp, zp in ((lib.hbegp_maximize_qei_f64, d(x), d(z)), (lib.hbegp_maximize_qei_f32, f(xf), f(zf))):
        _einval(fn(None, xp, 0, 2, d(lo), d(hi), zp, 4, 0.0, 0.0, 10, xp, d(qo), None), "R must be >= 1")
        _einval(fn(None, xp, 1, 2, d(lo), d(hi), zp, 4, 0.0, 0.0, 0, xp, d(qo), None), "maxeval must be >= 1")
        _einval(fn(None, xp, 1, 2, d(lo), d(hi), zp, 4, 0.0, 0.0, 10, xp, d(qo), None), "NULL model")
        _einval(fn(None, xp, 1, 70, d(lo), d(hi), zp, 4, 0.0, 0.0, 10, xp, d(qo), None), "q must be in [1, 64]")
        _einval(fn(None, xp, 1, 2, d(lo), d(hi), zp, 4, math.nan, 0.0, 10, xp, d(qo), None), "fmin must be finite")
    # (the element type, a non-finite coordinate, lo > hi and a start outside the box need a model: tests/test_gpu_qei.py)


def _post(nu, n=40, d=3, seed=0, noise=1e-2):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    return QR.Posterior(X, y, 1.7, np.array([0.3, 0.5, 0.8][:d]), nu, noise), y, rng


@pytest.mark.parametrize("jitter", [0.0, 1e-6])
@pytest.mark.parametrize("nu", NUS)
def test_restatement_is_torch_autograd(nu, jitter):
    post, y, rng = _post(nu)
    fmin = float(np.median(y))  # most draws improve: every term of the reverse pass is exercised
    for q, S in ((1, 300), (2, 64), (5, 500), (12, 1000)):
        xb = rng.uniform(-0.1, 1.1, (q, 3))
        z = rng.standard_normal((S, q))
        v, g = QR.qei_batch(post, xb, z, fmin, jitter)
        tv, tg = QR.qei_torch(post, xb, z, fmin, jitter)
        assert v > 0
        assert abs(v - tv) <= 1e-12 * abs(tv), (q, v, tv)
        assert np.abs(g - tg).max() <= 1e-12 * np.abs(tg).max(), (q, np.abs(g - tg).max())


@pytest.mark.parametrize("nu", [1.5, 2.5, math.inf])
def test_restatement_gradient_is_central_differences(nu):
    post, y, rng = _post(nu, seed=3)
    fmin = float(y.min()) + 0.3
    xb = rng.uniform(-0.1, 1.1, (4, 3))
    z = rng.standard_normal((400, 4))
    _, g = QR.qei_batch(post, xb, z, fmin)
    h = 1e-6
    fd = np.zeros_like(xb)
    for a in range(4):
        for k in range(3):
            xp, xm = xb.copy(), xb.copy()
            xp[a, k] += h
            xm[a, k] -= h
            fd[a, k] = (QR.qei_batch(post, xp, z, fmin)[0] - QR.qei_batch(post, xm, z, fmin)[0]) / (2 * h)
    assert np.abs(fd - g).max() <= 1e-6 * np.abs(g).max(), np.abs(fd - g).max()


@pytest.mark.parametrize("nu", NUS)
def test_q1_is_the_closed_form(nu):
    post, y, rng = _post(nu, seed=5)
    fmin = float(y.min()) + 0.3
    xs = rng.uniform(-0.1, 1.1, (6, 3))
    z = rng.standard_normal((700, 1))
    dmean = PG.dmean_ref(xs, post.X, post.alpha, post.amp, post.ell, nu)
    dvar = PG.dvar_ref(xs, post.X, post.amp, post.ell, nu, post.noise)
    for i in range(6):
        mu, S, *_ = post.batch(xs[i:i + 1])
        sd = math.sqrt(S[0, 0])
        f = mu[0] + sd * z[:, 0]
        act = f < fmin
        ref = np.maximum(fmin - f, 0.0).sum() / len(z)
        rg = (-dmean[i][None, :] - z[act, 0][:, None] * dvar[i][None, :] / (2 * sd)).sum(axis=0) / len(z)
        v, g = QR.qei_batch(post, xs[i:i + 1], z, fmin)
        assert abs(v - ref) <= 1e-13 * max(1.0, ref)
        assert np.abs(g[0] - rg).max() <= 1e-12 * max(1.0, np.abs(rg).max())


def test_adding_a_point_keeps_the_leading_factor_and_cannot_lower_qei():
    post, y, rng = _post(2.5, seed=7)
    fmin = float(y.min()) + 0.3
    xb = rng.uniform(-0.1, 1.1, (6, 3))
    z = rng.standard_normal((2000, 6))
    prev = -1.0
    for q in range(1, 7):
        mu, S, *_ = post.batch(xb[:q])
        L = np.linalg.cholesky(S)
        if q > 1:
            assert np.allclose(L[:q - 1, :q - 1], Lprev, rtol=0, atol=1e-13)
        Lprev = L
        v, _ = QR.qei_batch(post, xb[:q], z[:, :q], fmin)
        assert v >= prev - 1e-13  # every draw's minimum over more points is no larger (to the rounding of L)
        prev = v


def test_host_lbfgs_state_replays_the_fixed_state(tmp_path):
    exe = str(tmp_path / "test_lbfgs_host_state")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_lbfgs_host_state.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "DIFFERENT" not in out.stdout and out.stdout.count("same") == 10
