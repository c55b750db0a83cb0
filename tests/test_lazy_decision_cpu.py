"""CPU: the decision a fit takes before it pays for the gradient of a line-search trial (csrc/lbfgs_step.hpp:
lbfgs_is_trial / lbfgs_trial_accepted) says exactly what lbfgs_advance then does.

tests/cpp/test_lbfgs_decision.cpp (own main, built with AddressSanitizer + UndefinedBehaviorSanitizer): 48 randomised bounded
objectives with failing (+inf) and NaN regions and a constructed objective whose rejected trial is a new best -- the query agrees
with lbfgs_advance at every evaluation, and a run whose rejected trials get a poisoned gradient evaluates the points of
lbfgsb_minimize_loops bit for bit.  The second test asks the same of the library's own build through the debug ABI."""
import ctypes as C
import os
import subprocess

import numpy as np

from hbetune_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decision_query_agrees_with_the_state_machine_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_lbfgs_decision")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_lbfgs_decision.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "DIFFERENT" not in out.stdout and out.stdout.count(" same:") == 50 and ", 0 problems" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def decisions(x0, lo, hi, f, g, maxeval=150, fixed_work=False):
    lib = _lib.load()
    n, count = len(x0), len(f)
    req = np.zeros((count, n))
    trial, acc, took = (np.zeros(count, dtype=np.int32) for _ in range(3))
    nreq = C.c_int(0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    _lib.check(lib.hbegp_debug_lbfgs_decisions(n, _lib.dptr(np.asarray(x0, float)), _lib.dptr(np.asarray(lo, float)), _lib.dptr(np.asarray(hi, float)),
                                               maxeval, 0, int(fixed_work), count, _lib.dptr(f), _lib.dptr(g), _lib.dptr(req), ip(trial), ip(acc),
                                               ip(took), C.byref(nreq)))
    return req, trial, acc, took, nreq.value


def test_library_decision_query_on_recorded_values():
    # values that are NOT a function of the point (a recorded sequence is all the state machine sees): random walks around the
    # incumbent with +inf and NaN entries; whatever comes, accepted == took, and only trials are ever accepted
    rng = np.random.default_rng(5)
    seen_rejected = seen_accepted = seen_bad = 0
    for rep in range(20):
        n = int(rng.integers(1, 9))
        count = 60
        f = np.cumsum(rng.normal(-0.3, 1.0, count))
        bad = rng.random(count) < 0.1
        f[bad & (rng.random(count) < 0.5)] = np.inf
        f[bad & ~np.isinf(f)] = np.nan
        if rep % 5:
            f[0] = 0.0  # a start point that works
        g = rng.normal(0, 1, (count, n))
        req, trial, acc, took, nreq = decisions(rng.normal(0, 1, n), np.full(n, -3.0), np.full(n, 3.0), f, g, maxeval=count, fixed_work=bool(rep % 2))
        assert 1 <= nreq <= count
        k = nreq  # evaluations the state machine consumed a value for
        assert np.array_equal(acc[:k], took[:k])
        assert not np.any(acc[:k] & ~trial[:k].astype(bool))
        assert not np.any(acc[:k][~np.isfinite(f[:k])])
        seen_accepted += int(acc[:k].sum())
        seen_rejected += int((trial[:k] & ~acc[:k].astype(bool)).sum())
        seen_bad += int((~np.isfinite(f[:k]) & trial[:k].astype(bool)).sum())
    assert seen_accepted > 20 and seen_rejected > 20 and seen_bad > 3
