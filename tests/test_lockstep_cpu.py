"""CPU: the lockstep driver of the posterior-side optimisers (csrc/lockstep.hpp: maximize_ei, maximize_ehvi, maximize_qei and
paths_minimize are each one call of it around their own evaluator) against every run driven alone.

tests/cpp/test_lockstep.cpp (own main, built with AddressSanitizer + UndefinedBehaviorSanitizer): a bounded quadratic and a Rosenbrock
with +inf and NaN shells; R = 1 and 7, nvar = 1, 3, 8 and 70 (the host state), double and float with starts on the box's faces,
maxeval = 1 and 150, minimising and maximising -- every requested point, the best point, the best value and nevals agree bit for
bit with lbfgs_begin / lbfgs_request / lbfgs_advance on that run alone, with the gradient of every failed evaluation poisoned; a
run whose every evaluation fails keeps its start; an evaluator's status in round 2 ends the call.

The same program checks finite_gradient_eval (the evaluator of maximize_ehvi / maximize_constrained_ei / maximize_mes): a row is ok
iff its value and every gradient component is finite -- a value that is NaN, +inf or -inf, the last gradient component alone NaN,
+inf or -inf, a clean row -- float and double rows convert exactly, cnt = 1 and 9, d = 1, 2 and 5; a status of the call is handed on
and nothing is written."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lockstep_driver_replays_every_run_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_lockstep")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_lockstep.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "DIFFERENT" not in out.stdout and "NOT REACHED" not in out.stdout
    assert out.stdout.count("same: yes") == 59 and "59 cases, 0 problems" in out.stdout
    assert out.stdout.count("adaptor: ok") == 54 and "54 adaptor cases, 0 problems" in out.stdout and "WRONG" not in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
