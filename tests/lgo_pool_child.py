"""Child process of tests/test_gpu_lgo.py (pool hygiene): hbegp_model_lgo with a gradient at n = 200, once per pool setting named in
argv[2:] ("fresh": HBEGP_POOL_FRESH=1, "poison1" / "poison2": HBEGP_POOL_POISON=1 / 2, "plain": no switch -- the call then recycles
the blocks the calls before it gave back; the library reads the switches on every hand-out).  Writes every call's outputs and the
number of blocks / bytes the pool poisoned during it to the .npz named in argv[1], keys prefixed with the setting."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lgo_ref as GR  # noqa: E402
from hbetune_rs_amd import _lib, gpr  # noqa: E402


def _poisoned():
    blocks, nbytes = C.c_longlong(0), C.c_longlong(0)
    _lib.check(_lib.load().hbegp_debug_pool_poisoned(C.byref(blocks), C.byref(nbytes)))
    return blocks.value, nbytes.value


SETTINGS = {"fresh": {"HBEGP_POOL_FRESH": "1"}, "poison1": {"HBEGP_POOL_POISON": "1"}, "poison2": {"HBEGP_POOL_POISON": "2"}, "plain": {}}


def main(out, settings):
    n = 200
    rng = np.random.default_rng(n)
    X = rng.uniform(0, 1, (n, 4))
    y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(n)
    theta = np.log(np.concatenate([[1.3e-2, 1.3], np.linspace(0.3, 0.9, 4)]))
    g = GR.group_mix(n)
    fk = gpr.FittedKernel.extend(X, y, theta)
    res = {}
    for name in settings:
        for k in ("HBEGP_POOL_FRESH", "HBEGP_POOL_POISON"):
            os.environ.pop(k, None)
        os.environ.update(SETTINGS[name])
        b0 = _poisoned()
        got = fk.lgo(g, want_grad=True)
        b1 = _poisoned()
        res.update({f"{name}_{k}": np.asarray(v) for k, v in zip(("mean", "var", "lpd", "lgo", "grad"), got)})
        res[f"{name}_blocks"], res[f"{name}_bytes"] = b1[0] - b0[0], b1[1] - b0[1]
    fk.release()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
