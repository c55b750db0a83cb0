"""CPU guard of tests/test_gpu_incremental.py.

(a) The NumPy fp64 restatement of Problem::extend_from's block formulas (tests/incremental_cases.py::restate) equals the inverse
    and the oracle's FittedKernel::extend on every case of the table, and gives the q0 / nb / fix classification the table states.
(b) On every case, in both noise regimes, each term the engine adds into or takes out of K^-1 -- the fix term Xp21^T Xp21, the
    added term X21^T X21, the new x kept block -- reaches at least 10 x the device bar of max |K^-1|: a dropped or misplaced term
    fails the device comparison instead of hiding under the bar."""
import math

import numpy as np
import pytest

import incremental_cases as IC
import parity_rules as PR
from oracle import gpr_oracle as O

GUARD = 10.0  # x the device tolerance, of max |K^-1|
RESTATE_TOL = 1e-10  # fp64 block algebra against LAPACK's inverse at cond(K) <= 2e4 (noise >= 1e-2 c, n <= 900): eps cond ~ 4e-12


@pytest.fixture(scope="module")
def restated():
    """restate() of every (case, noise regime), computed once."""
    out = {}
    for case in IC.CASES:
        for dtype in IC.DTYPES:
            X, y, theta = IC.inputs(case, dtype)
            K = IC.kernel_matrix(X, theta, case[3])
            out[IC.case_id(case), np.dtype(dtype).name] = (K, IC.restate(K, y, case[0]))
    return out


@pytest.mark.parametrize("case", IC.CASES, ids=IC.case_id)
def test_classification(case):
    n0, n, d, nu, q0, nb, fix = case
    assert IC.geometry(n0, n) == (q0, nb, fix)
    # the fix runs exactly where the prior has rows beyond the kept blocks
    assert fix == (n0 > q0 * IC.NB)


def test_the_table_covers_what_it_claims():
    for nu in (0.5, 1.5, 2.5, math.inf):
        fixes = {c[6] for c in IC.CASES if c[3] == nu}
        assert fixes == {True, False}, (nu, fixes)
    assert IC.geometry(*IC.FALLBACK_128[:2])[0] == 0  # nothing to keep: the engine reports incremental == False
    assert any(c[1] == c[0] and c[1] % IC.NB for c in IC.CASES) and any(c[0] == IC.NB for c in IC.CASES)
    assert max(c[1] for c in IC.CASES) <= 900 and max(c[2] for c in IC.CASES) == 64


@pytest.mark.parametrize("dtype", IC.DTYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("case", IC.CASES, ids=IC.case_id)
def test_restatement_equals_the_inverse_and_the_oracle(case, dtype, restated):
    n0, n, d, nu = case[:4]
    K, r = restated[IC.case_id(case), np.dtype(dtype).name]
    assert (r["q0"], r["nb"], r["fix"]) == case[4:]
    kinv = np.linalg.inv(K)
    s = np.abs(kinv).max()
    for name, (ri, ci) in IC.regions(r["w"]).items():
        assert np.abs(r["kinv"][ri, ci] - kinv[ri, ci]).max() <= RESTATE_TOL * s, name
    assert np.abs(r["X"] - np.linalg.inv(np.linalg.cholesky(K))).max() <= RESTATE_TOL * np.abs(r["X"]).max()
    X, y, theta = IC.inputs(case, dtype)
    noise, c, ell = IC.params(theta)
    ref = O.extend(X.astype(np.float64), y.astype(np.float64), noise, c, ell, nu)
    assert PR.dev([r["lml"]], [ref["lml"]]) <= RESTATE_TOL
    assert PR.dev(r["alpha"], ref["alpha"]) <= RESTATE_TOL
    assert np.abs(r["kinv"] - ref["k_inv"]).max() <= RESTATE_TOL * s
    assert np.abs(r["ldiag"] - np.diag(ref["chol"])).max() <= RESTATE_TOL * np.abs(r["ldiag"]).max()
    # without the fix where it is due (or with it where it is not) the kept block is wrong by the whole fix term
    if r["fix"]:
        assert np.abs(r["kinv"][:r["w"], :r["w"]] + r["fix_term"] - kinv[:r["w"], :r["w"]]).max() > 1e3 * RESTATE_TOL * s
    else:
        assert r["fix_term"].size == 0 or np.abs(r["fix_term"]).max() == 0.0


def test_nothing_to_keep_below_one_block():
    n0, n, d, nu = IC.FALLBACK_128
    X, y = IC.data(n, d, np.float64)
    assert IC.restate(IC.kernel_matrix(X, IC.theta_of(d, nu, np.float64), nu), y, n0) is None


@pytest.mark.parametrize("dtype", IC.DTYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("case", IC.CASES, ids=IC.case_id)
def test_every_term_is_visible_to_the_device_bar(case, dtype, restated):
    K, r = restated[IC.case_id(case), np.dtype(dtype).name]
    s = np.abs(r["kinv"]).max()
    need = GUARD * IC.tol_of(dtype)
    terms = {"added term": r["added_term"], "new x kept": r["new_kept"]}
    if r["fix"]:
        terms["fix term"] = r["fix_term"]
    got = {k: float(np.abs(v).max() / s) for k, v in terms.items()}
    print(f"guard {IC.case_id(case)} {np.dtype(dtype).name}: " + ", ".join(f"{k} {v:.2e}" for k, v in got.items()) + f" (need {need:g})")
    for k, v in got.items():
        assert v >= need, (k, v, need)
