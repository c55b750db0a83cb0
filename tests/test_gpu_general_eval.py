"""GPU: the general evaluation path past 128 rows -- kmat_kernel, the factorisation, gradtrace_kernel and its two finalisers --
on both sides of every feature-count boundary, in all four orders and both element types, and the fits over it with 35 and 66
parameters.  DESIGN.md section 32 has the boundaries, the case table and the worst deviation measured per family.

The cases, data, thetas, boxes and references come from tests/general_eval_cases.py, which tests/test_general_eval_cpu.py guards:
every gradient group holds a reference entry of at least 20 bars, every matrix is well conditioned (cond(K) <= 2.5e4 up to
n = 320, <= 1e5 at n = 1921), and kmat_kernel's arithmetic restated in f32 stays within 4 eps32 c of the fp64 matrix.

Bars, none of them new: parity_rules.TOL64 = 1e-8 and TOL32 = 1e-4 relative to max(1, scale) for lml, gradient, alpha, K^-1 and
diag L; for K in f64 |dK| <= 1e-14 + 1e-12 |K| (tests/test_gpu_parity.py::test_lml_grad_predict_match_golden_f64's, applied to
the whole matrix); for K in f32 8 eps32 c against the fp64 oracle on the rounded inputs: 4 for the arithmetic the guard restates,
4 for the device's expf and sqrtf (about 1 ulp each)."""
import numpy as np
import pytest

import general_eval_cases as GE
import parity_rules as PRU
from hbetune_rs_amd import gpr

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
_name = lambda t: np.dtype(t).name  # noqa: E731


def _params(cases):
    return [pytest.param(*c, dt, id=GE.case_id(*c, dt)) for c in cases for dt in GE.DTYPES]


def _dn_params(cases):
    return [pytest.param(d, n, dt, id=f"d{d}-n{n}-{_name(dt)}") for d, n in cases for dt in GE.DTYPES]


def _check_grad(what, grad, ref_grad, tol):
    """Per group, relative to max(1, max |ref|) of the whole gradient (PRU.dev's scale): a failure names the chunk."""
    scale = max(1.0, float(np.abs(ref_grad).max()))
    devs = [(name, float(np.abs(np.asarray(grad)[sl] - ref_grad[sl]).max()) / scale) for name, sl in GE.grad_groups(len(ref_grad) - 2)]
    for name, v in devs:
        assert v <= tol, f"{what}: gradient group {name} off by {v:.2e} of the gradient's scale (bar {tol:g}); all groups: {devs}"
    worst = max(v for _, v in devs)
    assert worst == PRU.dev(grad, ref_grad)
    return worst


def _evaluate(prob, theta, lo=None, hi=None):
    out = prob.lml_with_gradient(theta, lo, hi)
    assert out is not None, "not positive definite"
    alpha, kinv, ldiag = prob.results()
    return [np.array(out[0]), out[1], alpha, kinv, ldiag]


def _bytes(parts):
    """lml, gradient, alpha, the lower triangle of K^-1 (the device's own entries: the upper one is their mirror), diag L."""
    lml, grad, alpha, kinv, ldiag = parts
    return [a.tobytes() for a in (lml, grad, alpha, np.tril(kinv), ldiag)]


# ---- a. the kernel matrix, every entry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,nu,dtype", _params(GE.EVAL_CASES))
def test_kernel_matrix_every_entry(d, n, nu, dtype):
    """hbegp_problem_kmat_*: kmat_kernel<T, NU2> alone.  Where the table asks for it, also the padded matrix it left in W1
    (problem_kmat launches into the slot's W1 and copies from there): the identity the factorisation relies on beyond row n."""
    X, y, theta = GE.inputs(d, n, dtype)
    want = GE.reference(d, n, nu, _name(dtype))["kernel_matrix"]
    c = float(np.exp(theta[1]))
    prob = gpr.Problem(X, y, nu=nu)
    K = prob.kernel_matrix(theta)
    W1 = prob.debug_work_matrix(1) if (d, n) in GE.PADDING_CASES and nu == GE.nu_of(d) else None
    prob.close()
    assert K.dtype == np.dtype(dtype) and K.shape == (n, n)
    err = np.abs(K.astype(np.float64) - want)
    i, j = np.unravel_index(int(np.argmax(err)), err.shape)
    if np.dtype(dtype) == np.float64:
        allowed = 1e-14 + 1e-12 * np.abs(want)
        print(f"GE kmat d={d} n={n} nu={nu} float64: worst entry ({i}, {j}) off by {err[i, j]:.2e}, {float((err / allowed).max()):.2e} "
              f"of 1e-14 + 1e-12 |K|")
        assert (err <= allowed).all(), (i, j, err[i, j])
    else:
        print(f"GE kmat d={d} n={n} nu={nu} float32: worst entry ({i}, {j}) off by {err[i, j] / (EPS32 * c):.2f} eps32 c (bar "
              f"{GE.KMAT_BAR32_GPU})")
        assert err[i, j] <= GE.KMAT_BAR32_GPU * EPS32 * c, (i, j, err[i, j] / (EPS32 * c))
    if W1 is not None:
        npad = W1.shape[0]
        assert npad == (n + 127) // 128 * 128 and npad > n
        low = np.tril(W1)
        assert np.array_equal(low[n:, :], np.eye(npad, dtype=W1.dtype)[n:, :]), "the padding is not the identity"
        assert np.tril(W1[:n, :n]).tobytes() == np.tril(K).tobytes(), "the live part of W1 is not what kernel_matrix returned"
        print(f"GE kmat d={d} n={n} {_name(dtype)}: rows {n}..{npad - 1} of W1 are the identity's, bit for bit")


# ---- b. lml, gradient per group, alpha, K^-1, diag L ---------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,nu,dtype", _params(GE.EVAL_CASES))
def test_evaluation_against_the_reference(d, n, nu, dtype):
    """hbegp_problem_eval + hbegp_problem_get_*: the three launches of every fit and of the benchmark.  gradtrace_kernel<T, NU2>
    past its first chunk of eight (kc > 0: no lead, published at my + 2 + kc), finalised inside the launch up to n = 320 and by
    finalize_grad_kernel over d + 2 workgroups at n = 1921."""
    X, y, theta = GE.inputs(d, n, dtype)
    ref = GE.reference(d, n, nu, _name(dtype))
    tol = GE.tol_of(dtype)
    what = f"d={d} n={n} nu={nu} {_name(dtype)}"
    prob = gpr.Problem(X, y, nu=nu)
    got = _evaluate(prob, theta)
    again = _evaluate(prob, theta) if (d, n) == (64, GE.N_BIG) else None
    prob.close()
    lml, grad, alpha, kinv, ldiag = got
    assert np.isfinite(grad).all() and grad.shape == (d + 2,)
    devs = dict(lml=PRU.dev(lml, ref["lml"]), alpha=PRU.dev(alpha, ref["alpha"]), kinv=PRU.dev(kinv, ref["k_inv"]),
                ldiag=PRU.dev(ldiag, ref["ldiag"]))
    scale = max(1.0, float(np.abs(ref["grad"]).max()))
    print(f"GE eval {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in devs.items()) +
          f", grad {float(np.abs(grad - ref['grad']).max()) / scale:.2e} (bar {tol:g})")
    for k, v in devs.items():
        assert v <= tol, (what, k, v)
    _check_grad(f"eval {what}", grad, ref["grad"], tol)
    if again is not None:
        assert _bytes(again) == _bytes(got), "a second evaluation returned other bytes"


# ---- c. the other finaliser ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,dtype", _dn_params(GE.HOSTIO_CASES + ((9, GE.N_BIG),)))
def test_both_finalisers_return_the_same_bytes(d, n, dtype, monkeypatch):
    """HBEGP_HOSTIO=0 (read when the problem is created): copy nodes, finalize_grad_kernel over p = 11 and 66 workgroups and a
    stream synchronise, against finalize_grad_in_block by the launch's last workgroup.  At n = 1921 both settings launch
    finalize_grad_kernel (tests/test_general_eval_cpu.py::test_the_finaliser_rule_is_enqueue_evals)."""
    X, y, theta = GE.inputs(d, n, dtype)
    nu = GE.nu_of(d)
    out = {}
    for hostio in ("1", "0"):
        monkeypatch.setenv("HBEGP_HOSTIO", hostio)
        prob = gpr.Problem(X, y, nu=nu)
        out[hostio] = _evaluate(prob, theta)
        prob.close()
    assert np.isfinite(out["1"][1]).all()
    for name, a, b in zip(("lml", "grad", "alpha", "tril K^-1", "diag L"), _bytes(out["1"]), _bytes(out["0"])):
        assert a == b, (d, n, _name(dtype), name)


# ---- d. two-phase trials at d > 8 ----------------------------------------------------------------------------------------------
def _fit_outputs(fk):
    alpha, kinv = fk.arrays()
    return dict(theta=fk.theta.copy(), theta_best=fk.theta_best.copy(), lml=np.array([fk.lml]), alpha=alpha, kinv_lower=np.tril(kinv),
                counts=np.array([fk.n_evals, fk.n_not_pd]))


@pytest.mark.parametrize("dtype", GE.DTYPES, ids=_name)
def test_two_phase_trials_past_eight_features(dtype, monkeypatch):
    """A fit at (17, 257): trials the line search rejects end after their lml, the ones it keeps run EVAL_GRAD_ONLY (the K^-1 tiles
    and gradtrace_kernel over three chunks on what the first phase left).  The same bytes as with every trial evaluated whole."""
    d, n = GE.TWO_PHASE_CASE
    X, y, theta = GE.inputs(d, n, dtype)
    lo, hi = GE.fit_box(theta)
    theta0, starts = GE.two_phase_starts(d, n, theta)
    out, skipped = {}, {}
    for lazy in ("0", None):
        if lazy is None:
            monkeypatch.delenv("HBEGP_LAZY_GRAD")
        else:
            monkeypatch.setenv("HBEGP_LAZY_GRAD", lazy)
        fk = gpr.FittedKernel.new(X, y, theta0, lo, hi, starts, nu=GE.nu_of(d), maxeval=GE.TWO_PHASE_MAXEVAL)
        out[lazy], skipped[lazy] = _fit_outputs(fk), fk.n_lml_only
        fk.release()
    print(f"GE two-phase d={d} n={n} {_name(dtype)}: {int(out[None]['counts'][0])} evaluations, {skipped[None]} of them lml only")
    assert skipped["0"] == 0 and skipped[None] >= 1, skipped
    assert out[None]["counts"][1] == 0
    for k in out["0"]:
        assert out["0"][k].dtype == out[None][k].dtype and out["0"][k].tobytes() == out[None][k].tobytes(), k


# ---- e. fits with 35 and 66 parameters -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,dtype", _dn_params(GE.FIT_CASES))
def test_fit_trace_replays_on_the_reference(d, n, dtype):
    """The host-driven general path with p = 35 and p = 66 = LBFGS_MAXN: every traced (theta, lml, gradient) against the
    reference at that theta, the gradient per group; the optimiser really moves; the model is `extend` at the captured theta."""
    X, y, theta = GE.inputs(d, n, dtype)
    Xr, yr, _ = GE.rounded_inputs(d, n, dtype)
    nu, tol = GE.nu_of(d), GE.tol_of(dtype)
    lo, hi = GE.fit_box(theta)
    fk = gpr.FittedKernel.new(X, y, theta, lo, hi, GE.fit_starts(d, n, theta, 1), nu=nu, maxeval=GE.FIT_MAXEVAL, trace=True)
    tr = fk.trace
    assert fk.n_not_pd == 0 and len(tr["lml"]) == fk.n_evals > 0
    worst, worst_cond = [0.0, 0.0], 0.0
    for i, th in enumerate(tr["theta"]):
        ref = GE.reference_at(Xr, yr, th, nu, lo, hi)
        worst_cond = max(worst_cond, GE.cond(ref["kernel_matrix"]))
        worst[0] = max(worst[0], PRU.dev(tr["lml"][i], ref["lml"]))
        assert worst[0] <= tol, (i, worst[0])
        worst[1] = max(worst[1], _check_grad(f"fit d={d} n={n} {_name(dtype)} evaluation {i}", tr["grad"][i], ref["grad"], tol))
    print(f"GE fit d={d} n={n} {_name(dtype)}: {len(tr['lml'])} traced evaluations, lml off by {worst[0]:.2e}, gradient by {worst[1]:.2e} "
          f"(bar {tol:g}), largest cond(K) {worst_cond:.0f}")
    assert worst_cond <= GE.COND_MAX, worst_cond
    runs = [np.flatnonzero(tr["run"] == r) for r in (0, 1)]
    assert sorted(np.unique(tr["run"]).tolist()) == [0, 1] and all(len(r) >= 2 for r in runs), [len(r) for r in runs]
    best = int(np.argmax(tr["lml"]))
    assert tr["lml"][best] == fk.lml
    assert best != runs[int(tr["run"][best])][0], "the best evaluation is its run's start point: the optimiser did not move"
    th_cap = tr["theta"][best]
    # (tests/test_gpu_rv.py::test_fit_trace_replays_on_the_reference_and_the_model_is_extend has the reasons for this rounding)
    assert np.all(np.abs(fk.theta_best - th_cap) <= (np.abs(th_cap) + 2) * np.finfo(float).eps), fk.theta_best - th_cap
    assert np.array_equal(fk.theta_best, fk.theta)
    ex = gpr.FittedKernel.extend(X, y, th_cap, lo, hi, nu=nu)
    if np.dtype(dtype) == np.float64:
        assert ex.lml == fk.lml
        assert all(a.tobytes() == b.tobytes() for a, b in zip(fk.arrays(), ex.arrays()))
    else:
        assert PRU.dev(ex.lml, fk.lml) <= PRU.TOL32
    fk.release(); ex.release()
