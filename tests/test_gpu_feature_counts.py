"""GPU: the d-dependent feature kernels on both sides of every feature-count boundary, at row counts on the tile edges of the
leave-one-out tail -- leave-one-out CV, posterior gradients, the joint covariance, q-EI and the sample paths, each against its
NumPy restatement at the device's parameters.  DESIGN.md section 17 has the table of boundaries (kernel, constant, the d that
straddle it) and the worst deviation measured per family and element type over this grid.

The cases, data, thetas, query points and draws come from tests/feature_count_cases.py, which tests/test_feature_counts_cpu.py
guards: every group of eight length-scale entries of the leave-one-out gradient and every group of 16 columns of dmean holds an
entry far above the bar, so that a dropped or misplaced chunk cannot hide below a comparison relative to the largest entry.

Bars, none of them new: parity_rules.TOL64 = 1e-8 and TOL32 = 1e-4, each exactly as the feature's own test file applies it
(tests/test_gpu_loo.py::_check, predict_grad_ref.row_dev, Sigma and the variance relative to c, tests/test_gpu_qei.py::_check,
tests/test_gpu_paths.py::_compare).  Models are well conditioned: cond(K) <= 2.5e4 in f64, <= n + 1 in f32."""
import math

import numpy as np
import pytest

import feature_count_cases as FC
import loo_ref as LR
import parity_rules as PRU
import paths_ref as PR
import posterior_cov_ref as PC
import predict_grad_ref as PG
import qei_ref as QR
from hbetune_rs_amd import estimator as E
from hbetune_rs_amd import gpr
from oracle import gpr_oracle as O

pytestmark = pytest.mark.gpu


def _cases(table):
    """(d, n[, nu]) x element type, with ids that name the case."""
    return [pytest.param(*c, dt, id=f"d{c[0]}-n{c[1]}" + (f"-nu{c[2]}" if len(c) > 2 else "") + f"-{np.dtype(dt).name}")
            for c in table for dt in FC.DTYPES]


class Model:
    """One case's model (FittedKernel.extend at the case's theta) and the parameters its kernels use."""

    def __init__(self, d, n, dtype, nu=None):
        self.d, self.n, self.dtype = d, n, np.dtype(dtype)
        self.nu = FC.nu_of(d) if nu is None else nu
        self.X, self.y, self.theta = FC.inputs(d, n, dtype)
        self.tol = FC.tol_of(dtype)
        self.fk = gpr.FittedKernel.extend(self.X, self.y, self.theta, nu=self.nu)
        self.noise, self.amp, self.ell = self.fk.device_params()
        # exp(theta) up to the rounding of theta (tests/test_gpu_model_kinds.py)
        want, got = np.exp(self.theta), np.concatenate([[self.noise, self.amp], self.ell])
        assert (np.abs(got - want) <= (np.abs(self.theta) + 2) * np.finfo(float).eps * want).all(), (got, want)
        self.X64, self.y64 = self.X.astype(np.float64), self.y.astype(np.float64)
        self.what = f"d={d} n={n} nu={self.nu} {self.dtype.name}"

    def release(self):
        self.fk.release()


def _grad_groups(d):
    """The leave-one-out gradient by what gradtrace_tile publishes together: the noise / amplitude lead, then each chunk of eight
    length scales."""
    return [("noise, amplitude", slice(0, 2))] + [(f"ell[{s.start}:{s.stop}]", slice(2 + s.start, 2 + s.stop))
                                                 for s in FC.groups(d, FC.GROUP_LOO)]


def _check_loo_grad(what, grad, ref_grad, tol):
    """Per group, relative to max(1, max |ref|) of the whole gradient (PRU.dev's scale): a failure names the chunk."""
    scale = max(1.0, float(np.abs(ref_grad).max()))
    devs = [(name, float(np.abs(np.asarray(grad)[sl] - ref_grad[sl]).max()) / scale) for name, sl in _grad_groups(len(ref_grad) - 2)]
    for name, v in devs:
        assert v <= tol, f"{what}: gradient group {name} off by {v:.2e} of the gradient's scale (bar {tol:g}); all groups: {devs}"
    return max(v for _, v in devs)


def _check_loo(what, got, ref, tol, c_plus_s2):
    """tests/test_gpu_loo.py::_check, with the gradient judged per group."""
    mean, var, lpd, loo, grad = got
    devs = dict(mean=PRU.dev(mean, ref["mean"]), var=PRU.dev(var, ref["var"], scale=1.0) / c_plus_s2, lpd=PRU.dev(lpd, ref["lpd"]),
                loo=PRU.dev(loo, ref["loo"]))
    for k, v in devs.items():
        assert v <= tol, (what, k, v)
    devs["grad"] = _check_loo_grad(what, grad, ref["grad"], tol)
    assert devs["grad"] == PRU.dev(grad, ref["grad"])
    return devs


@pytest.mark.parametrize("d,n,dtype", _cases(FC.LOO_CASES))
def test_loo(d, n, dtype):
    """hbegp_model_loo_* and hbegp_problem_eval_loo: gradtrace_tile<.., LOO = true> past its first chunk of eight (kc > 0: no
    lead, published at part + 2 + kc) and the tail's 64-tiles and 256-row chunks at n = 256, 257, 320 (and 90: one block)."""
    m = Model(d, n, dtype)
    ref = LR.loo_at_theta(m.X, m.y, m.theta, m.nu)
    got = m.fk.loo(want_grad=True)
    devs = _check_loo(f"loo {m.what} model", got, ref, m.tol, m.amp + m.noise)
    m.release()
    lo, hi, (theta, clamped) = FC.box_and_thetas(m.theta)
    prob = gpr.Problem(m.X, m.y, nu=m.nu)
    worst = np.zeros(2)
    for what, th, r in (("theta", theta, ref), ("clamped", clamped, None)):
        r = r or LR.loo_at_theta(m.X, m.y, th, m.nu, lo, hi)  # (theta lies inside the box: the reference above)
        loo, grad = prob.loo_with_gradient(th, lo, hi)
        d_l = PRU.dev(loo, r["loo"])
        assert d_l <= m.tol, (what, d_l)
        worst = np.maximum(worst, [d_l, _check_loo_grad(f"loo {m.what} problem at {what}", grad, r["grad"], m.tol)])
    prob.close()
    print(f"FC loo {m.what}: model " + ", ".join(f"{k} {v:.2e}" for k, v in devs.items()) +
          f"; problem loo {worst[0]:.2e} grad {worst[1]:.2e} (bar {m.tol:g})")


def _row_dev_by_pass(what, got, ref, tol):
    """PG.row_dev (relative to each row's largest entry over all columns), judged per group of 16 columns: a failure names
    pred_grad_kernel's pass."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max(axis=1)
    scale = np.where(scale > 0, scale, 1.0)
    worst = 0.0
    for sl in FC.groups(ref.shape[1], FC.GROUP_DMEAN):
        v = float((np.abs(got[:, sl] - ref[:, sl]).max(axis=1) / scale).max())
        assert v <= tol, f"{what}: columns {sl.start}:{sl.stop} off by {v:.2e} of their row's scale (bar {tol:g})"
        worst = max(worst, v)
    assert worst == PG.row_dev(got, ref)
    return worst


@pytest.mark.parametrize("d,n,dtype", _cases(FC.QUERY_CASES))
def test_predict_and_gradient(d, n, dtype):
    """hbegp_predict_* and hbegp_predict_grad_* at m = 5 (the handful path) and 70 (ragged over the four rows per workgroup and
    the 64-tile), two query rows on training rows: kstar_kernel / kstar_small_kernel, pred_grad_kernel past one pass of 16
    features (d >= 17) and two (d >= 33), and the d planes of kstar_grad_kernel, the W_k GEMMs and pred_dvar_kernel."""
    m = Model(d, n, dtype)
    ref = O.extend(m.X64, m.y64, m.noise, m.amp, m.ell, m.nu)
    pool = FC.query_points(m.X, dtype)
    worst = {}
    for mq in FC.M_QUERY:
        Xs = pool[:mq]
        X64 = Xs.astype(np.float64)
        lm, lv, _ = O.predict(X64, m.X64, ref["alpha"], ref["k_inv"], m.amp, m.ell, m.nu)
        rm = PG.dmean_ref(X64, m.X64, ref["alpha"], m.amp, m.ell, m.nu)
        assert (rm[[1, 3]] != 0).any(axis=1).all()
        for path, out in (("predict", m.fk.predict(Xs)), ("gradient", m.fk.predict_with_gradient(Xs))):
            mean, var = out[0], out[1]
            devs = {"mean": PRU.dev(mean, lm), "var": PRU.dev(var, lv, scale=1.0) / m.amp}
            if path == "gradient":
                dmean, dvar = out[2], out[3]
                assert dmean.dtype == m.dtype and dmean.shape == (mq, d) and dvar.shape == (mq, d)
                assert np.isfinite(dmean).all() and np.isfinite(dvar).all()
                rv = PG.dvar_ref(X64, m.X64, m.amp, m.ell, m.nu, m.noise, var=var)
                devs["dmean"] = _row_dev_by_pass(f"{m.what} m={mq} dmean", dmean, rm, m.tol)
                devs["dvar"] = _row_dev_by_pass(f"{m.what} m={mq} dvar", dvar, rv, m.tol)
            for k, v in devs.items():
                assert v <= m.tol, (m.what, mq, path, k, v)
                worst[k] = max(worst.get(k, 0.0), v)
    m.release()
    print(f"FC predict {m.what}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bar {m.tol:g})")


@pytest.mark.parametrize("d,n,dtype", _cases(FC.QUERY_CASES))
def test_predict_cov(d, n, dtype):
    """hbegp_predict_cov_* at m = 70: K* and the K** behind Sigma loop over d."""
    m = Model(d, n, dtype)
    Xs = FC.query_points(m.X, dtype)
    X64 = Xs.astype(np.float64)
    mean, cov = m.fk.predict_cov(Xs)
    assert cov.dtype == m.dtype and cov.shape == (len(Xs), len(Xs)) and np.array_equal(cov, cov.T)
    ref = PC.sigma_ref(X64, m.X64, m.amp, m.ell, m.nu, m.noise)
    fit = O.extend(m.X64, m.y64, m.noise, m.amp, m.ell, m.nu)
    lm, _, _ = O.predict(X64, m.X64, fit["alpha"], fit["k_inv"], m.amp, m.ell, m.nu)
    d_s = float(np.abs(cov.astype(np.float64) - ref).max()) / m.amp
    d_m = PRU.dev(mean, lm)
    m.release()
    print(f"FC cov {m.what}: Sigma {d_s:.2e}, mean {d_m:.2e} (bar {m.tol:g})")
    assert d_s <= m.tol and d_m <= m.tol, (d_s, d_m)


def _check_qei(fk, post, Xb, z, fmin, tol):
    """tests/test_gpu_qei.py::_check at jitter 0."""
    qei, grad, info = fk.qei(Xb, z, fmin)
    assert (info == 0).all(), info
    rq, rg = QR.qei_many(post, Xb.astype(np.float64), z.astype(np.float64), fmin)
    assert (rq > 0).all() and (np.abs(rg).max(axis=(1, 2)) > 0).all(), rq  # every batch improves: none is compared at 0 = 0
    dq = float(np.abs(qei - rq).max())
    assert dq <= tol * max(1.0, math.sqrt(post.amp)), (dq, qei, rq)
    worst = 0.0
    for b in range(len(Xb)):
        scale = max(1.0, float(np.abs(rg[b]).max()))
        dev = float(np.abs(grad[b].astype(np.float64) - rg[b]).max()) / scale
        worst = max(worst, dev)
        assert dev <= tol, (b, dev)
    return dq, worst


@pytest.mark.parametrize("d,n,dtype", _cases(FC.QUERY_CASES))
def test_qei(d, n, dtype):
    """hbegp_qei_* at (q, B, S) = (1, 3, 256) and (5, 3, 256): qei_batch_kernel's reverse pass (one wave per (a, eight k)) and
    its LDS carve-up behind q d doubles.  fmin comes from the restated draws (feature_count_cases.qei_fmin): every batch improves.
    f32: the seed search of tests/test_gpu_qei.py::test_device_matches_restatement_f32, started at the seed found on the CPU."""
    m = Model(d, n, dtype)
    post = QR.Posterior(m.X64, m.y64, m.amp, m.ell, m.nu, m.noise)
    f32 = m.dtype == np.float32
    worst = np.zeros(2)
    for q, B, S in FC.QEI_SHAPES:
        z = FC.qei_normals(q, S, dtype)
        z64 = z.astype(np.float64)
        for seed in range(FC.QEI_SEED32.get((d, n, q), 0) if f32 else 0, FC.QEI_SEED_CAP):
            Xb = FC.qei_batches(d, n, q, B, seed, dtype)
            fmin = FC.qei_fmin(np.stack([QR.draw_values(post, xb.astype(np.float64), z64).min(axis=1) for xb in Xb]))
            if not f32:
                break
            gaps = [QR.top_two_gap(post, xb.astype(np.float64), z64, fmin) for xb in Xb]
            if min(min(g) for g in gaps) > 1e-3 * math.sqrt(post.amp):
                break
        else:
            raise AssertionError(f"no seed keeps q={q} B={B} S={S} away from the kinks")
        worst = np.maximum(worst, _check_qei(m.fk, post, Xb, z, fmin, m.tol))
    m.release()
    print(f"FC qei {m.what}: qei {worst[0]:.2e}, grad {worst[1]:.2e} (bar {m.tol:g})")


def _path_points(m, d, seed, dtype, S=None):
    shape = (m, d) if S is None else (S, m, d)
    return np.random.default_rng(seed).uniform(-0.1, 1.1, shape).astype(dtype)


@pytest.mark.parametrize("d,n,nu,dtype", _cases(FC.PATH_CASES))
def test_paths(d, n, nu, dtype):
    """hbegp_paths_* with S = 5 paths of F = 512 features, with and without the noise draw, at shared (m = 9) and per-path
    (m = 2) points: paths_project_kernel stages d frequencies per feature, paths_eval_kernel takes eight gradient components
    per pass (two passes from d = 9, three from 17, five from 33, eight at 64)."""
    m = Model(d, n, dtype, nu=nu)
    S, F = FC.PATHS_S, FC.PATHS_F
    worst = np.zeros(2)
    for noise_draw in (True, False):
        rng = E.RNG(n + d + 3)
        om0, ph = gpr.draw_spectral(nu, F, d, rng)
        w = rng.standard_normal((S, F))
        eps = rng.standard_normal((S, n)) if noise_draw else None
        draws = [None if a is None else np.asarray(a, dtype=dtype) for a in (om0, ph, w, eps)]
        paths = m.fk.sample_paths(*draws)
        ref = PR.Paths(m.X, m.y, m.amp, m.ell, nu, m.noise, *draws)
        for x in (_path_points(9, d, 5, dtype), _path_points(2, d, 6, dtype, S=S)):
            f, df = paths.evaluate(x)
            rf, rdf = ref.evaluate(x)
            d_f, d_g = PRU.dev(f, rf), PRU.dev(df, rdf)
            for kb, sl in enumerate(FC.groups(d, 8)):  # per pass of eight components, on the scale of the whole gradient
                v = float(np.abs(df[..., sl] - rdf[..., sl]).max()) / max(1.0, float(np.abs(rdf).max()))
                assert v <= m.tol, f"{m.what} noise draw {noise_draw}: df components {sl.start}:{sl.stop} off by {v:.2e}"
            assert d_f <= m.tol and d_g <= m.tol, (m.what, noise_draw, x.ndim, d_f, d_g)
            worst = np.maximum(worst, [d_f, d_g])
        paths.release()
    m.release()
    print(f"FC paths {m.what}: f {worst[0]:.2e}, df {worst[1]:.2e} (max |omega0| {np.abs(om0).max():.3g}; bar {m.tol:g})")
