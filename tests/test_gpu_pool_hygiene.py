"""GPU: no result depends on what a block of the device pool held before it was handed out.

Every large device array of the engine comes from a pool that recycles blocks by exact size and clears only fresh ones, and
every entry point is bitwise reproducible.  So the check is exact: a *subject* -- one call through the Python wrappers, on a
problem and models it builds itself from fixed data -- must return the same bytes

  (a) with HBEGP_POOL_FRESH=1     every block a fresh, zeroed one: the reference (run twice: it has to repeat itself first),
  (b) with HBEGP_POOL_POISON=1    every block filled with the word 0x40490FDB: finite garbage in both element types,
  (c) with HBEGP_POOL_POISON=2    every block filled with the word 0x7FF80000: quiet NaNs in both element types,

and hbegp_debug_pool_poisoned must show that (b) and (c) poisoned at least the blocks the subject has to draw.  No tolerance
anywhere.  The second half runs the same subjects on dirt that is reachable without the switch: the work matrices of
evaluations that failed (NaN features, a singular K) and of models with huge or overflowing K^-1, released right before."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import feature_count_cases as FC
import sensitivity_ref as SR
from hbetune_rs_amd import _lib, gpr
from hbetune_rs_amd import estimator as E

pytestmark = pytest.mark.gpu

# (n, d, nu): the smallest sizes that reach each evaluation path -- np = 128: one launch in the LDS; 384: launches; 1024: eight
# blocks, the task queue (DAG_MIN_BLOCKS_FIT = 6)
CASES = [(100, 4, 2.5), (300, 5, 2.5), (300, 5, 0.5), (900, 8, 2.5)]
DTYPES = (np.float64, np.float32)
JITTER = 1e-4  # of the calls that factor Sigma at up to 900 candidates: positive definite in both element types
SWITCHES = ("HBEGP_POOL_FRESH", "HBEGP_POOL_POISON")


def _id(v):
    if isinstance(v, type):
        return np.dtype(v).name
    if isinstance(v, tuple):
        return "n%d-d%d-nu%s" % v
    return None


class _pool:
    """The pool's test switches for the length of a `with` block (the library reads them on every hand-out)."""

    def __init__(self, fresh=False, poison=0):
        self.want = {"HBEGP_POOL_FRESH": "1" if fresh else None, "HBEGP_POOL_POISON": str(poison) if poison else None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in SWITCHES}
        for k, v in self.want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _poisoned():
    blocks, nbytes = C.c_longlong(0), C.c_longlong(0)
    _lib.check(_lib.load().hbegp_debug_pool_poisoned(C.byref(blocks), C.byref(nbytes)))
    return blocks.value, nbytes.value


def _arrays(outs):
    return [np.array(o, copy=True) for o in outs]


def _difference(ref, got):
    """None when every output has the same bytes, else what differs first."""
    if len(ref) != len(got):
        return f"{len(got)} outputs instead of {len(ref)}"
    for i, (a, b) in enumerate(zip(ref, got)):
        if a.dtype != b.dtype or a.shape != b.shape:
            return f"output {i} is {b.dtype}{list(b.shape)} instead of {a.dtype}{list(a.shape)}"
        if a.tobytes() != b.tobytes():
            isf = a.dtype.kind == "f"
            bad = ~((a == b) | (np.isnan(a) & np.isnan(b))) if isf else a != b
            where = np.argwhere(np.atleast_1d(bad))[:4].tolist()
            return f"output {i} differs in {int(bad.sum())} of {a.size} entries ({int(np.isnan(b).sum()) if isf else 0} NaN), first at {where}"
    return None


def _run(subject):
    """The subject's outputs as arrays; a subject that raises (an evaluation that comes back NOT_PD, say) is its own output."""
    try:
        return _arrays(subject())
    except Exception as e:  # noqa: BLE001
        return [np.array(f"{type(e).__name__}: {e}")]


def _reference(subject):
    """(a): the outputs on fresh, zeroed blocks -- repeatable and, where they are floating point, finite."""
    with _pool(fresh=True):
        before = _poisoned()
        ref = _arrays(subject())
        again = _arrays(subject())
        assert _poisoned() == before  # the switch is off: no fill
    assert _difference(ref, again) is None, "not repeatable on fresh blocks: " + _difference(ref, again)
    for i, a in enumerate(ref):
        assert a.dtype.kind != "f" or np.isfinite(a).all(), f"output {i} of the reference is not finite"
    return ref


def _check(subject, min_blocks, min_bytes):
    """Runs (a) twice, (b), (c); `subject` takes no arguments and returns a list of arrays and numbers."""
    ref = _reference(subject)
    failed = []
    for mode, name in ((1, "finite poison"), (2, "NaN poison")):
        b0 = _poisoned()
        with _pool(poison=mode):
            got = _run(subject)
        b1 = _poisoned()
        assert b1[0] - b0[0] >= min_blocks and b1[1] - b0[1] >= min_bytes, (name, b0, b1, min_blocks, min_bytes)
        diff = _difference(ref, got)
        if diff:
            failed.append(f"{name}: {diff}")
    assert not failed, "; ".join(failed)


# ---- the data -------------------------------------------------------------------------------------------------------------------
def _inputs(case, dtype, k=0):
    """feature_count_cases.inputs; k > 0: another response on the same rows and reversed length scales (further models)."""
    n, d, nu = case
    X, y, theta = FC.inputs(d, n, dtype)
    if k:
        Xd = X.astype(np.float64)
        y = (np.cos((1.5 + 0.5 * k) * Xd + 0.7 * k).sum(axis=1) + ((Xd - 0.6) ** 2).sum(axis=1)).astype(dtype)
        theta = np.concatenate([theta[:2], theta[2:][::-1]])
    return X, y, theta


def _model(case, dtype, k=0):
    X, y, theta = _inputs(case, dtype, k)
    return gpr.FittedKernel.extend(X, y, theta, nu=case[2])


def _candidates(m, d, seed, dtype):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (m, d)).astype(dtype)


def _normals(S, m, seed, dtype):
    return np.random.default_rng(seed).standard_normal((S, m)).astype(dtype)


def _fit_box(theta, d):
    lo = np.concatenate([[math.exp(theta[0]) / 4, FC.AMP / 4], np.full(d, 0.1)])
    hi = np.concatenate([[math.exp(theta[0]) * 4, FC.AMP * 4], np.full(d, 3.0)])
    starts = np.log(lo) + (np.log(hi) - np.log(lo)) * np.random.default_rng(d).uniform(0, 1, (2, d + 2))
    return lo, hi, starts


def _npad(n):
    return (n + 127) // 128 * 128


def _mat_bytes(n, dtype):
    return _npad(n) ** 2 * np.dtype(dtype).itemsize


# ---- subjects on a problem: (case, dtype) -> list ----------------------------------------------------------------------------------
def _s_lml(case, dtype, n_slots=1, slot=0):
    X, y, theta = _inputs(case, dtype)
    prob = gpr.Problem(X, y, nu=case[2], n_slots=n_slots)
    lml, grad = prob.lml_with_gradient(theta, slot=slot)
    out = [lml, grad, *prob.results(slot=slot)]
    prob.close()
    return out


def _s_lml_slot2(case, dtype):
    return _s_lml(case, dtype, n_slots=3, slot=2)


def _s_loo_grad(case, dtype):
    X, y, theta = _inputs(case, dtype)
    prob = gpr.Problem(X, y, nu=case[2])
    loo, grad = prob.loo_with_gradient(theta)
    prob.close()
    return [loo, grad]


def _s_kmat(case, dtype):
    X, y, theta = _inputs(case, dtype)
    prob = gpr.Problem(X, y, nu=case[2])
    K = prob.kernel_matrix(theta)
    prob.close()
    return [K]


def _s_extend(case, dtype):
    fk = _model(case, dtype)
    out = [fk.lml, *fk.arrays()]
    fk.release()
    return out


def _s_extend_with(case, dtype):
    X, y, theta = _inputs(case, dtype)
    base = gpr.FittedKernel.extend(X[:256], y[:256], theta, nu=case[2])
    fk = base.extend_with(X, y)
    assert fk.incremental
    out = [fk.lml, *fk.arrays()]
    fk.release()
    base.release()
    return out


def _s_fit(case, dtype, by_loo=False):
    X, y, theta = _inputs(case, dtype)
    lo, hi, starts = _fit_box(theta, case[1])
    new = gpr.FittedKernel.new_by_loo if by_loo else gpr.FittedKernel.new
    fk = new(X, y, theta, lo, hi, starts, nu=case[2], maxeval=12)
    out = [fk.theta, fk.lml, *fk.arrays()]
    fk.release()
    return out


def _s_fit_loo(case, dtype):
    return _s_fit(case, dtype, by_loo=True)


def _s_model_loo(case, dtype):
    fk = _model(case, dtype)
    out = list(fk.loo(want_grad=True))
    fk.release()
    return out


# (subject, which n it runs at (None: all), blocks it must draw at least, work matrices of np^2 elements among them)
# a problem slot: W1, W2, two K^-1 buffers, the small slab, plus the features and targets; a model: K^-1, L^-1 and six small arrays
PROBLEM_SUBJECTS = [
    (_s_lml, None, 7, 4),
    (_s_lml_slot2, None, 17, 12),
    (_s_loo_grad, None, 7, 4),
    (_s_kmat, None, 7, 4),
    (_s_extend, None, 15, 6),
    (_s_extend_with, (300,), 15, 6),
    (_s_fit, (100, 300), 8, 2),
    (_s_fit_loo, (100,), 8, 2),
    (_s_model_loo, None, 15, 6),
]
PROBLEM_PARAMS = [pytest.param(s, c, mb, mm, id=f"{s.__name__[3:]}-{_id(c)}") for s, ns, mb, mm in PROBLEM_SUBJECTS for c in CASES
                  if ns is None or c[0] in ns]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("subject,case,min_blocks,min_mats", PROBLEM_PARAMS)
def test_problem_and_model_calls_ignore_what_their_blocks_held(subject, case, min_blocks, min_mats, dtype):
    _check(lambda: subject(case, dtype), min_blocks, min_mats * _mat_bytes(case[0], dtype))


# ---- subjects on a model: (fk, case, m, dtype) -> list; the model is built inside the run ------------------------------------------
def _q_predict(fk, case, m, dtype):
    return list(fk.predict(FC.query_points(fk.x_train, dtype)[:m]))


def _q_predict_grad(fk, case, m, dtype):
    return list(fk.predict_with_gradient(FC.query_points(fk.x_train, dtype)[:m]))


def _q_predict_cov(fk, case, m, dtype):
    return list(fk.predict_cov(_candidates(m, fk.d, 11 + m, dtype)))


def _q_sample_posterior(fk, case, m, dtype):
    return list(fk.sample_posterior(_candidates(m, fk.d, 12 + m, dtype), _normals(4, m, 13, dtype), jitter=JITTER))


def _q_select_batch(fk, case, m, dtype):
    return list(fk.select_batch(_candidates(m, fk.d, 14 + m, dtype), 4, float(fk.y_train.min())))


def _q_kg(fk, case, m, dtype):
    return list(fk.knowledge_gradient(_candidates(m, fk.d, 15 + m, dtype), n_candidates=min(m, 40), want_posterior=True))


def _q_noisy_ei(fk, case, m, dtype):
    base, cand = _candidates(m, fk.d, 16 + m, dtype), _candidates(16, fk.d, 17, dtype)
    return list(fk.noisy_ei(base, cand, _normals(8, m, 18, dtype), jitter=JITTER, want_details=True))


def _q_qei(fk, case, m, dtype):
    q = 10
    Xb = np.random.default_rng(19 + m).uniform(-0.1, 1.1, (m // q, q, fk.d)).astype(dtype)
    return list(fk.qei(Xb, _normals(32, q, 20, dtype), float(fk.y_train.min()) + 0.2, jitter=JITTER))


def _q_paths(fk, case, m, dtype):
    rng = E.RNG(21)
    om0, ph = gpr.draw_spectral(fk.nu, FC.PATHS_F, fk.d, rng)
    w, eps = rng.standard_normal((FC.PATHS_S, FC.PATHS_F)), rng.standard_normal((FC.PATHS_S, fk.n))
    paths = fk.sample_paths(*(np.asarray(a, dtype=dtype) for a in (om0, ph, w, eps)))
    out = list(paths.evaluate(_candidates(m, fk.d, 22 + m, dtype)))
    paths.release()
    return out


def _q_sensitivity(fk, case, m, dtype):
    A, B = SR.samples(fk.d, m, 23 + m, dtype)
    out = list(fk.sobol_indices(A, B, want_values=True))
    return out + list(fk.main_effects(A, np.linspace(0.0, 1.0, 9), want_base=True))


def _q_maximize_ei(fk, case, m, dtype):
    starts = np.random.default_rng(24 + m).uniform(0, 1, (m, fk.d)).astype(dtype)
    return list(fk.maximize_ei(starts, np.full(fk.d, -0.1), np.full(fk.d, 1.1), float(fk.y_train.min()), maxeval=8))


def _q_ehvi(fk, case, m, dtype):
    other = _model(case, dtype, k=1)
    fks = [fk, other]
    lo = np.array([float(f.y_train.min()) for f in fks])
    hi = np.array([float(f.y_train.max()) for f in fks])
    t = np.arange(6) / 6  # tests/test_gpu_ehvi.py::_front's convex front, without its extras
    front = np.stack([lo[0] + (hi[0] - lo[0]) * t, lo[1] + (hi[1] - lo[1]) * (1 - np.sqrt(t)) ** 2], axis=1)
    out = list(gpr.ehvi(fks, _candidates(m, fk.d, 25 + m, dtype), front, hi + 0.1 * (hi - lo), want_grad=True, want_posterior=True))
    other.release()
    return out


def _q_cei(fk, case, m, dtype):
    cons = [_model(case, dtype, k=1), _model(case, dtype, k=2)]
    limits = [float(np.median(c.y_train)) for c in cons]
    fmin = float(np.quantile(np.asarray(fk.y_train, dtype=np.float64), 0.2))
    out = list(gpr.constrained_ei(fk, cons, _candidates(m, fk.d, 26 + m, dtype), fmin, limits, want_grad=True, want_details=True))
    for c in cons:
        c.release()
    return out


def _on_model(query, case, m, dtype):
    fk = _model(case, dtype)
    out = query(fk, case, m, dtype)
    fk.release()
    return out


# with m = n the call's scratch matrices (mp == np) fall into the size class the model and the problem recycle
POSTERIOR = [_q_predict_cov, _q_sample_posterior, _q_select_batch, _q_kg, _q_noisy_ei, _q_qei, _q_paths, _q_sensitivity, _q_maximize_ei,
             _q_ehvi, _q_cei]
MODEL_PARAMS = [pytest.param(q, c, m, id=f"{q.__name__[3:]}-{_id(c)}-m{m}") for q in (_q_predict, _q_predict_grad) for c in CASES for m in FC.M_QUERY]
MODEL_PARAMS += [pytest.param(q, c, m, id=f"{q.__name__[3:]}-{_id(c)}-m{m}") for q in POSTERIOR for c in CASES for m in (70, c[0])]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("query,case,m", MODEL_PARAMS)
def test_posterior_calls_ignore_what_their_blocks_held(query, case, m, dtype):
    # at least the model itself: the problem of `extend` (7 blocks, 4 work matrices) and its own 8 (2 work matrices)
    _check(lambda: _on_model(query, case, m, dtype), 15, 6 * _mat_bytes(case[0], dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_kg_lines_in_a_pool_block_ignore_what_it_held(dtype):
    """m = 8193 candidates: 16384 padded lines, kept in a pool block that the candidates of one workgroup reuse (mc = 520 > 512
    workgroups: eight of them run a second candidate).  tests/test_gpu_kg.py::test_replay_past_the_lds_limit's model."""
    def subject():
        rng = np.random.default_rng(4)
        X = rng.uniform(0, 1, (300, 4))
        y = np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(300)
        theta = np.log(np.concatenate([[(1e-2 if dtype == np.float64 else 1.0) * 1.3, 1.3], np.linspace(0.3, 0.9, 4)]))
        fk = gpr.FittedKernel.extend(X.astype(dtype), y.astype(dtype), theta, nu=2.5)
        out = list(fk.knowledge_gradient(_candidates(8193, 4, 6, dtype), n_candidates=520))
        fk.release()
        return out

    mp = _npad(8193)
    _check(subject, 16, mp * mp * np.dtype(dtype).itemsize)


# ---- dirt that is reachable without the switch ------------------------------------------------------------------------------------
DIRT_CASES = [(300, 5, 2.5), (900, 8, 2.5)]  # np = 384, 1024


def _d_lml(case, dtype):
    return _s_lml(case, dtype)


def _d_extend(case, dtype):
    return _s_extend(case, dtype)


def _d_predict(case, dtype):
    return _on_model(_q_predict, case, 70, dtype)


def _d_predict_cov(case, dtype):
    return _on_model(_q_predict_cov, case, case[0], dtype)


def _d_sample_posterior(case, dtype):
    return _on_model(_q_sample_posterior, case, case[0], dtype)


def _d_noisy_ei(case, dtype):
    return _on_model(_q_noisy_ei, case, case[0], dtype)


DIRT_SUBJECTS = [_d_lml, _d_extend, _d_predict, _d_predict_cov, _d_sample_posterior, _d_noisy_ei]


def _failed_evaluations(case, dtype):
    """Three problems of three slots whose every evaluation fails -- a NaN feature in row 0, one in row n - 1, 100 copies of one
    row at noise 1e-300 (tests/test_gpu_dag.py::test_task_queue_drains_when_not_positive_definite) -- closed right after: their
    15 work matrices each go back to the pool as the failure left them."""
    n, d, nu = case
    X, y, theta = _inputs(case, dtype)
    singular = theta.copy()
    singular[0] = math.log(1e-300)
    first, last, copies = X.copy(), X.copy(), X.copy()
    first[0, 1] = np.nan
    last[n - 1, d - 1] = np.nan
    copies[n - 100:] = X[10]
    for Xbad, th in ((first, theta), (last, theta), (copies, singular)):
        prob = gpr.Problem(Xbad, y, nu=nu, n_slots=3)
        for slot in range(3):
            assert prob.lml_with_gradient(th, slot=slot) is None
        prob.close()


def _foreign_owners(case, dtype):
    """A model whose K^-1 is full, symmetric and ~1e6 (noise 1e-6 c), and in f64 one whose parameters overflow K^-1 (amplitude
    1e-300, noise 1e-309: entries ~1e309), released right before.  Whether `extend` accepts the latter: DESIGN section 23."""
    X, y, theta = _inputs(case, dtype)
    tiny = theta.copy()
    tiny[0] = theta[1] + math.log(1e-6)
    try:  # (should the factor fail in f32 at this noise: the attempt's work matrices go back all the same)
        gpr.FittedKernel.extend(X, y, tiny, nu=case[2]).release()
    except gpr.HbegpError:
        pass
    if np.dtype(dtype) == np.float64:
        over = theta.copy()
        over[0], over[1] = math.log(1e-309), math.log(1e-300)
        try:
            gpr.FittedKernel.extend(X, y, over, nu=case[2]).release()
        except gpr.HbegpError:
            pass


@pytest.fixture(scope="module")
def fresh_reference():
    """The HBEGP_POOL_FRESH=1 outputs of the dirt subjects, computed once per (subject, case, dtype) and left unchanged."""
    cache = {}

    def get(subject, case, dtype):
        key = (subject.__name__, case, np.dtype(dtype).name)
        if key not in cache:
            cache[key] = _reference(lambda: subject(case, dtype))
        return cache[key]

    return get


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("case", DIRT_CASES, ids=_id)
@pytest.mark.parametrize("dirt", [_failed_evaluations, _foreign_owners], ids=lambda f: f.__name__[1:])
def test_good_calls_after_dirty_owners(dirt, case, dtype, fresh_reference):
    failed = []
    for subject in DIRT_SUBJECTS:
        ref = fresh_reference(subject, case, dtype)
        with _pool():  # recycling, no poison: the blocks come back as the owners above left them
            dirt(case, dtype)
            got = _run(lambda: subject(case, dtype))
        diff = _difference(ref, got)
        if diff:
            failed.append(f"{subject.__name__[3:]} after {dirt.__name__[1:]}: {diff}")
    assert not failed, "; ".join(failed)
