"""GPU: the phase clocks of the nine posterior-side calls (hbegp_debug_*_phases; csrc/hbegp.cpp: PhaseClock and the per-thread
record of each kind).

For every kind, on an f64 and an f32 model of n = 96, d = 2 at a fixed theta and m = 130 query rows (two row blocks) where the call
takes rows: an untimed call leaves every kind's stored phases as they were; a timed call returns the bits of the untimed one,
stores the documented number of phases (finite, >= 0, one of them > 0) and leaves the other kinds' alone;
hbegp_debug_X_phases(0, out) hands those values out and switches the timing off.  A timed predict_cov leaves the sampling phases
alone, and so does a timed leave-one-out call without a gradient."""
import numpy as np
import pytest

from hbetune_rs_amd import _lib, gpr

pytestmark = pytest.mark.gpu

N, D, M = 96, 2, 130
# kind -> (the symbol's middle, phases it stores)
KINDS = {"posterior": ("posterior", 4), "select": ("batch_select", 2), "kg": ("kg", 2), "nei": ("nei", 4), "sens": ("sens", 4),
         "ehvi": ("ehvi", 3), "qei": ("qei", 2), "loo": ("loo", 4), "paths": ("paths", 3)}
JITTER = 0.1  # far above what the f32 factor of Sigma needs: no call here may end NOT_PD


def _phases(kind, enable):
    """hbegp_debug_<kind>_phases(enable, out): the stored phases (the entries past the kind's count stay NaN)."""
    out = np.full(5, np.nan)
    assert getattr(_lib.load(), f"hbegp_debug_{KINDS[kind][0]}_phases")(int(enable), _lib.dptr(out)) == _lib.OK
    assert np.isnan(out[KINDS[kind][1]:]).all()  # nothing is written past the documented count
    return out[: KINDS[kind][1]].copy()


def _enable(kind):
    assert getattr(_lib.load(), f"hbegp_debug_{KINDS[kind][0]}_phases")(1, None) == _lib.OK


def _snapshot():
    """every kind's stored phases as bytes; leaves every kind's timing off"""
    return {k: _phases(k, 0).tobytes() for k in KINDS}


@pytest.fixture(scope="module", params=[np.float64, np.float32], ids=["f64", "f32"])
def setup(request):
    dtype = request.param
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (N, D))
    ys = [np.sin(3 * X).sum(axis=1) + 0.1 * rng.standard_normal(N), ((X - 0.6) ** 2).sum(axis=1) * 3 + 0.1 * rng.standard_normal(N)]
    # f32: a noise of the amplitude's size keeps cond(K) <= n + 1 (tests/test_gpu_posterior_cov.py)
    noise = 1e-2 if dtype == np.float64 else 1.0
    theta = np.log([noise * 1.3, 1.3, 0.4, 0.7])
    fks = [gpr.FittedKernel.extend(X.astype(dtype), y.astype(dtype), theta, nu=2.5) for y in ys]
    fk = fks[0]
    Xs = rng.uniform(-0.1, 1.1, (M, D)).astype(dtype)
    z = rng.standard_normal((3, M)).astype(dtype)
    zb = rng.standard_normal((3, 20)).astype(dtype)
    zq = rng.standard_normal((8, 2)).astype(dtype)
    A, B = rng.uniform(0, 1, (M // 2, D)).astype(dtype), rng.uniform(0, 1, (M // 2, D)).astype(dtype)
    omega0, phase = gpr.draw_spectral(2.5, 64, D, rng)
    w = rng.standard_normal((3, 64))
    fmin = float(fk.y_train.min())
    front = np.array([[float(f.y_train.min()), float(f.y_train.max())] for f in fks]).T  # two points: (min0, min1), (max0, max1)
    ref = front.max(axis=0) + 0.5

    def paths():
        p = fk.sample_paths(omega0, phase, w)
        out = p.evaluate(Xs)
        p.release()
        return out

    calls = {
        "posterior": lambda: fk.sample_posterior(Xs, z, jitter=JITTER),
        "select": lambda: fk.select_batch(Xs, 3, fmin),
        "kg": lambda: fk.knowledge_gradient(Xs, want_posterior=True),
        "nei": lambda: fk.noisy_ei(Xs[:20], Xs[20:], zb, jitter=JITTER, want_details=True),
        "sens": lambda: fk.sobol_indices(A, B, want_values=True),
        "ehvi": lambda: gpr.ehvi(fks, Xs, front, ref, want_grad=True, want_posterior=True),
        "qei": lambda: fk.qei(Xs.reshape(M // 2, 2, D), zq, fmin, jitter=JITTER),
        "loo": lambda: fk.loo(want_grad=True),
        "paths": paths,
    }
    # calls of a kind that its clock must NOT time
    untimed = {"posterior": lambda: fk.predict_cov(Xs, jitter=JITTER), "loo": lambda: fk.loo(want_grad=False)}
    yield calls, untimed
    for f in fks:
        f.release()


def _bits(out):
    return [np.asarray(a).tobytes() for a in out]


@pytest.mark.parametrize("kind", list(KINDS))
def test_phase_clock(setup, kind):
    calls, untimed = setup
    call = calls[kind]
    before = _snapshot()
    off = _bits(call())
    assert _snapshot() == before  # an untimed call stores nothing, for any kind
    _enable(kind)
    on = _bits(call())
    assert on == off  # timing changes no output bit
    ph = _phases(kind, 0)
    print(f"{kind}: {ph} ms")
    assert np.isfinite(ph).all() and (ph >= 0).all() and (ph > 0).any(), ph
    after = _snapshot()
    assert all(after[k] == before[k] for k in KINDS if k != kind)  # the other kinds' records are untouched
    assert after[kind] == ph.tobytes()
    assert _bits(call()) == off
    assert _phases(kind, 0).tobytes() == ph.tobytes()  # the read above switched the timing off: this call stored nothing
    if kind in untimed:
        _enable(kind)
        untimed[kind]()
        assert _phases(kind, 0).tobytes() == ph.tobytes()
