"""GPU: the sample-path entry points at the path, feature and point counts that split them ("The
size-dependent splits under test"; the cases and the rules: tests/paths_size_cases.py; its guard: tests/test_paths_sizes_cpu.py).

Every case, in both element types, with the same m points for every path and with per-path points:

  (a) f and df at all points of the call against the fp64 restatement (tests/paths_ref.py, its matrix-product form), at the bars
      of tests/test_gpu_paths.py: parity_rules.TOL64 = 1e-8 / TOL32 = 1e-4, relative to max(1, scale of the reference).  The
      per-path points of path s are pool[idx[s]], a random draw per (path, point) from the shared call's points: the device is
      handed S m unrelated rows, the reference is the pool's, gathered (at S = 1000, F = 16384 the cosines of 130000 distinct points
      would take minutes on a CPU).
  (b) every call of several blocks bit for bit against calls on the same handle that are one block each (the library's query says
      so, the test asserts it), cut at offsets that are no block edges; f without the gradient equals f with it; and a per-path
      value equals the shared call's value of the same (path, point), as the header promises.
  (c) the call really had the blocks, and the handle's projection the chunks, of the table (through the queries).

The minimiser on part-cap's handle from 60 starts per path: its first round is an [S][60] evaluation of 56 + 4 points.  The
rows-per-path subject on poisoned pool blocks (tests/test_gpu_pool_hygiene.py): every block after the first reuses the handle's
grown scratch.

S = 1024 (rows-shared, cap4) and F = 16384 (part-cap) are accepted here; that 1025 and 16385 are refused, with their messages, is
tests/test_paths_cpu.py::test_bad_arguments_are_refused_before_any_device_call."""
import ctypes as C

import numpy as np
import pytest

import paths_ref as PR
import paths_size_cases as PC
import test_gpu_paths as TP
import test_gpu_pool_hygiene as PH
from hbetune_rs_amd import _lib

pytestmark = pytest.mark.gpu

PARAMS = [pytest.param(c, t, id=PC.case_id(c, t)) for t in PC.DTYPES for c in PC.CASES]


def _seed(case):
    return 100 + 10 * PC.CASES.index(case)


def _build(case, dtype):
    """(model, handle, X, y, draws): tests/test_gpu_paths.py's data recipe, noise regime and draws at the case's sizes."""
    fk, X, y = TP._model(case.n, case.nu, dtype, seed=_seed(case), d=case.d)
    draws = TP._draws(fk, case.F, case.S, seed=_seed(case) + 1)
    return fk, fk.sample_paths(*draws), X, y, draws


class _Subject:
    """A case's model and handle, the points of its two calls and the restatement's values at them: built once, left unchanged."""

    def __init__(self, case, dtype):
        self.case, self.dtype = case, np.dtype(dtype)
        self.fk, self.paths, X, y, draws = _build(case, dtype)
        self.pool = TP._points(case.m, _seed(case) + 2, dtype, d=case.d)                                  # the shared call's points
        self.idx = np.random.default_rng(_seed(case) + 3).integers(0, case.m, (case.S, case.m))  # path s at pool[idx[s]]
        self.f_ref, self.df_ref = TP._ref(self.fk, X, y, draws).evaluate_by_matmul(self.pool)

    def release(self):
        self.paths.release()
        self.fk.release()


@pytest.fixture(scope="module")
def subject():
    """part-cap's subjects are kept for the minimiser's test (a handle of 131 MB of weights and a second of reference each); every
    other one lives for its own test."""
    kept = {}

    def get(case, dtype):
        key = PC.case_id(case, dtype)
        if key in kept:
            return kept[key], False
        s = _Subject(case, dtype)
        if case is PC.ROUND_CASE:
            kept[key] = s
        return s, case is not PC.ROUND_CASE

    yield get
    for s in kept.values():
        s.release()


def _info(paths):
    n, d, F, S, is32 = (C.c_int() for _ in range(5))
    _lib.check(_lib.load().hbegp_paths_info(paths._h, C.byref(n), C.byref(d), C.byref(F), C.byref(S), C.byref(is32)))
    return n.value, d.value, F.value, S.value, bool(is32.value)


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), (what, int((got != want).sum()), got.size)


@pytest.mark.parametrize("case,dtype", PARAMS)
def test_a_case_at_every_point_of_its_calls(case, dtype, subject):
    s, mine = subject(case, dtype)
    try:
        _check_case(s, case, dtype)
    finally:
        if mine:
            s.release()


def _check_case(s, case, dtype):
    paths, tol, m, mb = s.paths, TP._tol(dtype), case.m, case.blocks[0]
    # (c) the handle has the table's sizes, so its calls have the table's blocks and its projection the table's chunks
    assert _info(paths) == (case.n, case.d, case.F, case.S, np.dtype(dtype) == np.float32)
    assert PC.blocks_of(case) == case.blocks and PC.project_chunks(case.F, case.n, case.S) == (case.cap, case.nch, case.fch)
    xs, xp = s.pool, s.pool[s.idx]
    f, df = paths.evaluate(xs)
    fp, dfp = paths.evaluate(xp)
    assert f.shape == (case.S, m) and df.shape == (case.S, m, case.d) and fp.shape == f.shape and dfp.shape == df.shape
    for a in (f, df, fp, dfp):
        assert np.isfinite(a).all()
    # (a) the restatement at all points of both calls
    rfp, rdfp = PR.gather(s.f_ref, s.df_ref, s.idx)
    devs = [TP._devs(f, s.f_ref), TP._devs(df, s.df_ref), TP._devs(fp, rfp), TP._devs(dfp, rdfp)]
    print(f"{PC.case_id(case, dtype)}: blocks {case.blocks}, chunks {case.nch} x {case.fch}: shared f off by {devs[0]:.2e}, df by "
          f"{devs[1]:.2e}; per path f by {devs[2]:.2e}, df by {devs[3]:.2e} (scales {np.abs(s.f_ref).max():.3g}, "
          f"{np.abs(s.df_ref).max():.3g}; bar {tol:g})")
    for what, v in zip(("shared f", "shared df", "per-path f", "per-path df"), devs):
        assert v <= tol, (what, v)
    # (b) the same (path, point) has the same bits in both calls, and f does not depend on whether the gradient is asked for
    gf, gdf = PR.gather(f, df, s.idx)
    _same(fp, gf, "per path vs shared: f")
    _same(dfp, gdf, "per path vs shared: df")
    f0, none = paths.evaluate(xs, want_grad=False)
    fp0, nonep = paths.evaluate(xp, want_grad=False)
    assert none is None and nonep is None
    _same(f0, f, "shared f without the gradient")
    _same(fp0, fp, "per-path f without the gradient")
    if len(case.blocks) == 1:
        return
    # ... and every piece of a call of several blocks, as a call of one block
    for a, b in PC.slices(m, mb):
        assert PC.blocks_of(case, b - a) == (b - a,) and (a == 0 or a % mb != 0)
        piece = np.ascontiguousarray(xp[:, a:b])
        fa, dfa = paths.evaluate(xs[a:b])
        _same(fa, f[:, a:b], f"shared f [{a}, {b})")
        _same(dfa, df[:, a:b], f"shared df [{a}, {b})")
        _same(paths.evaluate(xs[a:b], want_grad=False)[0], f[:, a:b], f"shared f without the gradient [{a}, {b})")
        fa, dfa = paths.evaluate(piece)
        _same(fa, fp[:, a:b], f"per-path f [{a}, {b})")
        _same(dfa, dfp[:, a:b], f"per-path df [{a}, {b})")
        _same(paths.evaluate(piece, want_grad=False)[0], fp[:, a:b], f"per-path f without the gradient [{a}, {b})")


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=lambda t: np.dtype(t).name)
def test_a_round_of_the_minimiser_spans_blocks(dtype, subject):
    """part-cap's handle, R = 60 starts per path: the first lockstep round evaluates [S][60] per-path points in blocks of 56 + 4.
    maxeval = 1 is that round alone: per path exactly the best of its starts (ties to the first), the value bit for bit
    `evaluate`'s there.  maxeval = 4 keeps tests/test_gpu_paths.py::test_minimiser_contract's contract."""
    case, Rn = PC.ROUND_CASE, PC.ROUND_STARTS
    s, mine = subject(case, dtype)
    assert not mine
    paths, S, d = s.paths, case.S, case.d
    assert PC.blocks_of(case, Rn) == PC.ROUND_BLOCKS
    lo, hi = np.zeros(d), np.ones(d)
    starts = np.random.default_rng(77).uniform(0, 1, (S, Rn, d)).astype(dtype)
    f_at, df_at = paths.evaluate(starts)
    for a, b in PC.slices(Rn, PC.ROUND_BLOCKS[0]):  # the values at the starts, from calls of one block each
        assert PC.blocks_of(case, b - a) == (b - a,)
        fa, dfa = paths.evaluate(np.ascontiguousarray(starts[:, a:b]))
        _same(fa, f_at[:, a:b], f"f at the starts [{a}, {b})")
        _same(dfa, df_at[:, a:b], f"df at the starts [{a}, {b})")
    f_starts = f_at.astype(np.float64)
    assert np.isfinite(f_starts).all()
    x1, fb1, nev1 = paths.minimize(starts, lo, hi, maxeval=1)
    best = f_starts.argmin(axis=1)  # the first of equal values
    _same(x1, starts[np.arange(S), best], "x_best of the first round")
    _same(fb1, f_starts.min(axis=1), "f_best of the first round")
    assert (nev1 == Rn).all()
    x4, fb4, nev4 = paths.minimize(starts, lo, hi, maxeval=4)
    assert ((x4 >= 0) & (x4 <= 1)).all() and (nev4 >= Rn).all() and (nev4 <= 4 * Rn).all()
    at = paths.evaluate(x4[:, None, :], want_grad=False)[0][:, 0]
    _same(at.astype(np.float64), fb4, "f_best against evaluate at x_best")
    assert (fb4[:, None] <= f_starts).all()
    print(f"{np.dtype(dtype).name}: {int((fb4 < f_starts.min(axis=1)).sum())} of {S} paths below their best start after 4 evaluations per run; "
          f"evaluations {int(nev4.sum())}")
    assert (fb4 < f_starts.min(axis=1)).any()  # it moved


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=lambda t: np.dtype(t).name)
def test_later_blocks_ignore_what_the_scratch_held(dtype):
    """rows-per-path, three blocks of per-path points with gradients, on fresh, finitely poisoned and NaN-poisoned pool blocks: the
    handle's scratch (the partial sums among it) is drawn once and reused by the second and third block."""
    case = PC.HYGIENE_CASE
    assert len(case.blocks) == 3
    x = TP._points(case.m, _seed(case) + 4, dtype, d=case.d, S=case.S)

    def run():
        fk, paths, _, _, _ = _build(case, dtype)
        out = list(paths.evaluate(x))
        paths.release()
        fk.release()
        return out

    # the model (15 blocks, 6 work matrices: tests/test_gpu_pool_hygiene.py), the handle's 4 arrays and its 4 of scratch, among them
    # a block's partial sums: however they are chunked, at least one double per (path, point, component of f and df)
    part = 8 * case.S * case.blocks[0] * (case.d + 1)
    PH._check(run, 15 + 8, 6 * PH._mat_bytes(case.n, dtype) + part)
