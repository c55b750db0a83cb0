"""The case table of tests/test_gpu_general_eval.py and of its input guard tests/test_general_eval_cpu.py (DESIGN.md section
32): the (d, n, nu) at which the general evaluation path -- kmat_kernel, the factorisation, gradtrace_kernel with one of its two
finalisers -- is run past 128 rows, the fits over it, and the reference of each case.  Both modules take them from here, so the
guard judges the inputs the device is judged on.

The feature counts are feature_count_cases.D_CLASSES (both sides of GT_CHUNK = 8 and of every later chunk edge the grid has, and
the two ends of the ABI's range); the data, theta and noise regimes are feature_count_cases.inputs'.  The row counts:

  320   np = 384: a multiple of 64 but not of 128, the fast branches of both kernels end exactly at n
  257   np = 384: one live row in the last 128-block
  192   np = 256: the last row of 64x64 tiles is all padding
  1921  np = 2048, the smallest n with 528 > FUSE_GRAD_MAX_TILES tiles: finalize_grad_kernel runs whatever HBEGP_HOSTIO says, and
        the last live tile row holds one row"""
import functools
import math

import numpy as np

import feature_count_cases as FC
from oracle import gpr_oracle as O

D_CLASSES = FC.D_CLASSES
NUS = FC.NUS
DTYPES = FC.DTYPES
GROUP = FC.GROUP_LOO  # GT_CHUNK: length-scale parameters per register pass of gradtrace_tile
N_ORACLE_MAX = 320    # beyond it the oracle's [n, n, p] derivative array is too large (2 GB at (64, 1921)): lean_reference
N_BIG = 1921
FUSE_GRAD_MAX_TILES = 512  # enqueue_eval: fuse_grad = hostio && (np / 64) * (np / 64 + 1) / 2 <= 512
ALL_ORDERS_AT = ((9, 320), (64, 257))
PADDING_CASES = ((9, 192), (9, 257), (64, N_BIG))
HOSTIO_CASES = ((9, 320), (64, 320))
TWO_PHASE_CASE = (17, 257)
FIT_CASES = ((33, 257), (64, 257))
COND_MAX = 2.5e4      # DESIGN.md section 17's figure: cond(K) of every case with n <= 320, and of every fit box's worst corner
COND_MAX_BIG = 1e5    # n = 1921
GUARD_BARS = 20       # a gradient group's largest reference entry, in bars of the element type
KMAT_BAR32_CPU = 4    # |K restated in f32 - K in f64 on the rounded inputs|, in eps32 c
KMAT_BAR32_GPU = 8    # the same for the device: 4 more for its expf and sqrtf, each documented at about 1 ulp


def nu_of(d):
    return FC.nu_of(d)


def _eval_cases():
    cases = [(d, 320, nu_of(d)) for d in D_CLASSES]
    cases += [(d, 257, nu_of(d)) for d in (9, 17, 64)]
    cases += [(d, 192, nu_of(d)) for d in (9, 33)]
    cases += [(d, N_BIG, nu_of(d)) for d in (9, 64)]
    cases += [(d, n, nu) for d, n in ALL_ORDERS_AT for nu in NUS if nu != nu_of(d)]
    return cases


EVAL_CASES = _eval_cases()  # (d, n, nu), each in both element types


def tol_of(dtype):
    return FC.tol_of(dtype)


def tiles(n):
    """64x64 tiles of the lower triangle of the padded matrix: the grid of kmat_kernel and of gradtrace_kernel."""
    nt = (n + 127) // 128 * 128 // 64
    return nt * (nt + 1) // 2


# the data seed is feature_count_cases' (n + d), except where that draw fails the input guard (tests/test_general_eval_cpu.py);
# each entry with its reason
DATA_SEED = {}


def inputs(d, n, dtype):
    """(X, y, theta): feature_count_cases.inputs' recipe -- noise 1e-2 c in f64, c in f32."""
    return FC.inputs(d, n, dtype, seed=DATA_SEED.get((d, n)))


def rounded_inputs(d, n, dtype):
    """(X, y, theta) with X and y rounded to the element type and widened: what the device sees, as the references take it."""
    X, y, theta = inputs(d, n, dtype)
    return X.astype(np.float64), y.astype(np.float64), theta


def grad_groups(d):
    """The lml gradient by what gradtrace_tile publishes together: the noise / amplitude lead (with the first chunk, at `my`),
    then each chunk of eight length scales (at my + 2 + kc)."""
    return [("noise, amplitude", slice(0, 2))] + [(f"ell[{s.start}:{s.stop}]", slice(2 + s.start, 2 + s.stop))
                                                 for s in FC.groups(d, GROUP)]


def case_id(d, n, nu, dtype):
    return f"d{d}-n{n}-nu{nu}-{np.dtype(dtype).name}"


# ------------------------------------------------------------------------------------------------------------ the references
def _gr(dsum, kernel, nu):
    """gr(r) of dK_matern / dlog(ell_k) = gr * d_k, per order as oracle/gpr_oracle.py::matern_theta_grad forms it (fp64)."""
    if nu == 0.5:
        with np.errstate(divide="ignore", invalid="ignore"):
            g = kernel / np.sqrt(dsum)  # :103-104
        g[~np.isfinite(g)] = 0          # :105-109
        return g
    if nu == 1.5:
        return np.exp(-np.sqrt(dsum * 3.0)) * 3.0  # :114-117
    if nu == 2.5:
        tmp = np.sqrt(dsum * 5.0)
        return np.exp(-tmp) * (tmp + 1.0) * (5.0 / 3.0)  # :120-130
    assert math.isinf(nu)
    return np.exp(-0.5 * dsum)


def matern_by_rows(x, length_scale, nu, rows=128):
    """oracle.gpr_oracle.matern_kernel(x, x, ..), 128 rows at a time: the same entries (its arithmetic is per entry) without
    its [n, n, d] array of differences, 1.9 GB at (64, 1921)."""
    return np.concatenate([O.matern_kernel(x[a:a + rows], x, length_scale, nu) for a in range(0, len(x), rows)], axis=0)


def lean_reference(x, y, noise, amplitude, length_scale, nu):
    """oracle.gpr_oracle.lml_with_gradient in fp64 without the [n, n, p] derivative array: with W = alpha alpha^T - K^-1,
    g_k = 1/2 sum W o (c gr(r)) o d_k, one n x n matrix d_k per parameter.  The same LAPACK calls for everything else.
    tests/test_general_eval_cpu.py holds it to 1e-12 of the oracle on every case the oracle can take."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = len(y)
    ell = np.asarray(length_scale, np.float64)
    kernel = matern_by_rows(x, ell, nu)
    K = amplitude * kernel
    K[np.diag_indices(n)] += noise
    chol, info = O._potrf(K)
    if info != 0:
        return None
    alpha = O._potrs(chol, y)
    lml = -0.5 * float(y.dot(alpha)) - float(np.log(np.diag(chol)).sum()) - n / 2.0 * math.log(2.0 * math.pi)
    k_inv = O._potri(chol)
    W = np.outer(alpha, alpha) - k_inv
    scales_sq = ell * ell

    def d_k(k, out):  # the oracle's d[:, :, k] = diff^2 / ell_k^2, in place
        np.subtract.outer(x[:, k], x[:, k], out=out)
        np.square(out, out=out)
        out /= scales_sq[k]
        return out

    dsum, D = np.zeros((n, n)), np.empty((n, n))
    for k in range(x.shape[1]):  # summed over the features in turn, as the oracle does
        dsum += d_k(k, D)
    Wg = W * (amplitude * _gr(dsum, kernel, nu))
    grads = [0.5 * noise * float(np.trace(W)), 0.5 * float((W * (amplitude * kernel)).sum())]
    for k in range(x.shape[1]):
        grads.append(0.5 * float(np.vdot(Wg, d_k(k, D))))
    return dict(lml=lml, grad=np.array(grads), alpha=alpha, chol=chol, k_inv=k_inv, kernel_matrix=K)


def reference_at(x, y, theta, nu, lo=None, hi=None):
    """The fp64 reference at a log-space theta (clamped into [lo, hi] as fit.rs:94-96 does): the oracle up to N_ORACLE_MAX rows,
    its lean restatement beyond.  Adds ldiag = diag(L)."""
    v = np.exp(np.asarray(theta, np.float64))
    if lo is not None:
        v[1:] = np.minimum(np.maximum(v[1:], lo[1:]), hi[1:])
    fn = O.lml_with_gradient if len(y) <= N_ORACLE_MAX else lean_reference
    ref = fn(np.asarray(x, np.float64), np.asarray(y, np.float64), v[0], v[1], v[2:], nu)
    assert ref is not None, "the reference's factorisation failed"
    ref["ldiag"] = np.diag(ref["chol"]).copy()
    return ref


@functools.lru_cache(maxsize=None)
def reference(d, n, nu, dtype_name):
    """The case's reference on the inputs the device sees.  Cached per case and shared: callers leave it unchanged."""
    X, y, theta = rounded_inputs(d, n, np.dtype(dtype_name))
    return reference_at(X, y, theta, nu)


def cond(K):
    w = np.linalg.eigvalsh(np.asarray(K, np.float64))
    return float(w[-1] / w[0])


# ------------------------------------------------------------------------- kmat_kernel's arithmetic, in the element type
def kmat_restated(X, theta, nu, dtype, oracle_poly=False):
    """K as kmat_kernel forms it, every operation rounded to the element type: x / ell with ell = T(exp(theta)), the squared
    differences summed in feature order, sqrt, matern_map's expressions, amp * k, the noise added last on the diagonal.  (NumPy
    has no fused multiply-add: the kernel's `acc += df * df` and matern_map's fma for nu = 5/2 are written as two roundings.)

    matern_map's expressions are the oracle's for three orders.  For nu = 5/2 it groups the polynomial as k^2 (1/3) + (1 + k)
    where the oracle (matern_kernel.rs:75) has (1 + k) + k^2 / 3: other roundings, the same number of them.  oracle_poly takes
    the oracle's grouping, so that the guard can show that nothing else differs."""
    T = np.dtype(dtype).type
    v = np.exp(np.asarray(theta, np.float64))
    noise, amp, ell = T(v[0]), T(v[1]), v[2:].astype(T)
    xs = np.asarray(X, dtype=T) / ell[None, :]
    n = len(xs)
    acc = np.zeros((n, n), dtype=T)
    for k in range(xs.shape[1]):
        df = xs[:, None, k] - xs[None, :, k]
        acc += df * df
    r = np.sqrt(acc)
    if math.isinf(nu):
        km = np.exp(T(-0.5) * r * r)
    elif nu == 0.5:
        km = np.exp(-r)
    elif nu == 1.5:
        k = r * T(1.7320508075688772)
        km = (k + T(1)) * np.exp(-k)
    else:
        k = r * T(2.23606797749979)
        poly = (T(1) + k + k * k / T(3)) if oracle_poly else (k * k * T(1.0 / 3.0) + (T(1) + k))
        km = poly * np.exp(-k)
    K = amp * km
    K[np.diag_indices(n)] += noise
    assert K.dtype == np.dtype(dtype)
    return K


def kmat_reference(X, theta, nu):
    """The fp64 oracle's matrix on X as given (rounded inputs widened): c Matern + s2 I."""
    v = np.exp(np.asarray(theta, np.float64))
    X = np.asarray(X, np.float64)
    K = v[1] * matern_by_rows(X, v[2:], nu)  # product_kernel.rs:37
    K[np.diag_indices(len(X))] += v[0]       # lml.rs:44
    return K


# ------------------------------------------------------------------------------------------------------------------- the fits
FIT_MAXEVAL = 10
TWO_PHASE_MAXEVAL = 40


def fit_box(theta):
    """(lo, hi) around exp(theta), tight enough that every evaluation of a run can be replayed on LAPACK: noise in [0.5, 4] x
    the case's own, amplitude in [0.6, 1.5] x, every length scale in [0.7, 1.25] x."""
    v = np.exp(theta)
    lo = np.concatenate([[0.5 * v[0], 0.6 * v[1]], 0.7 * v[2:]])
    hi = np.concatenate([[4.0 * v[0], 1.5 * v[1]], 1.25 * v[2:]])
    return lo, hi


def worst_corner(theta):
    """The corner of fit_box where cond(K) is largest: lowest noise, largest amplitude, longest length scales."""
    lo, hi = fit_box(theta)
    return np.log(np.concatenate([[lo[0]], hi[1:]]))


def fit_starts(d, n, theta, k):
    """k start points uniform in the log box (the first run starts at theta)."""
    lo, hi = (np.log(b) for b in fit_box(theta))
    u = np.random.default_rng(9000 + 100 * d + n).uniform(0, 1, (k, d + 2))
    return lo + (hi - lo) * u


# Inside the tight box the lml is close to monotone along most search directions, and a run rarely sees its line search reject a
# trial: of 160 uniform draws of the start point, with the oracle as the objective of the library's own state machine
# (tests/test_general_eval_cpu.py::test_the_two_phase_starts_have_rejected_trials replays it), 27 lead to one in the f64 regime and 2
# in the f32 regime.  The two draws below are the ones with the most: 3 rejected trials that are no new best of their run in f64
# (none in f32), and 2 in f32 (none in f64).  The first is theta0, the second the one start.
TWO_PHASE_SEEDS = (1114, 1029)


def two_phase_starts(d, n, theta):
    """(theta0, starts[1, p]) of the two-phase fit: uniform draws in the log box, well away from the case's theta."""
    assert (d, n) == TWO_PHASE_CASE
    lo, hi = (np.log(b) for b in fit_box(theta))
    pts = [lo + (hi - lo) * np.random.default_rng(s).uniform(0, 1, d + 2) for s in TWO_PHASE_SEEDS]
    return pts[0], pts[1][None, :]
