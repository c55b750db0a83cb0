"""NumPy restatement of the knowledge gradient over a candidate set (include/hbegp.h, hbegp_knowledge_gradient_*), shared by the
CPU and GPU tests.

From the posterior mean mu and Sigma (predict_cov's matrix at jitter 0) and the model's noise s2, for candidate j:
r = Sigma[:, j], r_j = Sigma_jj - 1e-5, d_j = max(r_j, 0) + s2, st = r / sqrt(d_j); the mean after one noisy sample at row j is
mu + st Z, and kg_j = min mu - E[min_i (mu_i + st_i Z)] by Algorithm 1 of Frazier, Powell, Dayanik (2009) on the lines
a = -mu, b = -st: sort by (b, a), keep the largest a of equal slopes, build the upper envelope, sum (b_{k+1} - b_k) f(-|c_k|)."""
import math

import numpy as np
from scipy.special import erfc

MIN_NOISE = 1e-5


def sigma_tilde(sigma, j, s2):
    """(st, sqrt(d_j)): the change of the posterior mean per unit Z of a noisy sample at row j."""
    r = np.array(np.asarray(sigma, np.float64)[j], np.float64)
    r[j] = r[j] - MIN_NOISE  # the latent variance: the sample's own noise is s2
    sd = math.sqrt(max(r[j], 0.0) + s2)
    return r / sd, sd


def tail(ac):
    """f(-|c|) = phi(c) - |c| Phi(-|c|), 0 beyond 38 (both terms are below 1e-314 there; an infinite breakpoint too)."""
    ac = np.asarray(ac, np.float64)
    near = ac < 38.0
    x = np.where(near, ac, 0.0)
    f = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi) - x * (0.5 * erfc(x / math.sqrt(2.0)))
    return np.where(near, np.maximum(f, 0.0), 0.0)


def envelope(a, b):
    """The lines of the upper envelope of a_i + b_i z, left to right: (a[k], b[k]) with strictly increasing slopes and strictly
    increasing breakpoints."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    order = np.lexsort((a, b))  # by b, then a
    a, b = a[order].tolist(), b[order].tolist()  # Python floats: IEEE doubles, and the loop below is the hot part of the tests
    m = len(a)
    sa, sb, sc = [], [], []  # the stack; sc[k]: the breakpoint at which line k begins
    for i in range(m):
        if i + 1 < m and b[i + 1] == b[i]:
            continue  # equal slopes: the last of the run has the largest a
        c = -math.inf
        while sa:
            c = (sa[-1] - a[i]) / (b[i] - sb[-1])  # slopes on the stack are distinct and ascending: never a zero divisor
            if len(sa) == 1 or c > sc[-1]:
                break
            sa.pop(), sb.pop(), sc.pop()
        sa.append(a[i]), sb.append(b[i]), sc.append(c)
    return np.array(sa), np.array(sb)


def h(a, b):
    """E[max_i (a_i + b_i Z)] - max_i a_i for Z ~ N(0, 1); exactly 0 when one line survives."""
    ea, eb = envelope(a, b)
    if len(ea) < 2:
        return 0.0
    with np.errstate(all="ignore"):
        c = (ea[:-1] - ea[1:]) / (eb[1:] - eb[:-1])
    return float(np.sum((eb[1:] - eb[:-1]) * tail(np.abs(c))))


def kg(mu, sigma, s2, mc=None):
    """kg[mc] of the first mc rows (all by default), the minimum over every row."""
    mu = np.asarray(mu, np.float64)
    m = len(mu)
    mc = m if mc is None else mc
    out = np.zeros(mc)
    for j in range(mc):
        st, _ = sigma_tilde(sigma, j, s2)
        out[j] = h(-mu, -st)
    return out


def argmax_last(v):
    return len(v) - 1 - int(np.argmax(np.asarray(v)[::-1]))


def expected_min_quadrature(mu, st, step, zmax=12.0):
    """E[min_i (mu_i + st_i Z)] by the trapezoid rule on [-zmax, zmax] (the tail beyond 12 sigma is below 1e-30)."""
    n = int(round(2 * zmax / step))
    z = np.linspace(-zmax, zmax, n + 1)
    g = np.min(np.asarray(mu)[:, None] + np.asarray(st)[:, None] * z[None, :], axis=0) * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return float(step * (g.sum() - 0.5 * (g[0] + g[-1])))


def bars(dtype, amplitude):
    """The project's plain bars scaled to y units: kg is a difference of means."""
    return (1e-8 if dtype == np.float64 else 1e-4) * max(1.0, math.sqrt(amplitude))
