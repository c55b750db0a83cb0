"""Writes tests/golden/mes_table.npy: t(g) = g lambda(g) / 2 - log Phi(g) and t'(g) = -(lambda / 2) (1 + g^2 + g lambda),
lambda = phi / Phi, at fixed g, from mpmath at 60 digits.  The file holds one float64 array [3, 5219]: row 0 is g as the double it is, rows 1
and 2 are t and t' as the nearest doubles -- binary, as 5 219 rows of text would be most of a change's lines, and .npy, as the
fixture tests take every .npz of this directory for one of their cases.  The tests read only the file.

    python tests/golden/make_mes_table.py

Up to |g| = 100 both functions come from the definition with mpmath's ncdf and npdf (mpf does not underflow; the working
precision covers the cancellation of about g^2 in t and g^4 in t').  Beyond, from the asymptotic series of the Mills ratio,
a u = sum_k (-1)^k (2k-1)!! / a^(2k) (its terms fall below 1e-100 long before they grow again), with 1 - a u summed on its own so
that only (a u - a^2 (1 - a u)) cancels, at a precision that covers it.  At g = -100 the two routes are compared."""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from mes_ref import BRANCH_POINTS  # noqa: E402

mp.mp.dps = 60
POINTS = (-1e150, -1e7, -25.001, -25.0, -24.999, -1.0, -0.999999, 0.0, 1e-300, 8.0, 37.9, 38.5)


def points():
    g = list(np.linspace(-40.0, 8.0, 4801)) + list(-(10.0 ** np.linspace(0.0, 7.0, 400)))
    for b in BRANCH_POINTS:
        g += [np.nextafter(b, -np.inf), np.nextafter(b, np.inf)]
    g += list(POINTS)
    return [float(v) for v in g]


def by_definition(g):
    with mp.workdps(200):
        g = mp.mpf(g)
        cdf = mp.ncdf(g)
        lam = mp.npdf(g) / cdf
        return +(g * lam / 2 - mp.log(cdf)), +(-(lam / 2) * (1 + g * g + g * lam))


def by_series(g):
    a = -mp.mpf(g)
    with mp.workdps(60 + int(4 * mp.log10(a)) + 40):
        x = 1 / (a * a)
        au, b, term, k = mp.mpf(1), mp.mpf(0), mp.mpf(1), 0
        while abs(term) > mp.mpf(10) ** -(mp.mp.dps + 5):
            k += 1
            term = -term * (2 * k - 1) * x  # (-1)^k (2k-1)!! / a^(2k)
            au += term
            b -= term
            assert k < 400
        w = b / x / au
        t = -w / 2 + mp.log(2 * mp.pi) / 2 + mp.log(a) - mp.log(au)
        return +t, +(-(a / au) * (1 - w) / 2)


def functions(g):
    return by_definition(g) if abs(g) <= 100.0 else by_series(g)


def main():
    for f, h in zip(by_definition(-100.0), by_series(-100.0)):
        assert abs(f - h) <= mp.mpf(10) ** -50 * abs(f), (f, h)
    gs = points()
    vals = [functions(g) for g in gs]
    np.save(os.path.join(HERE, "mes_table.npy"), np.array([gs, [float(v[0]) for v in vals], [float(v[1]) for v in vals]]))
    print(f"{len(gs)} rows")


if __name__ == "__main__":
    main()
