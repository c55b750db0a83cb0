"""Writes tests/golden/logei_table.json: log h, Phi / h, phi / h, log Phi and phi / Phi (h(z) = z Phi(z) + phi(z)) at fixed z, from
mpmath at 60 digits.  Each entry holds z as the double it is (hex) and every function as the nearest double (hex) and as a decimal
string of 40 significant digits.  The tests read only the JSON.

    python tests/golden/make_logei_table.py
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from lcei_ref import BRANCH_POINTS  # noqa: E402

mp.mp.dps = 60
NAMES = ("log_h", "cdf_over_h", "pdf_over_h", "log_cdf", "pdf_over_cdf")


def points():
    z = list(np.linspace(-40.0, 10.0, 201)) + list(-(10.0 ** np.linspace(0.0, 8.0, 81)))
    for b in BRANCH_POINTS:
        z += [b - 1e-6, b + 1e-6]
    z += [38.0, -38.0, 50.0, 1e3]
    return [float(v) for v in z]


def functions(z):
    """The five functions at the double z, as mpf.  phi is never formed on its own: with E = exp(z^2 / 2), cdf E and h E stay in
    range at any z."""
    z = mp.mpf(z)
    half_log_2pi = mp.log(2 * mp.pi) / 2
    if z < 0:
        a = -z
        # u = Phi(-a) / phi(a) = sqrt(pi / 2) exp(a^2 / 2) erfc(a / sqrt 2), evaluated with enough digits for the cancellation in b
        with mp.workdps(60 + int(2 * mp.log10(a + 1)) + 30):
            u = mp.sqrt(mp.pi / 2) * mp.exp(a * a / 2) * mp.erfc(a / mp.sqrt(2))
            b = 1 - a * u
            base = -a * a / 2 - half_log_2pi
            return (+(base + mp.log(b)), +(u / b), +(1 / b), +(base + mp.log(u)), +(1 / u))
    cdf = mp.ncdf(z)
    pdf = mp.npdf(z)
    h = z * cdf + pdf
    return (mp.log(h), cdf / h, pdf / h, mp.log1p(-mp.ncdf(-z)), pdf / cdf)


def main():
    rows = []
    for z in points():
        row = {"z": z.hex()}
        for name, val in zip(NAMES, functions(z)):
            row[name] = {"double": float(val).hex(), "decimal": mp.nstr(val, 40)}
        rows.append(row)
    with open(os.path.join(HERE, "logei_table.json"), "w") as f:
        json.dump({"digits": 60, "functions": list(NAMES), "rows": rows}, f, indent=0)
        f.write("\n")
    print(f"{len(rows)} rows")


if __name__ == "__main__":
    main()
