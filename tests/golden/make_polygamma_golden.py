#!/usr/bin/env python3
"""Generate tests/golden/f14_polygamma.npz from the REFERENCE's own polygamma.

    make -C oracle && python tests/golden/make_polygamma_golden.py

``oracle.pyoracle.Reference().polygamma`` calls TRLDA::polygamma(int, double)
(src/utils.cpp:107-111) in oracle/_ref/libtrlda_ref.so; only its outputs are stored, with the
orders n and arguments x this script chooses:
  n in {-1, 0, 1, 2, 3, 5, 10, 20, 50};
  x: 300 points log-spaced from 1e-300 to 1e12, points either side of 1e8 (where the reference
  switches from Euler-Maclaurin to its asymptotic formula), small integers and half-integers,
  non-positive integers, negative non-integers down to -100, +-inf and nan.
Also, for n in {-1, 0} only (`n_far`, `x_far`, `y_far`), negative non-integers below -2^20, where
the reference's digamma reflects; for n >= 1 its zeta would sum |x| terms one by one.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import pyoracle  # noqa: E402

ORDERS = [-1, 0, 1, 2, 3, 5, 10, 20, 50]


def arguments():
    xs = list(np.logspace(-300, 12, 300))
    xs += [1e8 * (1 + d) for d in (-1e-3, -1e-9, 0.0, 1e-9, 1e-3)] + [np.nextafter(1e8, 0), np.nextafter(1e8, 2e8)]
    xs += [0.5, 1.0, 1.4616321449683622, 1.5, 2.0, 3.0, 7.5, 9.999999, 10.0, 10.5, 20.0, 67.0, 120.0, 1e5 + 0.25]
    xs += [0.0, -0.0, -1.0, -2.0, -7.0, -50.0, -100.0]
    xs += [-1e-9, -0.25, -0.5, -0.75, -1.3, -2.5, -3.9, -7.25, -12.125, -33.3, -50.01, -77.7, -99.5, -99.9, -100.0 + 1e-6]
    xs += [np.inf, -np.inf, np.nan]
    return np.array(xs, dtype=np.float64)


def far_arguments():
    return np.array([-1048576.5, -1048576.25, -1048577.1, -2e6 - 0.3, -1e7 + 0.3, -123456789.75,
                     -3.5e9 - 0.0625, -1e15 - 0.125, -4503599627370495.5], dtype=np.float64)


def main():
    if not pyoracle.Reference.available():
        sys.exit("oracle/_ref not built (make -C oracle): nothing generated")
    ref = pyoracle.Reference()
    x = arguments()
    n = np.array(ORDERS, dtype=np.int64)
    y = np.array([[ref.polygamma(int(k), float(v)) for v in x] for k in n], dtype=np.float64)
    path = os.path.join(HERE, "f14_polygamma.npz")
    n_far = np.array([-1, 0], dtype=np.int64)
    x_far = far_arguments()
    y_far = np.array([[ref.polygamma(int(k), float(v)) for v in x_far] for k in n_far], dtype=np.float64)
    np.savez_compressed(path, n=n, x=x, y=y, n_far=n_far, x_far=x_far, y_far=y_far)
    print("f14_polygamma.npz %d x %d, %.1f kB" % (len(n), len(x), os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
