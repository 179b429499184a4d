#!/usr/bin/env python3
"""Generate tests/golden/f16_trained_table.npz: the table the samplers read,
e = exp(psi(lambda) - psi(rowsum(lambda))), of the Gibbs cases of tests/trained_cases.py (and the one
V = 2000 case), at the columns of the table test's batch, from mpmath at 50 digits.

    python tests/golden/make_trained_table_golden.py

lambda and its row sums are taken as the exact fp64 inputs: every lambda_kv is converted exactly, the
row sum is their sum in exact arithmetic (lambda = eta + an integer below 2^17, at most 2000 of them: far
inside 50 digits), psi and exp are evaluated at 50 digits and the result is rounded to fp64 ONCE -- below
2^-1022 onto the subnormal grid directly (to the nearest multiple of 2^-1074), not to 53 bits first.
mpmath is needed by this script alone; no test imports it.  Stored per case: the columns, lambda at
those columns (the tests compare the lambda they rebuild with it bitwise), psi(lambda) and psi(row sum)
rounded to fp64 (the test's bound is made of their magnitudes), and the table.
"""
import os
import sys

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import trained_cases as tc  # noqa: E402

mp.dps = 50
TWO_1074 = mpf(2) ** -1074
TINY = mpf(2) ** -1022


def to_fp64(x):
    """x >= 0 at 50 digits -> the nearest fp64, rounded once"""
    if x < TINY:
        return float(np.ldexp(float(int(mp.nint(x / TWO_1074))), -1074))
    return float(x)


def table(lam, cols):
    K = lam.shape[0]
    e = np.empty((K, len(cols)))
    psi_lam = np.empty((K, len(cols)))
    psi_rs = np.empty(K)
    memo = {}
    for k in range(K):
        rs = mpf(0)
        for v in lam[k].tolist():
            rs += mpf(v)
        prs = mp.digamma(rs)
        psi_rs[k] = float(prs)
        for j, w in enumerate(cols):
            v = float(lam[k, w])
            if v not in memo:
                memo[v] = mp.digamma(mpf(v))
            psi_lam[k, j] = float(memo[v])
            e[k, j] = to_fp64(mp.exp(memo[v] - prs))
    return e, psi_lam, psi_rs


def main():
    out = {}
    for c in tc.table_cases():
        lam = tc.build(c)[0]
        cols = np.array(tc.table_columns(c), dtype=np.int32)
        e, psi_lam, psi_rs = table(lam, cols)
        name = tc.case_id(c) + ("" if c.V == tc.V else "-V%d" % c.V)
        out[name + "/cols"] = cols
        out[name + "/lam"] = np.ascontiguousarray(lam[:, cols])
        out[name + "/e"] = e
        out[name + "/psi_lam"] = psi_lam
        out[name + "/psi_rs"] = psi_rs
        print(name, e.shape, "min > 0: %.3g" % (e[e > 0].min() if (e > 0).any() else 0), "zeros:", int((e == 0).sum()))
    path = os.path.join(HERE, "f16_trained_table.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
