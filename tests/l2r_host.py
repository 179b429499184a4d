"""NumPy restatement of the left-to-right sampler of csrc/l2r_kernels.h (a helper module, not a
test file).

It follows the kernel's header step by step: the tokens are the entries in order, an entry giving
its count c > 0 of consecutive tokens; per position n the prefix's tokens t = 0 .. n-1 are redrawn
in order (purpose 22, counter (t, n, d R + r)) when `resample`, then the new token is drawn (purpose
23, counter (n, n, d R + r)); a weight is (lambda_kw * inv_k) * (alpha_k + (double)n_k) with each
operation rounded once; the histogram draw is gibbs_kernels.h's (lane-local prefix, Hillis-Steele
over the 64 lanes, r = u * total, the first lane and topic above r, the fall-backs), written here
for many streams at once; p_r(n) = total / (A + n) with A the k-ascending sum of alpha.  The two
combinations add in the kernel's orders.  Every draw and every weight is the kernel's to the bit
(given the same row sums); the logarithms are the host's, so loglik agrees to rounding.

A stream is one (document index d, particle r): its third counter word is d R + r.  `table` takes
any array of such words, so that one call runs the replicates of a statistical test at once.
"""
import math

import numpy as np

from gibbs_host import WAVE, kpl_of, philox4x32_10, split_key, uniform

PREFIX, TOKEN = 22, 23
ERROR = "Something went wrong while sampling from histogram."


def draw(p, u, kpl):
    """One histogram draw per row of p (S x 64 kpl, topics >= K zero) with the uniforms u (S).
    Returns (topics, totals); raises as the library does when a total is not > 0 or not finite."""
    S = p.shape[0]
    rows = np.arange(S)
    pr = p.reshape(S, WAVE, kpl)
    q = np.cumsum(pr, axis=2)                               # lane-local sequential prefix
    x = q[:, :, -1].copy()
    off = 1
    while off < WAVE:                                       # Hillis-Steele, offsets 1 .. 32
        x[:, off:] = x[:, off:] + x[:, :-off]
        off <<= 1
    total = x[:, -1].copy()
    if not np.all((total > 0.0) & np.isfinite(total)):
        raise RuntimeError(ERROR)
    r = u * total
    excl = np.concatenate((np.zeros((S, 1)), x[:, :-1]), axis=1)
    hit = x > r[:, None]
    anyhit = hit.any(axis=1)
    L = hit.argmax(axis=1)
    inl = (excl[rows, L][:, None] + q[rows, L]) > r[:, None]
    anyin = inl.any(axis=1)
    nzl = pr[rows, L] > 0.0
    lastl = kpl - 1 - nzl[:, ::-1].argmax(axis=1)
    nz = p > 0.0
    last = p.shape[1] - 1 - nz[:, ::-1].argmax(axis=1)
    z = np.where(anyhit & anyin, L * kpl + inl.argmax(axis=1),
                 np.where(anyhit & nzl.any(axis=1), L * kpl + lastl, last))
    return z.astype(np.int64), total


def alpha_sum(alpha):
    A = 0.0
    for a in np.asarray(alpha, dtype=np.float64).reshape(-1).tolist():
        A = A + a
    return A


def table(entries, lam, inv, alpha, c2, key, resample):
    """p[n, s]: position n of the document `entries` = [(w, c), ..] in stream s, whose third
    counter word is c2[s]."""
    lam = np.asarray(lam, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    c2 = np.asarray(c2, dtype=np.uint64)
    K = lam.shape[0]
    kpl = kpl_of(K)
    KP = WAVE * kpl
    k0, k1 = split_key(key)
    S = len(c2)
    rows = np.arange(S)
    words = [int(w) for w, c in entries for _ in range(max(int(c), 0))]
    N = len(words)
    A = alpha_sum(alpha)
    al = np.zeros(KP)
    al[:K] = alpha
    cols = {}
    for w in set(words):
        col = np.zeros(KP)
        col[:K] = lam[:, w] * inv
        cols[w] = col
    cnt = np.zeros((S, KP), dtype=np.int64)
    z = np.zeros((S, max(N, 1)), dtype=np.int64)
    P = np.empty((N, S))
    for n in range(N):
        if resample and n > 0:
            x = philox4x32_10(np.arange(n, dtype=np.uint64)[None, :], n, c2[:, None], PREFIX, k0, k1)
            us = uniform(x[0], x[1])
            for t in range(n):
                cnt[rows, z[:, t]] -= 1
                p = cols[words[t]][None, :] * (al[None, :] + cnt.astype(np.float64))
                zz, _ = draw(p, us[:, t], kpl)
                cnt[rows, zz] += 1
                z[:, t] = zz
        x = philox4x32_10(n, n, c2, TOKEN, k0, k1)
        p = cols[words[n]][None, :] * (al[None, :] + cnt.astype(np.float64))
        zz, total = draw(p, uniform(x[0], x[1]), kpl)
        P[n] = total / (A + float(n))
        cnt[rows, zz] += 1
        z[:, n] = zz
    return P


def combine(P, how):
    """loglik of each group of R streams: P is N x G x R (or N x R).  'particle': L_r = sum_n log
    p_r(n), n ascending; (M + log sum_r exp(L_r - M)) - log R, r ascending.  'position': sum_n
    log((sum_r p_r(n)) / R), r ascending, then n ascending."""
    P = np.asarray(P, dtype=np.float64)
    single = P.ndim == 2
    if single:
        P = P[:, None, :]
    N, G, R = P.shape
    if N == 0:
        out = np.zeros(G)
    elif how == "particle":
        Lr = np.cumsum(np.log(P), axis=0)[-1]                              # G x R
        M = Lr.max(axis=1)
        with np.errstate(invalid="ignore"):
            s = np.cumsum(np.exp(Lr - M[:, None]), axis=1)[:, -1]
            out = np.where(M == -np.inf, -np.inf, (M + np.log(s)) - math.log(float(R)))
    elif how == "position":
        s = np.cumsum(P, axis=2)[:, :, -1]                                 # N x G
        out = np.cumsum(np.log(s / float(R)), axis=0)[-1]
    else:
        raise TypeError("`combine` should be either 'particle' or 'position'.")
    return float(out[0]) if single else out


def left_to_right(indptr, ids, cnts, lam, alpha, key, R, resample=True, rowsum=None, only=None):
    """({'particle': loglik[B], 'position': loglik[B]}, tokens[B]) of the CSR batch under `key` with
    R particles.  `rowsum`: the row sums of lambda (default: lam.sum(axis=1)).  `only`: the document
    indices to compute (the others stay nan)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    lam = np.asarray(lam, dtype=np.float64)
    B = len(indptr) - 1
    inv = 1.0 / (lam.sum(axis=1) if rowsum is None else np.asarray(rowsum, dtype=np.float64))
    out = {"particle": np.full(B, np.nan), "position": np.full(B, np.nan)}
    tokens = np.zeros(B)
    for d in range(B):
        p0, p1 = int(indptr[d]), int(indptr[d + 1])
        entries = list(zip(np.asarray(ids[p0:p1]).tolist(), np.asarray(cnts[p0:p1]).tolist()))
        tokens[d] = float(sum(max(c, 0) for _, c in entries))
        if only is not None and d not in only:
            continue
        P = table(entries, lam, inv, alpha, d * R + np.arange(R), key, resample)
        for how in out:
            out[how][d] = combine(P, how)
    return out, tokens
