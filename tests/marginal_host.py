"""NumPy restatement of the documents' marginal likelihood by importance sampling of theta
(csrc/marginal_kernels.h; a helper module, not a test file), and the exact value by enumeration.

It follows the kernel's header step by step: the log-gamma draws are sample_host.log_gamma with
purposes 19 / 20 / 21 and counter (s K + k, d); log theta is lg - (mx + log sum exp(lg - mx)); every
sum over the topics is per lane (k = q 64 + l, q ascending) and then wave_sum_dpp's tree; the
constants are per thread (k = t, t + 64 W, ..), wave_sum_dpp, the waves in order; log w_s adds the
entries in document order; wave w keeps a running (max, sum, sum of squares) over its samples
s = w, w + W, .. and the waves are merged in order against the overall max.  The kernel's dot
products are FMAs and its log / exp / cos / lgamma are the device's, so values agree to rounding,
not bitwise.
"""
import itertools
import math

import numpy as np

from sample_host import log_gamma

PURPOSES = (19, 20, 21)
WAVE, MAX_WAVES, REG_MAX_K = 64, 8, 512
RED_DOUBLES = 4 * MAX_WAVES
LDS_DOUBLES = (160 * 1024 - 256) // 8

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def waves(K):
    """Waves of a document's workgroup (marginal_waves)."""
    if K <= REG_MAX_K:
        return MAX_WAVES
    return min(MAX_WAVES, (LDS_DOUBLES - RED_DOUBLES) // K)


def wave_sum_dpp(v):
    """estep_kernels.h, wave_sum_dpp over the last axis (64 lanes): row shifts by 1, 2, 4, 8 inside
    each row of 16 lanes (zeros shifted in), lane 15 of a row then holds the row's sum r; the total
    is (r3 + r2) + (r1 + r0)."""
    v = np.asarray(v, dtype=np.float64)
    v = v.reshape(v.shape[:-1] + (4, 16))
    for sh in (1, 2, 4, 8):
        moved = np.zeros_like(v)
        moved[..., sh:] = v[..., :-sh]
        v = v + moved
    r = v[..., 15]
    return (r[..., 3] + r[..., 2]) + (r[..., 1] + r[..., 0])


def lane_sum(x):
    """Sum over the last axis (K topics): lane l adds k = l, 64 + l, .. in order, then wave_sum_dpp."""
    K = x.shape[-1]
    kpl = -(-K // WAVE)
    pad = np.zeros(x.shape[:-1] + (kpl * WAVE,))
    pad[..., :K] = x
    pad = pad.reshape(x.shape[:-1] + (kpl, WAVE))
    s = np.zeros(x.shape[:-1] + (WAVE,))
    for q in range(kpl):
        s = s + pad[..., q, :]
    return wave_sum_dpp(s)


def block_sum(x, W):
    """Sum of K numbers by a workgroup of W waves: thread t adds k = t, t + 64 W, .. in order,
    wave_sum_dpp per wave, the waves in order."""
    K, T = len(x), W * WAVE
    n = -(-K // T)
    pad = np.zeros(n * T)
    pad[:K] = x
    pad = pad.reshape(n, W, WAVE)
    s = np.zeros((W, WAVE))
    for i in range(n):
        s = s + pad[i]
    per_wave = wave_sum_dpp(s)
    total = 0.0
    for w in range(W):
        total = total + per_wave[w]
    return float(total)


def dirichlet_constant(alpha, a, W):
    """C_d = [lgamma(sum alpha) - sum lgamma(alpha)] - [lgamma(sum a) - sum lgamma(a)]."""
    sa, la = block_sum(alpha, W), block_sum(_lgamma(alpha), W)
    sg, lg = block_sum(a, W), block_sum(_lgamma(a), W)
    return (math.lgamma(sa) - la) - (math.lgamma(sg) - lg)


def log_weights(entries, lam, irs, alpha, a, d, key, S, vi):
    """log w_s, s < S, of the document at index d with `entries` = [(w, c), ..] and proposal Dir(a)."""
    K = lam.shape[0]
    W = waves(K)
    s = np.arange(S, dtype=np.uint64)[:, None]
    k = np.arange(K, dtype=np.uint64)[None, :]
    lg = log_gamma(a[None, :], s * np.uint64(K) + k, d, PURPOSES, key)         # S x K
    mx = lg.max(axis=1)
    lse = mx + np.log(lane_sum(np.exp(lg - mx[:, None])))
    lt = lg - lse[:, None]
    phi = np.exp(lt) * irs[None, :]
    ll = np.zeros(S)
    for w, c in entries:
        if c == 0:
            continue
        ll = ll + float(c) * np.log(lane_sum(phi * lam[:, w][None, :]))
    if not vi:
        return ll
    t = lane_sum((alpha - a)[None, :] * lt)
    return ll + (dirichlet_constant(alpha, a, W) + t)


def combine(lw, W):
    """(loglik, ess) from the samples' log weights: a running (m, s1, s2) per wave over s = w, w + W, ..,
    the waves merged in order."""
    S = len(lw)
    parts = []
    for w in range(W):
        m, s1, s2 = -math.inf, 0.0, 0.0
        for x in lw[w::W].tolist():
            if x == -math.inf:
                continue
            if x > m:
                sc = math.exp(m - x)
                s1 = s1 * sc + 1.0
                s2 = s2 * (sc * sc) + 1.0
                m = x
            else:
                e = math.exp(x - m)
                s1 = s1 + e
                s2 = s2 + e * e
        parts.append((m, s1, s2))
    M = max(p[0] for p in parts)
    if M == -math.inf:
        return -math.inf, 0.0
    A = Q = 0.0
    for m, s1, s2 in parts:
        if m == -math.inf:
            continue
        sc = math.exp(m - M)
        A = A + s1 * sc
        Q = Q + s2 * (sc * sc)
    return (M + math.log(A)) - math.log(float(S)), min(max((A * A) / Q, 1.0), float(S))


def document_loglik(indptr, ids, cnts, lam, alpha, key, S, gamma=None, only=None):
    """(loglik[B], ess[B]) of the CSR batch under `key`: proposal Dir(gamma[:, d]) when gamma (K x B) is
    given ('vi'), else Dir(alpha) ('prior').  `only`: the document indices to compute (the others
    stay nan)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    lam = np.asarray(lam, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    K = lam.shape[0]
    B = len(indptr) - 1
    irs = 1.0 / lam.sum(axis=1)
    loglik, ess = np.full(B, np.nan), np.full(B, np.nan)
    for d in (range(B) if only is None else only):
        p0, p1 = int(indptr[d]), int(indptr[d + 1])
        if p0 >= p1:
            loglik[d], ess[d] = 0.0, float(S)
            continue
        entries = list(zip(np.asarray(ids[p0:p1]).tolist(), np.asarray(cnts[p0:p1]).tolist()))
        vi = gamma is not None
        a = np.ascontiguousarray(gamma[:, d], dtype=np.float64) if vi else alpha
        lw = log_weights(entries, lam, irs, alpha, a, d, key, S, vi)
        loglik[d], ess[d] = combine(lw, waves(K))
    return loglik, ess


def exact_log_marginal(beta, alpha, words):
    """log p(w) of a document whose tokens have the word ids `words`, by enumeration of the K^N topic
    assignments z:  p(w) = sum_z prod_i beta[z_i, w_i] Gamma(sum alpha) / Gamma(sum alpha + N)
    prod_k Gamma(alpha_k + n_k(z)) / Gamma(alpha_k)."""
    beta = np.asarray(beta, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    K, N = beta.shape[0], len(words)
    if N == 0:
        return 0.0
    states = np.array(list(itertools.product(range(K), repeat=N)), dtype=np.int64).reshape(-1, N)
    logp = np.zeros(len(states))
    for i, w in enumerate(words):
        logp += np.log(beta[states[:, i], w])
    for k in range(K):
        n_k = (states == k).sum(axis=1)
        logp += _lgamma(alpha[k] + n_k) - math.lgamma(alpha[k])
    logp += math.lgamma(alpha.sum()) - math.lgamma(alpha.sum() + N)
    m = logp.max()
    return float(m + np.log(np.exp(logp - m).sum()))
