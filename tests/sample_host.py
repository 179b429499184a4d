"""NumPy restatement of the document sampler of csrc/sample_kernels.h and trlda_sample_lengths (a
helper module, not a test file).

It follows the contract of csrc/philox.h and csrc/sample_kernels.h step by step: the gamma draws
with their purposes as parameters, the lengths by inversion against a table built with Python's
math.log and math.exp (the C library's, as the host code calls them), the beta table's chunked
prefix and theta's lane-blocked prefix in the kernels' order of additions, and the two search
rules of a token.  Given the device's own theta and beta table it reproduces every word id
exactly; the table and theta themselves to log / exp / cos rounding.
"""
import bisect
import math

import numpy as np

from gibbs_host import philox4x32_10, uniform, uniform_open

BETA = (8, 9, 10)          # beta gamma: normal / accept / boost, counter (word w, topic k, attempt)
THETA = (11, 12, 13)       # theta gamma: normal / accept / boost, counter (topic k, document d, attempt)
LENGTH, TOKEN = 14, 15
GAMMA_TRIES = 64
WAVE, PER_LANE, WAVES = 64, 16, 4
CHUNK = WAVE * PER_LANE * WAVES


def split_key(key):
    return int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF


def log_gamma(a, c0, c1, purposes, key):
    """log of the Gamma(a) draws of counter words (c0, c1) (broadcast arrays) under the three
    purposes (normal, accept, boost): philox.h's recipe."""
    k0, k1 = split_key(key)
    pn, pa, pb = purposes
    a, c0, c1 = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(c0, dtype=np.uint64),
                                    np.asarray(c1, dtype=np.uint64))
    ok = (a > 0) & (a <= 1e300)
    boost = a < 1.0
    sh = np.where(boost, a + 1.0, a)
    d = sh - 1.0 / 3.0
    with np.errstate(divide="ignore", invalid="ignore"):
        c = 1.0 / np.sqrt(9.0 * d)
        lg = np.log(d)
        todo = ok.copy()
        for n in range(GAMMA_TRIES):
            if not todo.any():
                break
            w = philox4x32_10(c0, c1, n, pn, k0, k1)
            x = np.sqrt(-2.0 * np.log(uniform_open(w[0], w[1]))) * np.cos(6.283185307179586 * uniform(w[2], w[3]))
            v1 = 1.0 + c * x
            v = v1 * v1 * v1
            w = philox4x32_10(c0, c1, n, pa, k0, k1)
            lu = np.log(uniform_open(w[0], w[1]))
            lv = np.log(v)
            acc = todo & (v1 > 0.0) & (lu < 0.5 * x * x + d - d * v + d * lv)
            lg = np.where(acc, np.log(d) + lv, lg)
            todo &= ~acc
        w = philox4x32_10(c0, c1, 0, pb, k0, k1)
        lg = np.where(boost, lg + np.log(uniform_open(w[0], w[1])) / a, lg)
    return np.where(ok, lg, -np.inf)


# ---- lengths --------------------------------------------------------------------------------
def length_cdf(length):
    """CDF_0 .. CDF_kmax of the header's table, with math.log / math.exp and sequential sums."""
    length = float(length)
    kmax = int(math.ceil(length + 12.0 * math.sqrt(length) + 40.0))
    log_lambda = math.log(length) if length > 0 else -math.inf
    l = -length
    cdf = [math.exp(l)]
    for k in range(1, kmax + 1):
        l = l + log_lambda - math.log(float(k))
        cdf.append(cdf[-1] + math.exp(l))
    return cdf


def lengths(B, length, key):
    """indptr[B+1] of trlda_sample_lengths."""
    k0, k1 = split_key(key)
    cdf = length_cdf(length)
    total = cdf[-1]
    w = philox4x32_10(np.arange(B), 0, 0, LENGTH, k0, k1)
    r = uniform(w[0], w[1]) * total
    n = []
    for x in r.tolist():
        k = bisect.bisect_right(cdf, x)          # the first k with CDF_k > x
        if k == len(cdf):
            k = bisect.bisect_left(cdf, total)   # x rounded up to the total
        n.append(k)
    return np.concatenate(([0], np.cumsum(n))).astype(np.int64)


# ---- the two prefixes -----------------------------------------------------------------------
def _seq_offsets(lasts, axis):
    """e_0 = 0, e_{i+1} = e_i + lasts_i along `axis` (sequential), and e_n."""
    c = np.cumsum(lasts, axis=axis)
    e = np.concatenate((np.zeros_like(np.take(c, [0], axis=axis)), c), axis=axis)
    n = e.shape[axis]
    return np.take(e, range(n - 1), axis=axis), np.take(e, [n - 1], axis=axis)


def beta_prefix(W):
    """C of the header from the weights W (K x V), topic-major."""
    K, V = W.shape
    nchunk = -(-V // CHUNK)
    pad = np.zeros((K, nchunk * CHUNK))
    pad[:, :V] = W
    q = np.cumsum(pad.reshape(K, nchunk, WAVES, WAVE, PER_LANE), axis=-1)
    e, _ = _seq_offsets(q[..., -1], axis=-1)                 # lanes of a wave
    L1 = e[..., None] + q
    g, _ = _seq_offsets(L1[..., -1, -1], axis=-1)            # the 4 waves
    L2 = g[..., None, None] + L1
    o, _ = _seq_offsets(L2[:, :, -1, -1, -1], axis=-1)       # the chunks
    C = o[:, :, None, None, None] + L2
    return C.reshape(K, -1)[:, :V]


def beta_table(lam, key):
    """The beta prefix table of lambda (K x V) and the key."""
    lam = np.asarray(lam, dtype=np.float64)
    K, V = lam.shape
    lg = log_gamma(lam, np.arange(V)[None, :], np.arange(K)[:, None], BETA, key)
    mx = lg.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        W = np.exp(lg - mx)
    return beta_prefix(W)


def theta_blocked(v):
    """The lane-blocked prefix of the K x B columns v (header: P), and S = its value at K - 1."""
    K, B = v.shape
    kpl = -(-K // WAVE)
    pad = np.zeros((WAVE * kpl, B))
    pad[:K] = v
    q = np.cumsum(pad.reshape(WAVE, kpl, B), axis=1)
    E, total = _seq_offsets(q[:, -1, :], axis=0)
    P = (E[:, None, :] + q).reshape(WAVE * kpl, B)[:K]
    return P, total[0]


def theta(alpha, B, key):
    """theta (K x B) of the documents 0 .. B-1."""
    alpha = np.asarray(alpha, dtype=np.float64)
    K = alpha.size
    lg = log_gamma(alpha[:, None], np.arange(K)[:, None], np.arange(B)[None, :], THETA, key)
    W = np.exp(lg - lg.max(axis=0, keepdims=True))
    _, S = theta_blocked(W)
    return W / S


# ---- tokens ---------------------------------------------------------------------------------
def _first_above(c, r):
    """The first i with c[i] > r, else the first with c[i] >= c[-1] (c non-decreasing)."""
    i = np.searchsorted(c, r, side="right")
    if (i == len(c)).any():
        i = np.where(i == len(c), np.searchsorted(c, c[-1], side="left"), i)
    return i


def tokens(indptr, theta_dev, table, key):
    """Every token's word id (and topic), from the device's theta (K x B) and beta table."""
    indptr = np.asarray(indptr, dtype=np.int64)
    P, _ = theta_blocked(np.asarray(theta_dev, dtype=np.float64))
    nnz = int(indptr[-1])
    t = np.arange(nnz, dtype=np.int64)
    d = np.searchsorted(indptr, t, side="right") - 1
    k0, k1 = split_key(key)
    x = philox4x32_10(t - indptr[d], d, 0, TOKEN, k0, k1)
    u1, u2 = uniform(x[0], x[1]), uniform(x[2], x[3])
    z = np.empty(nnz, dtype=np.int64)
    for doc in np.unique(d):
        sel = d == doc
        col = P[:, doc]
        z[sel] = _first_above(col, u1[sel] * col[-1])
    w = np.empty(nnz, dtype=np.int64)
    for k in np.unique(z):
        sel = z == k
        row = table[k]
        w[sel] = _first_above(row, u2[sel] * row[-1])
    return w, z
