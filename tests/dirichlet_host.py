"""NumPy restatement of sample_dirichlet (csrc/dirichlet_kernels.h; a helper module, not a test file).

Entry (i, j) is sample_host.log_gamma with purposes 16 / 17 / 18 and counter (row i, column j); a
column is normalised in log space with the kernels' order of additions: m <= 1024 a wave's lanes
(rows q * 64 + l, summed in order of q) and then the butterfly over the 64 lanes; larger m the
chunks of 4096 rows (thread t of wave w holds rows c * 4096 + q * 256 + w * 64 + l), a butterfly per
wave, the four waves in order, then the chunks in order.  The device's log, exp and cos are not
NumPy's to the last bit, so values agree to rounding, not bitwise.
"""
import numpy as np

from sample_host import log_gamma

PURPOSES = (16, 17, 18)
WAVE_ROWS, CHUNK, WAVE = 1024, 4096, 64


def _butterfly(t):
    """t: (..., 64, n) -> (..., n), t_l + t_{l+h} for h = 32 .. 1."""
    h = WAVE // 2
    while h:
        t = t[..., :h, :] + t[..., h:2 * h, :]
        h //= 2
    return t[..., 0, :]


def sample_dirichlet(m, n, alpha, key, columns=None):
    """The (m, n) draw, or only the given columns of it."""
    cols = np.arange(n) if columns is None else np.asarray(columns)
    i = np.arange(m, dtype=np.uint64)[:, None]
    j = cols.astype(np.uint64)[None, :]
    lg = log_gamma(np.full((m, len(cols)), float(alpha)), i, j, PURPOSES, key)
    W = np.exp(lg - lg.max(axis=0))
    return W / column_sums(W)


def column_sums(W):
    """S of every column of W (m x n) in the kernels' order of additions."""
    m, n = W.shape
    if m <= WAVE_ROWS:
        kpl = -(-m // WAVE)
        P = np.zeros((kpl * WAVE, n))
        P[:m] = W
        s = np.zeros((WAVE, n))
        for q in range(kpl):
            s = s + P[q * WAVE:(q + 1) * WAVE]
        S = _butterfly(s)
    else:
        nchunk = -(-m // CHUNK)
        P = np.zeros((nchunk * CHUNK, n))
        P[:m] = W
        P = P.reshape(nchunk, CHUNK // 256, 4, WAVE, n)          # (chunk, q, wave, lane, column)
        s = np.zeros((nchunk, 4, WAVE, n))
        for q in range(CHUNK // 256):
            s = s + P[:, q]
        waves = _butterfly(s)                                   # (chunk, wave, column)
        chunk = np.zeros((nchunk, n))
        for w in range(4):
            chunk = chunk + waves[:, w]
        S = np.zeros(n)
        for c in range(nchunk):
            S = S + chunk[c]
    return S
