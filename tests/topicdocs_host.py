"""NumPy restatement of the topic summaries of a document index (csrc/topicdocs_kernels.h, DESIGN.md
3.24).  theta^ is theta recovered from the stored rows r (N x K float64),

    hellinger:  theta^_dk = r_dk * r_dk
    cosine:     theta^_dk = r_dk / sum_j r_dj, the sum in the device's order: lane l of 64 adds
                elements l, l + 64, ... in that order, and the 64 lane sums are added as a balanced
                binary tree of neighbours (what the six DPP steps of wave_sum_dpp come to)

both in float64, so on the device's own rows theta^ is the device's bit for bit.  On it: the ranking
per topic in the total order (theta^ descending, id ascending) with a near-tie report, and the mean,
the centred scatter, the covariance and the correlation in np.longdouble."""
import numpy as np

LD = np.longdouble
LANES = 64


def row_sums(rows):
    """sum_j r_dj (N, float64) in the device's order."""
    r = np.asarray(rows, dtype=np.float64)
    N, K = r.shape
    pad = np.zeros((N, -(-K // LANES) * LANES))
    pad[:, :K] = r
    lanes = np.zeros((N, LANES))
    for c in range(pad.shape[1] // LANES):               # lane l: elements l, l + 64, ... (x + 0 = x)
        lanes = lanes + pad[:, c * LANES:(c + 1) * LANES]
    while lanes.shape[1] > 1:
        lanes = lanes[:, 0::2] + lanes[:, 1::2]
    return lanes[:, 0]


def theta_hat(rows, measure="hellinger"):
    """rows N x K -> theta^ N x K (float64)."""
    r = np.asarray(rows, dtype=np.float64)
    if measure == "hellinger":
        return r * r
    if measure == "cosine":
        return r / row_sums(r)[:, None]
    raise ValueError(measure)


def rank(theta):
    """Per topic the ids in the order (theta descending, id ascending): K x N."""
    theta = np.asarray(theta)
    N, K = theta.shape
    ids = np.arange(N)
    order = np.empty((K, N), dtype=np.int64)
    for k in range(K):
        order[k] = np.lexsort((ids, -theta[:, k]))
    return order


def gaps(ranked, top_n):
    """Per topic the smallest relative gap (t_r - t_{r+1}) / t_r between consecutive ranked values
    among the first top_n + 1 -- the first value left out included; all N where there are fewer; inf
    for a single one: how far the topic's top_n is from a different answer."""
    q = np.asarray(ranked, dtype=np.float64)[:, :top_n + 1]
    if q.shape[1] < 2:
        return np.full(q.shape[0], np.inf)
    return np.min((q[:, :-1] - q[:, 1:]) / q[:, :-1], axis=1)


def top_documents(theta, top_n):
    """(ids K x top_n int64, theta K x top_n float64, gap K) of theta (N x K)."""
    theta = np.asarray(theta, dtype=np.float64)
    order = rank(theta)
    ranked = np.take_along_axis(theta.T, order, axis=1)
    return order[:, :top_n], ranked[:, :top_n], gaps(ranked, top_n)


def mean(theta):
    """m_k = sum_d theta_dk / N in longdouble."""
    t = np.asarray(theta, dtype=np.float64).astype(LD)
    return t.sum(axis=0) / LD(t.shape[0])


def scatter(theta, m=None):
    """(S, A) in longdouble: S_ij = sum_d (theta_di - m_i)(theta_dj - m_j) about `m` (default: the
    longdouble mean) and A_ij = sum_d |theta_di - m_i| |theta_dj - m_j|, what a rounding error of S
    scales with."""
    t = np.asarray(theta, dtype=np.float64).astype(LD)
    c = t - (mean(theta) if m is None else np.asarray(m).astype(LD))
    return c.T.dot(c), np.abs(c).T.dot(np.abs(c))


def covariance(S, N, ddof=1):
    """S / (N - ddof), in the type of S."""
    S = np.asarray(S)
    return S / S.dtype.type(N - ddof)


def correlation(S):
    """S_ij / (sqrt(S_ii) sqrt(S_jj)), the two roots apart, clamped to [-1, 1]; an exact 1 on the
    diagonal; NaN where either variance is 0 (the diagonal included), as np.corrcoef gives.  In the
    type of S."""
    S = np.asarray(S)
    var = np.diag(S)
    sd = np.sqrt(np.maximum(var, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.clip(S / (sd[:, None] * sd[None, :]), -1, 1)
    flat = ~(var > 0)
    np.fill_diagonal(c, 1)
    c[flat, :] = np.nan
    c[:, flat] = np.nan
    return c
