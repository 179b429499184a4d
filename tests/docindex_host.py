"""NumPy restatement of the document index (csrc/docindex_kernels.h): the row of a
document with variational parameter gamma (K values),

    hellinger:  r_k = sqrt(gamma_k / sum(gamma))
    cosine:     t_k = gamma_k / sum(gamma),  r_k = t_k / sqrt(sum_k t_k^2)

the similarity s(q, d) = sum_k r_qk r_dk as an np.longdouble dot of float64 rows, and the ranking in
the total order (s descending, id ascending)."""
import numpy as np


def rows(gamma, measure="hellinger"):
    """gamma K x B -> rows B x K (float64)."""
    g = np.asarray(gamma, dtype=np.float64)
    g = g.reshape(g.shape[0], -1)
    theta = (g / g.sum(axis=0)).T
    if measure == "hellinger":
        return np.sqrt(theta)
    if measure == "cosine":
        return theta / np.sqrt((theta * theta).sum(axis=1))[:, None]
    raise ValueError(measure)


def similarities(qrows, irows):
    """s, B x N, rounded from the longdouble dot of the float64 rows."""
    q = np.asarray(qrows, dtype=np.float64).astype(np.longdouble)
    r = np.asarray(irows, dtype=np.float64).astype(np.longdouble)
    return q.dot(r.T)


def rank(s):
    """Per query the ids in the order (s descending, id ascending): B x N."""
    s = np.asarray(s)
    B, N = s.shape
    ids = np.arange(N)
    order = np.empty((B, N), dtype=np.int64)
    for b in range(B):
        order[b] = np.lexsort((ids, -s[b]))
    return order


def gaps(ranked_s, top_n):
    """Per query the smallest gap s_r - s_{r+1} between consecutive ranked similarities among the
    first top_n + 1 (all N where there are fewer; inf for a single one): how far the query's top_n
    is from a different answer."""
    q = np.asarray(ranked_s)[:, :top_n + 1]
    if q.shape[1] < 2:
        return np.full(q.shape[0], np.inf)
    return np.min(q[:, :-1] - q[:, 1:], axis=1).astype(np.float64)


def distance(s, measure="hellinger"):
    rest = np.maximum(0.0, 1.0 - np.asarray(s, dtype=np.float64))
    return np.sqrt(rest) if measure == "hellinger" else rest


def search(qrows, irows, top_n):
    """(ids B x top_n int64, s B x top_n longdouble, gap B) of the queries' rows against the index's."""
    s = similarities(qrows, irows)
    order = rank(s)
    ranked = np.take_along_axis(s, order, axis=1)
    return order[:, :top_n], ranked[:, :top_n], gaps(ranked, top_n)
