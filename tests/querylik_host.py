"""NumPy restatement of the query-likelihood search over a document index (csrc/querylik_kernels.h,
DESIGN.md 3.25): for a query with entries (w_i, c_i) and an indexed document d

    score(q, d) = sum_i c_i log P(d, w_i),   P(d, w) = sum_k theta^_dk beta_kw,   beta_kw = lambda_kw / sum_v lambda_kv

in np.longdouble from float64 theta^ and lambda, and the ranking in the total order (score descending,
id ascending).  theta^ is topicdocs_host.theta_hat of the device's own rows, so on that side the
restatement has the device's bits.

The device adds a score's terms in an order that depends on the entry's position i within its query
alone: position i lies in tile i // 16 at j = i % 16; the terms j, j + 4, j + 8, j + 12 of a lane group
g = j % 4 are added in that order, the four groups' sums as (p_0 + p_1) + (p_2 + p_3), and the tiles'
sums in ascending order.  Entries with a count <= 0 and the pad of the last tile add no term.  The
restatement adds in longdouble in the entries' order; the difference is inside the tests' bound."""
import numpy as np

LD = np.longdouble


def word_rows(lam):
    """beta (K x V longdouble) of lambda (K x V float64)."""
    lam = np.asarray(lam, dtype=np.float64).astype(LD)
    return lam / lam.sum(axis=1)[:, None]


def probs(theta_hat, lam):
    """P(d, w), N x V longdouble."""
    return np.asarray(theta_hat, dtype=np.float64).astype(LD).dot(word_rows(lam))


def scores(theta_hat, lam, queries):
    """B x N longdouble: sum_i c_i log(theta^ . beta_w_i); an entry with c_i <= 0 adds nothing."""
    P = probs(theta_hat, lam)
    out = np.zeros((len(queries), P.shape[0]), dtype=LD)
    with np.errstate(divide="ignore"):
        logP = np.log(P)
    for b, query in enumerate(queries):
        for w, c in query:
            if c > 0:
                out[b] += LD(c) * logP[:, w]
    return out


def rank(s):
    """Per query the ids in the order (score descending, id ascending): B x N."""
    s = np.asarray(s)
    B, N = s.shape
    ids = np.arange(N)
    order = np.empty((B, N), dtype=np.int64)
    for b in range(B):
        order[b] = np.lexsort((ids, -s[b]))
    return order


def gaps(ranked_s, top_n):
    """Per query the smallest absolute gap between consecutive ranked scores among the first
    top_n + 1 (all N where there are fewer; inf for a single one)."""
    q = np.asarray(ranked_s)[:, :top_n + 1]
    if q.shape[1] < 2:
        return np.full(q.shape[0], np.inf)
    with np.errstate(invalid="ignore"):
        d = q[:, :-1] - q[:, 1:]
    return np.min(np.where(np.isnan(d), 0, d), axis=1).astype(np.float64)   # (-inf next to -inf: a tie)


def search(theta_hat, lam, queries, top_n):
    """(ids B x top_n int64, scores B x top_n longdouble, gap B)."""
    s = scores(theta_hat, lam, queries)
    order = rank(s)
    ranked = np.take_along_axis(s, order, axis=1)
    return order[:, :top_n], ranked[:, :top_n], gaps(ranked, top_n)


def per_word(s, queries):
    """s (B x anything) divided by each query's sum of counts; a query without words keeps its 0.0."""
    s = np.array(s, copy=True)
    for b, query in enumerate(queries):
        total = sum(c for _, c in query if c > 0)
        if total > 0:
            s[b] = s[b] / total
    return s
