"""NumPy restatement of the word recommendation (csrc/recommend_kernels.h): for
document d with variational parameter gamma_d (K values) and word w

    t_dk = gamma_dk / sum_j gamma_dj,  q_dk = t_dk / rs_k,  rs_k = sum_v lambda_kv,
    s(d, w) = sum_k q_dk lambda_kw,

as an np.longdouble computation from the float64 gamma and lambda (sums, divisions and the dot all
in longdouble: the device's own roundings are what the accuracy bound of the GPU test allows for),
the exclusion of seen words (an entry (w, c) with c > 0; repeated entries count once), the ranking
in the total order (s descending, word id ascending) and the pad (-1, 0.0)."""
import numpy as np


def scores(gamma, lam):
    """s, B x V longdouble, from gamma K x B and lambda K x V."""
    g = np.asarray(gamma, dtype=np.float64)
    g = g.reshape(g.shape[0], -1).astype(np.longdouble)
    lm = np.asarray(lam, dtype=np.float64).astype(np.longdouble)
    q = (g / g.sum(axis=0)) / lm.sum(axis=1)[:, None]
    return q.T.dot(lm)


def seen(indptr, ids, cnts, V):
    """B x V bool: document d has an entry (w, c) with c > 0."""
    indptr = np.asarray(indptr, dtype=np.int64)
    B = len(indptr) - 1
    out = np.zeros((B, V), dtype=bool)
    for d in range(B):
        for p in range(indptr[d], indptr[d + 1]):
            if cnts[p] > 0:
                out[d, ids[p]] = True
    return out


def rank(s, left_out=None):
    """Per document the candidate words in the order (s descending, id ascending): a list of B int64 arrays."""
    s = np.asarray(s)
    B, V = s.shape
    ids = np.arange(V)
    out = []
    for d in range(B):
        order = np.lexsort((ids, -s[d]))
        if left_out is not None:
            order = order[~left_out[d][order]]
        out.append(order.astype(np.int64))
    return out


def ranked_gaps(s, orders, top_n):
    """Per document the relative gaps (s_r - s_{r+1}) / s_r between consecutive ranked scores among
    the first top_n + 1 candidates (all of them where there are fewer): a list of B float64 arrays."""
    out = []
    for d, order in enumerate(orders):
        r = np.asarray(s)[d][order[:top_n + 1]]
        out.append(((r[:-1] - r[1:]) / r[:-1]).astype(np.float64))
    return out


def gaps(s, orders, top_n):
    """Per document the smallest of ranked_gaps (inf for fewer than two candidates): how far the
    document's top_n is from a different answer."""
    return np.array([g.min() if len(g) else np.inf for g in ranked_gaps(s, orders, top_n)])


def recommend(gamma, lam, top_n, docs=None, s=None):
    """(words B x top_n int32, probs B x top_n longdouble, gap B); docs = (indptr, ids, cnts) of the
    seen words, or None to rank every word.  Rows shorter than top_n are padded with (-1, 0.0).
    `s`: scores(gamma, lam) where the caller has them already."""
    if s is None:
        s = scores(gamma, lam)
    B, V = s.shape
    left_out = seen(docs[0], docs[1], docs[2], V) if docs is not None else None
    orders = rank(s, left_out)
    words = np.full((B, top_n), -1, dtype=np.int32)
    probs = np.zeros((B, top_n), dtype=np.longdouble)
    for d, order in enumerate(orders):
        n = min(top_n, len(order))
        words[d, :n] = order[:n]
        probs[d, :n] = s[d][order[:n]]
    return words, probs, gaps(s, orders, top_n)


def recall(words, observed, heldout, V):
    """(recall, hits, relevant) by the definition, one document at a time: relevant_d is the number
    of distinct words with a positive count in heldout_d that observed_d has not seen, hits_d how
    many of them are among words[d]; the mean of hits / relevant over the documents with relevant > 0
    (None when there is none)."""
    held, obs = seen(*heldout, V), seen(*observed, V)
    B = held.shape[0]
    hits = np.zeros(B, dtype=np.int64)
    relevant = np.zeros(B, dtype=np.int64)
    for d in range(B):
        want = set(np.flatnonzero(held[d] & ~obs[d]).tolist())
        relevant[d] = len(want)
        hits[d] = len(want & set(int(w) for w in words[d] if w >= 0))
    keep = relevant > 0
    if not keep.any():
        return None, hits, relevant
    return float(np.mean(hits[keep] / relevant[keep])), hits, relevant
