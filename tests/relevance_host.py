"""The contract of csrc/relevance_kernels.h restated in NumPy ``longdouble``: what
the GPU tests compare against and what tests/test_relevance_host.py checks by hand.

    R_k = sum_w lambda_kw, beta_kw = lambda_kw / R_k
    pi: None -> R_k / sum_j R_j; else the given weights / their sum
    p_w = sum_k c_k lambda_kw, c_k = pi_k / R_k
    r_kw = log lambda_kw - log R_k - (1 - weight) log p_w
    q_kw = c_k lambda_kw / p_w, D_w = sum_k q_kw (log q_kw - log pi_k), S_w = p_w D_w
    rankings: np.lexsort((arange(V), -value))[:top_n]
    prevalence: pi_k ~ sum_d N_d gamma_dk / sum_j gamma_dj, N_d = sum of the positive counts (or 1),
                documents without a positive count skipped
"""
import numpy as np

LD = np.longdouble


def weights(lam, topic_weights=None):
    """(pi, R) in longdouble."""
    lam = np.asarray(lam, dtype=LD)
    R = lam.sum(axis=1)
    if topic_weights is None:
        pi = R / R.sum()
    else:
        pi = np.asarray(topic_weights, dtype=LD).reshape(-1)
        pi = pi / pi.sum()
    return pi, R


def word_statistics(lam, topic_weights=None):
    """(p, D, S, scale) in longdouble; scale_w = sum_k |q_kw (log q_kw - log pi_k)|."""
    lam = np.asarray(lam, dtype=LD)
    pi, R = weights(lam, topic_weights)
    c = pi / R
    p = (c[:, None] * lam).sum(axis=0)
    q = c[:, None] * lam / p[None, :]
    terms = q * (np.log(q) - np.log(pi)[:, None])
    D = terms.sum(axis=0)
    return p, D, p * D, np.abs(terms).sum(axis=0)


def relevance(lam, weight, topic_weights=None):
    """The K x V matrix r in longdouble."""
    lam = np.asarray(lam, dtype=LD)
    _, R = weights(lam, topic_weights)
    p = word_statistics(lam, topic_weights)[0]
    return np.log(lam) - np.log(R)[:, None] - (LD(1) - LD(weight)) * np.log(p)[None, :]


def rank(values, top_n, relative):
    """(ids, scores, gap) of one row: the first ``top_n`` of np.lexsort((arange(V), -values)), their
    values, and the smallest gap between consecutive values among the first ``top_n + 1`` (absolute,
    or relative to the larger magnitude of the two); inf when there is a single value."""
    values = np.asarray(values, dtype=LD)
    V = values.size
    order = np.lexsort((np.arange(V), -values))
    head = values[order[:min(V, top_n + 1)]]
    gap = np.inf
    if head.size > 1:
        d = head[:-1] - head[1:]
        if relative:                                     # (two zeros: an exact tie, gap 0)
            big = np.maximum(np.abs(head[:-1]), np.abs(head[1:]))
            d = np.where(big > 0, d / np.where(big > 0, big, 1), 0)
        gap = float(d.min())
    return order[:top_n].astype(np.int32), values[order[:top_n]], gap


def relevant_words(lam, top_n, weight, topic_weights=None):
    """(ids K x top_n int32, scores K x top_n longdouble, smallest absolute gap over the rows)."""
    r = relevance(lam, weight, topic_weights)
    rows = [rank(r[k], top_n, relative=False) for k in range(r.shape[0])]
    return (np.stack([x[0] for x in rows]), np.stack([x[1] for x in rows]), min(x[2] for x in rows))


def salient_words(lam, top_n, topic_weights=None):
    """(ids, saliency, smallest relative gap)."""
    return rank(word_statistics(lam, topic_weights)[2], top_n, relative=True)


def prevalence(gamma, docs, weight_by_length=True):
    """pi in longdouble from gamma (K x B) and the documents (lists of (id, count) pairs); None when
    no document contributes."""
    gamma = np.asarray(gamma, dtype=LD)
    acc = np.zeros(gamma.shape[0], dtype=LD)
    used = 0
    for d, doc in enumerate(docs):
        n = sum(int(c) for _, c in doc if c > 0)
        if n <= 0:
            continue
        used += 1
        acc += (LD(n) if weight_by_length else LD(1)) * gamma[:, d] / gamma[:, d].sum()
    return acc / acc.sum() if used else None
