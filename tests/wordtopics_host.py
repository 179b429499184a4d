"""NumPy restatement of the per-word topic posteriors (csrc/wordtopics_kernels.h),
given lambda (K x V), gamma (K x B) and the batch's CSR: per entry p = (d, w_p, c_p), in entry order,

    s_pk   = exp(psi(gamma_dk) - psi(rs_k)) exp(psi(lambda_{k, w_p})),   rs_k = sum_v lambda_kv
    phi_pk = s_pk / sum_j s_pj

and the top_n topics of each row in decreasing phi, equal values by smaller topic id first.  The
counts play no part: an entry with c_p = 0 has a row like any other.  psi is scipy's, as in
elbo_host.py."""
import numpy as np
from scipy.special import psi


def posterior(indptr, ids, gamma, lam):
    """phi, entries x K."""
    indptr = np.asarray(indptr, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    gamma = np.asarray(gamma, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    K = lam.shape[0]
    gamma = gamma.reshape(K, len(indptr) - 1)
    doc = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    fac = np.exp(psi(gamma) - psi(lam.sum(axis=1))[:, None])          # K x B
    s = fac[:, doc].T * np.exp(psi(lam[:, ids])).T                   # entries x K
    return s / s.sum(axis=1)[:, None]


def rank(phi):
    """Per row the topic ids in the order (phi descending, id ascending): entries x K."""
    phi = np.asarray(phi, dtype=np.float64)
    n, K = phi.shape
    order = np.empty((n, K), dtype=np.int64)
    ids = np.arange(K)
    for p in range(n):
        order[p] = np.lexsort((ids, -phi[p]))
    return order


def gaps(ranked_probs, top_n):
    """Per row the smallest relative gap (p_r - p_{r+1}) / p_r between consecutive ranked
    probabilities among the first top_n + 1 (all K where there are fewer; inf for a single one):
    how far the row's top_n is from a different answer."""
    q = np.asarray(ranked_probs, dtype=np.float64)[:, :top_n + 1]
    if q.shape[1] < 2:
        return np.full(q.shape[0], np.inf)
    return np.min((q[:, :-1] - q[:, 1:]) / q[:, :-1], axis=1)


def word_topics(indptr, ids, gamma, lam, top_n):
    """(phi entries x K, topics entries x top_n int32, probs entries x top_n, gap entries)."""
    phi = posterior(indptr, ids, gamma, lam)
    order = rank(phi)
    ranked = np.take_along_axis(phi, order, axis=1)
    return phi, order[:, :top_n].astype(np.int32), ranked[:, :top_n], gaps(ranked, top_n)
