"""The contract of csrc/wordsim_kernels.h restated in NumPy ``longdouble``: what the
GPU tests compare against and what tests/test_wordsim_host.py checks by hand.

    R_k = sum_v lambda_kv
    pi: None -> R_k / sum_j R_j; else the given weights / their sum
    c_k = pi_k / R_k,  a_kw = c_k lambda_kw,  p_w = sum_k a_kw,  p(k | w) = a_kw / p_w
    row of word w:  hellinger  r_wk = sqrt(p(k | w));  cosine  r_wk = a_kw / sqrt(sum_j a_jw^2)
    s(q, w) = sum_k r_qk r_wk;  distance sqrt(max(0, 1 - s)) (hellinger), max(0, 1 - s) (cosine)
    ranking: the total order (s descending, word id ascending), the query word left out by id
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def coefficients(lam, topic_weights=None):
    """c in longdouble."""
    lam = np.asarray(lam, dtype=LD)
    R = lam.sum(axis=1)
    if topic_weights is None:
        pi = R / R.sum()
    else:
        pi = np.asarray(topic_weights, dtype=LD).reshape(-1)
        pi = pi / pi.sum()
    return pi / R


def proportions(lam, topic_weights=None, words=None):
    """p(k | w), K x V (or K x len(words)), longdouble."""
    lam = np.asarray(lam, dtype=LD)
    a = coefficients(lam, topic_weights)[:, None] * lam
    if words is not None:
        a = a[:, np.asarray(words, dtype=np.int64)]
    return a / a.sum(axis=0)[None, :]


def rows(lam, measure="hellinger", topic_weights=None):
    """The unit rows of all words, V x K, longdouble."""
    lam = np.asarray(lam, dtype=LD)
    a = (coefficients(lam, topic_weights)[:, None] * lam).T
    if measure == "hellinger":
        return np.sqrt(a / a.sum(axis=1)[:, None])
    if measure == "cosine":
        return a / np.sqrt((a * a).sum(axis=1))[:, None]
    raise ValueError(measure)


def proportion_rows(props, measure="hellinger"):
    """The unit rows of K x B proportions (any positive scale), B x K, longdouble."""
    g = np.asarray(props, dtype=LD)
    g = g.reshape(g.shape[0], -1)
    theta = (g / g.sum(axis=0)).T
    if measure == "hellinger":
        return np.sqrt(theta)
    if measure == "cosine":
        return theta / np.sqrt((theta * theta).sum(axis=1))[:, None]
    raise ValueError(measure)


def similarities(qrows, wrows):
    """s, B x V, longdouble."""
    return np.asarray(qrows, dtype=LD).dot(np.asarray(wrows, dtype=LD).T)


def search(qrows, wrows, top_n, self_ids=None):
    """(ids B x top_n int32, s B x top_n longdouble, gap): per query the first ``top_n`` words in the
    order (s descending, id ascending), word ``self_ids[b]`` left out of query b's candidates (None,
    or an entry of -1: nothing is left out), and the smallest gap between consecutive ranked
    similarities among the first ``top_n + 1`` over all queries (inf when no query has two)."""
    return search_s(similarities(qrows, wrows), top_n, self_ids)


def search_s(s, top_n, self_ids=None):
    """``search`` from the B x V similarities themselves."""
    B, V = s.shape
    ids = np.empty((B, top_n), dtype=np.int32)
    out = np.empty((B, top_n), dtype=LD)
    gap = np.inf
    for b in range(B):
        cand = np.arange(V)
        if self_ids is not None and self_ids[b] >= 0:
            cand = cand[cand != self_ids[b]]
        order = cand[np.lexsort((cand, -s[b, cand]))]
        head = s[b, order[:top_n + 1]]
        if head.size > 1:
            gap = min(gap, float(np.min(head[:-1] - head[1:])))
        ids[b] = order[:top_n]
        out[b] = s[b, order[:top_n]]
    return ids, out, gap


def distance(s, measure="hellinger"):
    rest = np.maximum(0.0, 1.0 - np.asarray(s, dtype=np.float64))
    return np.sqrt(rest) if measure == "hellinger" else rest


def prop_bound(K, V=0, given=True):
    """|p_dev(k | w) - p(k | w)| / p(k | w), first order: a_kw is off by e_a (``sim_bound``), the sum
    p_w by e_a and the depth of its additions -- a lane adds ceil(K / 64) terms in turn, the
    butterfly six levels more --, then the division."""
    e_a = (V + 1 if given else 2) + 1
    return (2 * e_a + (K + 63) // 64 - 1 + 6 + 1) * U


def sim_bound(K, measure, V=0, given=True):
    """|s_dev - s| / s, first order, from the order of operations documented in
    csrc/wordsim_kernels.h; every term of every sum is positive, so relative errors of the terms
    bound the relative error of a sum.  In units of u = 2^-53:

    c_k.  Whatever relative error is common to all k cancels in both measures (a row is invariant
    under a scaling of c), so only the part that varies with k counts.  Given weights: pi_k's
    rounding (1), R_k's V - 1 additions (V - 1, in the worst case), the division (1): V + 1.
    Default weights: c_k = fl(fl(R_k / S) / R_k); S is common, R_k's own error cancels between the
    two divisions, which leave 2.  Both within V + 1 (pass V = 0 to leave R_k's part out).
    a_kw: the multiply, 1.  So each a_kw is off by at most e_a = V + 2.

    hellinger.  t = sqrt(a): e_a / 2 + 1.  n_w = sum_k a_kw: e_a from its terms, K - 1 additions at
    most (the wave's order adds ceil(K / 64) - 1 + 6 deep, K - 1 bounds it); z_w = 1 / sqrt(n_w):
    (e_a + K - 1) / 2 + 1 (the root) + 1 (the division).  Each product t_qk t_wk inside the MFMA
    carries 2 (e_a / 2 + 1); the chain of ceil(K / 4) steps adds at most ceil(K / 4) + 3 roundings
    (one per step, and up to three inside a step were the four products added one by one).  The
    scales: 2 ((e_a + K - 1) / 2 + 2), their product 1, the final multiply 1.
      total: 2 e_a + K + ceil(K / 4) + 10.
    (the common-factor cancellation is not used here for e_a in t against e_a in z, which would
    leave less: the bound stays first order and simple.)

    cosine.  t = a: e_a.  n_w = sum_k fl(a^2): 2 e_a + 1 per term, K - 1 additions; z_w:
    (2 e_a + 1 + K - 1) / 2 + 2.  Products: 2 e_a; chain: ceil(K / 4) + 3; scales: 2 z, their
    product 1, the final multiply 1.
      total: 4 e_a + K + ceil(K / 4) + 9.

    The restatement itself is longdouble (u_ld = 2^-64, K terms): K 2^-11 u, rounded up to 1 u for
    every K here.  s <= 1 up to this bound, so it serves as an absolute bound too."""
    e_a = (V + 1 if given else 2) + 1
    chain = (K + 3) // 4 + 3
    if measure == "hellinger":
        return (2 * e_a + K + chain + 7 + 1) * U
    if measure == "cosine":
        return (4 * e_a + K + chain + 6 + 1) * U
    raise ValueError(measure)
