"""NumPy restatement of the topic distances (LDA.topic_distances) in np.longdouble, by
the definitions: p_i = lambda_i / sum(lambda_i), q_j = mu_j / sum(mu_j);

    hellinger       sqrt(max(0, 1 - BC)),  BC = sum_v sqrt(p_iv q_jv)
    cosine          max(0, 1 - c),         c = sum_v p_iv q_jv / (|p_i| |q_j|)
    kl              sum_v p_iv log(p_iv / q_jv)
    jensen_shannon  H(m) - H(p_i) / 2 - H(q_j) / 2,  m = (p_i + q_j) / 2,  H(x) = -sum_v x_v log x_v

and, for each entry, A_ij = the sum of the absolute values of the terms of the sum the device forms,
which is what its rounding error scales with."""
import numpy as np

LD = np.longdouble
MEASURES = ("hellinger", "cosine", "kl", "jensen_shannon")


def topics(lam):
    lam = np.asarray(lam, dtype=LD)
    return lam / lam.sum(axis=1, keepdims=True)


def entropy(p):
    return -(p * np.log(p)).sum(axis=1)


def distances(lam, mu):
    """{measure: (D, A)}: the K x K' matrices in longdouble.  For hellinger D is the distance and the
    entry's BC is A; for cosine A is a tuple (c, numerator, |p_i|, |q_j|) -- c itself is what the
    bound scales with, the parts are returned as the definition's sum of terms."""
    lam, mu = np.asarray(lam, dtype=LD), np.asarray(mu, dtype=LD)
    p, q = topics(lam), topics(mu)
    K, K2 = p.shape[0], q.shape[0]
    S, T = lam.sum(axis=1), mu.sum(axis=1)
    lq, abs_lmu = np.log(q), np.abs(np.log(mu))
    nq, hq = np.sqrt((q * q).sum(axis=1)), entropy(q)
    bc, num, kl, a_kl, hm = (np.empty((K, K2), dtype=LD) for _ in range(5))
    for i in range(K):                                   # (row by row: K' x V temporaries)
        bc[i] = np.sqrt(p[i] * q).sum(axis=1)
        num[i] = (p[i] * q).sum(axis=1)
        kl[i] = (p[i] * np.log(p[i])).sum() - (p[i] * lq).sum(axis=1)
        a_kl[i] = ((lam[i] * np.abs(np.log(lam[i]))).sum() + (lam[i] * abs_lmu).sum(axis=1)) / S[i] + \
            np.abs(np.log(S[i])) + np.abs(np.log(T))
        m = (p[i] + q) / 2
        hm[i] = -(m * np.log(m)).sum(axis=1)
    n_p, hp = np.sqrt((p * p).sum(axis=1)), entropy(p)
    c = num / (n_p[:, None] * nq[None, :])
    return {"hellinger": (np.sqrt(np.maximum(0, 1 - bc)), bc),
            "cosine": (np.maximum(0, 1 - c), (c, num, n_p, nq)),
            "kl": (kl, a_kl),
            "jensen_shannon": (hm - hp[:, None] / 2 - hq[None, :] / 2, hm + hp[:, None] / 2 + hq[None, :] / 2)}


def greedy_match(D):
    """(match int64, dist float64) of the greedy one-to-one matching: repeatedly the smallest free
    entry in the order (distance, i, j)."""
    D = np.asarray(D, dtype=np.float64)
    K, K2 = D.shape
    match, dist = np.full(K, -1, dtype=np.int64), np.full(K, np.inf)
    rows, cols = set(range(K)), set(range(K2))
    while rows and cols:
        d, i, j = min((D[i, j], i, j) for i in rows for j in cols)
        match[i], dist[i] = j, d
        rows.remove(i)
        cols.remove(j)
    return match, dist


def min_gap(D):
    """The smallest difference between neighbouring values of the sorted entries."""
    s = np.sort(np.asarray(D, dtype=np.float64).ravel())
    return float(np.min(np.diff(s))) if s.size > 1 else float("inf")
