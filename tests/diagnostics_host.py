"""The contract of csrc/diagnostics_kernels.h restated in NumPy ``longdouble``: what
the GPU tests compare against and what tests/test_diagnostics_host.py checks by hand, and the inputs
both files use.

    R_k = sum_w lambda_kw, beta_kw = lambda_kw / R_k, p_w as relevance_host.word_statistics
    eff_num_words = 1 / sum_w beta_kw^2;  word_entropy H_k = -sum_w beta_kw log beta_kw
    uniform_dist = log V - H_k;  corpus_dist = sum_w beta_kw (log beta_kw - log p_w)
    exclusivity = mean over the listed words of beta_kw / sum_j beta_jw
    per document with a positive count: N_d (or 1), theta_dk = gamma_dk / sum_j gamma_dj, a_dk = N_d theta_dk
    tokens T_k = sum_d a_dk;  document_entropy = log T_k - (sum_d a_dk log a_dk) / T_k
    rank_1_docs: the smallest k with the largest gamma_dk;  docs_high, docs_low: theta_dk > high, > low
"""
from fractions import Fraction

import numpy as np

import relevance_host as vh

LD = np.longdouble
U = 2.0 ** -53


def top_words(lam, top_n):
    lam = np.asarray(lam)
    V = lam.shape[1]
    return np.stack([np.lexsort((np.arange(V), -row))[:top_n] for row in lam]).astype(np.int32)


def exclusivity(lam, words):
    """The mean over each row of ``words`` (K x n ids) of beta_kw / sum_j beta_jw, in longdouble."""
    lam = np.asarray(lam, dtype=LD)
    beta = lam / lam.sum(axis=1)[:, None]
    u = beta.sum(axis=0)
    return np.array([(beta[k, row] / u[row]).mean() for k, row in enumerate(np.asarray(words))], dtype=LD)


def word_side(lam, top_n=10, topic_weights=None, words=None):
    """The word-side dict in longdouble, plus what the error bounds scale with: ``scale_corpus`` =
    sum_w |beta (log beta - log p)| per topic and ``L`` = the largest |log| met."""
    lam = np.asarray(lam, dtype=LD)
    K, V = lam.shape
    R = lam.sum(axis=1)
    beta = lam / R[:, None]
    logl, logp = np.log(lam), np.log(vh.word_statistics(lam, topic_weights)[0])
    logb = logl - np.log(R)[:, None]
    H = -(beta * logb).sum(axis=1)
    terms = beta * (logb - logp[None, :])
    words = top_words(lam, top_n) if words is None else np.asarray(words)
    L = float(max(np.abs(x).max() for x in (logl, np.log(R), logb, logp)))
    return {"eff_num_words": 1 / (beta * beta).sum(axis=1), "word_entropy": H, "uniform_dist": np.log(LD(V)) - H,
            "corpus_dist": terms.sum(axis=1), "exclusivity": exclusivity(lam, words), "top_words": words,
            "scale_corpus": np.abs(terms).sum(axis=1), "L": L}


def theta_bound(K):
    """|theta_dev - theta| / theta, first order: K - 1 additions, a division and a product."""
    return (K + 1) * U


def document_side(gamma, docs, weight_by_length=True, high=0.5, low=0.02):
    """The document-side dict in longdouble (counts int64; None when no document contributes), plus
    ``near`` -- the (document, topic, what) whose theta lies within theta_bound of a threshold, and
    the documents whose two largest gamma differ, but by less than that bound relatively: where the
    device may count differently -- and ``scales`` for the entropy's error bound: per topic
    (sum_d a (|log a| + 1) / T, sum_d |a log a| / T)."""
    gamma = np.asarray(gamma, dtype=LD)
    K = gamma.shape[0]
    T, A = np.zeros(K, dtype=LD), np.zeros(K, dtype=LD)
    s1, s2 = np.zeros(K, dtype=LD), np.zeros(K, dtype=LD)
    rank1, above, present = (np.zeros(K, dtype=np.int64) for _ in range(3))
    near, used = [], 0
    tb = theta_bound(K)
    for d, doc in enumerate(docs):
        n = sum(int(c) for _, c in doc if c > 0)
        if n <= 0:
            continue
        used += 1
        g = gamma[:, d]
        theta = g / g.sum()
        a = (LD(n) if weight_by_length else LD(1)) * theta
        T += a
        A += a * np.log(a)
        s1 += a * (np.abs(np.log(a)) + 1)
        s2 += np.abs(a * np.log(a))
        best = int(np.argmax(g))                              # (the first of equal values)
        rank1[best] += 1
        if K > 1:
            second = np.delete(g, best).max()
            if 0 < (g[best] - second) / g[best] < tb:
                near.append((d, best, "rank"))
        for name, thr, counts in (("high", high, above), ("low", low, present)):
            counts += theta > thr
            for k in np.nonzero(np.abs(theta - LD(thr)) <= tb * theta)[0]:
                near.append((d, int(k), name))
    if not used:
        return None
    ratio = np.full(K, np.nan)
    ratio[present > 0] = above[present > 0] / present[present > 0]
    return {"tokens": T, "document_entropy": np.log(T) - A / T, "rank_1_docs": rank1, "docs_high": above,
            "docs_low": present, "allocation_ratio": ratio, "num_docs": used, "near": near,
            "scales": (s1 / T, s2 / T)}


def _fma(a, b, c):
    """fl(a b + c) of three doubles, one rounding."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def tokens_device_order(gamma, docs, weight_by_length=True):
    """T in fp64 exactly as the device forms it (the prevalence sums before normalisation): each
    document's sum_j gamma_dj lane-local over j = lane, lane + 64, ... then the butterfly over xor
    32 .. 1, inv = 1 / sum, and acc_k = fma(fl(N_d gamma_dk), inv, acc_k) over the documents in order."""
    gamma = np.asarray(gamma, dtype=np.float64)
    K = gamma.shape[0]
    acc = [0.0] * K
    lanes = np.arange(64)
    for d, doc in enumerate(docs):
        n = sum(int(c) for _, c in doc if c > 0)
        if n <= 0:
            continue
        g = gamma[:, d]
        part = np.zeros(64)
        for k in range(K):
            part[k % 64] += g[k]
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[lanes ^ off]
        inv = 1.0 / part[0]
        nd = float(n) if weight_by_length else 1.0
        for k in range(K):
            acc[k] = _fma(nd * g[k], inv, acc[k])
    return np.array(acc)


def normalise(tokens):
    """tokens / their sum as the library's prevalence read-out forms it: the sum in long double in
    topic order, one rounding per quotient."""
    total = LD(0)
    for t in tokens:
        total += LD(t)
    return (np.asarray(tokens, dtype=LD) / total).astype(np.float64)


# -- the inputs of tests/test_gpu_diagnostics.py (test_diagnostics_host.py checks their near lists) --
WORD_TOPICS = (1, 3, 64, 65, 100, 513)
WORD_VOCABS = (1, 5, 255, 256, 257, 1025)                 # (the chunk of 256: below, at, past; five chunks)
DOC_TOPICS = (3, 64, 65, 513)
DOC_V, DOC_B = 400, 33


def lam(K, V, seed=0):
    return np.random.RandomState(9000 + 17 * K + V + seed).gamma(0.3, 1.0, size=(K, V)) + 0.01


def given(K):
    return np.random.RandomState(31 + K).gamma(0.5, 1.0, K) + 0.01


def documents(negative=True, seed=0):
    """DOC_B documents over DOC_V words: document 1 empty, document 2 of one token, document 3 with
    counts <= 0 only (a negative one only where no E-step sees it), document 4 of 300 entries, the
    others of 1 .. 13 entries with counts 0 .. 7 and repeated ids."""
    rng = np.random.RandomState(600 + seed)
    docs = [[(int(rng.randint(DOC_V)), int(rng.randint(0, 8))) for _ in range(rng.randint(1, 14))]
            for _ in range(DOC_B)]
    docs[0] = [(3, 2), (3, 1), (1, 4)]
    docs[1] = []
    docs[2] = [(DOC_V - 1, 1)]
    docs[3] = [(2, 0), (5, -3 if negative else 0)]
    docs[4] = [(int(w), int(rng.randint(1, 8))) for w in rng.permutation(DOC_V)[:300]]
    return docs


def gammas(K, seed=0):
    """K x DOC_B: every third document has one topic at 1.5 times the sum of the others (theta near
    0.6, above `high`), at large K many theta lie below 0.02; document 5 has its two largest values
    exactly equal where K > 1 (the smaller topic ranks first)."""
    rng = np.random.RandomState(700 + K + seed)
    g = rng.gamma(0.3, 1.0, size=(K, DOC_B)) + 0.01
    g = np.asfortranarray(g * rng.uniform(0.5, 40.0, size=DOC_B))
    for d in range(0, DOC_B, 3):
        k = rng.randint(K)
        g[k, d] = 1.5 * (g[:, d].sum() - g[k, d])
    if K > 1:
        hi = int(np.argmax(g[:, 5]))
        g[(hi + 1) % K, 5] = g[hi, 5]
    return g
