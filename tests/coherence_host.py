"""NumPy restatement of topic coherence: presence as a dense boolean matrix, the
counts as P.T @ P, and UMass (Mimno et al. 2011, as a mean) and NPMI (Bouma 2009, document level)
pair by pair in the order m ascending, then l ascending.

Document d contains word w when it has an entry (w, c) with c > 0."""
import math

import numpy as np


def presence(indptr, ids, cnts, V):
    """B x V bool: document d contains word w."""
    indptr = np.asarray(indptr, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    cnts = np.asarray(cnts)
    B = len(indptr) - 1
    P = np.zeros((B, V), dtype=bool)
    doc = np.repeat(np.arange(B), np.diff(indptr))
    on = cnts > 0
    P[doc[on], ids[on]] = True
    return P


def counts(P, words):
    """(doc_freq T x N, co_doc_freq T x N x N, M) of the word lists `words` (T x N)."""
    words = np.asarray(words, dtype=np.int64)
    Pi = P.astype(np.int64)
    full = Pi.T @ Pi                                  # V x V documents containing both
    co = full[words[:, :, None], words[:, None, :]]
    doc_freq = np.diagonal(full)[words]
    return doc_freq, co, P.shape[0]


def umass(doc_freq, co):
    out = np.empty(len(doc_freq))
    for t in range(len(doc_freq)):
        s, used = 0.0, 0
        N = doc_freq.shape[1]
        for m in range(1, N):
            for l in range(m):
                if doc_freq[t, l] == 0:
                    continue
                s += math.log((co[t, m, l] + 1) / doc_freq[t, l])
                used += 1
        out[t] = s / used if used else math.nan
    return out


def npmi(doc_freq, co, M):
    out = np.empty(len(doc_freq))
    for t in range(len(doc_freq)):
        s = 0.0
        N = doc_freq.shape[1]
        for j in range(1, N):
            for i in range(j):
                dij = int(co[t, i, j])
                if dij == 0:
                    s += -1.0
                elif dij == M:
                    s += 1.0
                else:
                    s += (math.log(dij) + math.log(M) - math.log(doc_freq[t, i]) - math.log(doc_freq[t, j])) \
                        / (math.log(M) - math.log(dij))
        out[t] = s / (N * (N - 1) // 2)
    return out


def coherence(measure, doc_freq, co, M):
    return umass(doc_freq, co) if measure == "umass" else npmi(doc_freq, co, M)


def top_words(lam, top_n):
    """Row k: np.lexsort((arange(V), -lam[k]))[:top_n]."""
    lam = np.asarray(lam, dtype=np.float64)
    V = lam.shape[1]
    return np.stack([np.lexsort((np.arange(V), -row))[:top_n] for row in lam]).astype(np.int32)
