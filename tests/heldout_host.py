"""NumPy restatement of the held-out predictive log-likelihood (Hoffman et al. 2013), given gamma and
lambda: per document d

    loglik[d] = sum over the held-out entries (w, c) of c log sum_k (gamma_dk / sum_j gamma_dj)
                                                               (lambda_kw / sum_v lambda_kv)
    tokens[d] = sum of c

Entries with c = 0 add nothing; a document without held-out entries gets 0 and 0."""
import numpy as np


def score(indptr, ids, cnts, gamma, lam):
    """(loglik[B], tokens[B]) for the held-out CSR (indptr, ids, cnts), gamma K x B, lambda K x V."""
    indptr = np.asarray(indptr, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    cnts = np.asarray(cnts, dtype=np.float64)
    gamma = np.asarray(gamma, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    B = len(indptr) - 1
    doc = np.repeat(np.arange(B), np.diff(indptr))
    on = cnts != 0
    theta = gamma / gamma.sum(axis=0)                 # E[theta], K x B
    beta = lam / lam.sum(axis=1)[:, None]             # E[beta], K x V
    p = np.einsum("kn,kn->n", theta[:, doc[on]], beta[:, ids[on]])
    loglik = np.bincount(doc[on], weights=cnts[on] * np.log(p), minlength=B)
    tokens = np.bincount(doc, weights=cnts, minlength=B)
    return loglik, tokens


def per_word(indptr, ids, cnts, gamma, lam):
    loglik, tokens = score(indptr, ids, cnts, gamma, lam)
    return loglik.sum() / tokens.sum()
