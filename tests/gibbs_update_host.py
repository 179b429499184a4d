"""NumPy restatement of the Gibbs update loops (a helper module, not a test file):
OnlineLDA.update_parameters / BatchLDA.update_parameters with inference_method='GIBBS'
(reference src/onlinelda.cpp:53-179, src/batchlda.cpp:43-61; csrc/gibbs_kernels.h,
gibbs_mstep_kernel).  Each E-step is gibbs_host.gibbs driven by the key the library drew for it;
the table it reads is exp(psi(lambda) - psi(rowsum(lambda))) of the batch's words, formed with the
digamma the caller passes (the oracle's), or the one the caller hands in for the last E-step.
Also the steps that follow an update (onlinelda.cpp:147-175): the adaptive learning rate and the
empirical-Bayes Newton step on eta.
"""
import math

import numpy as np

import gibbs_host


def csr(docs):
    indptr = np.zeros(len(docs) + 1, dtype=np.int32)
    ids, cnts = [], []
    for i, d in enumerate(docs):
        indptr[i + 1] = indptr[i] + len(d)
        ids += [w for w, _ in d]
        cnts += [c for _, c in d]
    return indptr, np.array(ids, dtype=np.int32), np.array(cnts, dtype=np.int32)


def table(lam, words, psi):
    """K x V: exp(psi(lambda) - psi(rowsum)) in the columns `words`, 0 elsewhere."""
    lam = np.asarray(lam, dtype=np.float64)
    e = np.zeros_like(lam)
    if len(words):
        ps = np.vectorize(psi, otypes=[np.float64])
        e[:, words] = np.exp(ps(lam[:, words]) - ps(lam.sum(axis=1))[:, None])
    return e


def _estep(lam, alpha, docs, theta0, num_samples, burn_in, key, psi, e=None):
    indptr, ids, cnts = csr(docs)
    if e is None:
        e = table(lam, np.unique(ids), psi)
    theta, counts, _ = gibbs_host.gibbs(e, alpha, indptr, ids, cnts, theta0, num_samples, burn_in, key)
    unit = 1.0 / num_samples if num_samples > 0 else 0.0
    return theta, counts * unit, e


def online(lam, alpha, eta, docs, num_documents, rho, max_iter_tr, init_theta, num_samples, burn_in,
           keys, psi, last_table=None):
    """One online update: returns (lambda, sstats of the last E-step, theta, its table, the lambda
    that E-step read).  `last_table`: the table of the last E-step, if the caller has the one the
    device read."""
    lam_p = np.array(lam, dtype=np.float64)
    K, V = lam_p.shape
    B = len(docs)
    scale = float(num_documents) / B
    if max_iter_tr > 0:
        indptr, ids, cnts = csr(docs)
        wc = np.bincount(ids, weights=np.maximum(cnts, 0), minlength=V).astype(np.float64)
        coef = float(num_documents) / B / K                                # onlinelda.cpp:86
        lam = (1. - rho) * lam_p + rho * (eta + coef * wc)[None, :]
        theta = None
        for i in range(max_iter_tr):                                       # onlinelda.cpp:89-101
            th0 = theta if (init_theta and i > 0) else None
            e = last_table if i + 1 == max_iter_tr else None
            seen = lam
            theta, sstats, e = _estep(lam, alpha, docs, th0, num_samples, burn_in, keys[i], psi, e)
            lam = (1. - rho) * lam_p + rho * (eta + scale * sstats)
        return lam, sstats, theta, e, seen
    theta, sstats, e = _estep(lam_p, alpha, docs, None, num_samples, burn_in, keys[0], psi, last_table)
    return (1. - rho) * lam_p + rho * (eta + scale * sstats), sstats, theta, e, lam_p    # :103-109


def batch(lam, alpha, eta, docs, max_epochs, num_samples, burn_in, keys, psi, last_table=None):
    """max_epochs x {fresh-theta E-step; lambda = eta + sstats} (batchlda.cpp:48-61); returns what
    online() returns."""
    lam = np.array(lam, dtype=np.float64)
    sstats = theta = e = seen = None
    for i in range(max_epochs):
        t = last_table if i + 1 == max_epochs else None
        seen = lam
        theta, sstats, e = _estep(lam, alpha, docs, None, num_samples, burn_in, keys[i], psi, t)
        lam = eta + sstats
    return lam, sstats, theta, e, seen


def online_rho(update_count, kappa, tau):
    """onlinelda.cpp:59-66."""
    return (tau + update_count) ** -kappa


def trigamma(x):
    """psi'(x), x > 0: the recurrence psi'(x) = psi'(x + 1) + 1 / x^2 up to x >= 20, then the
    asymptotic series (its first omitted term is below 1e-19 there)."""
    x = float(x)
    r = 0.0
    while x < 20.0:
        r += 1.0 / (x * x)
        x += 1.0
    f = 1.0 / (x * x)
    series = (1.0 / x + 0.5 * f + f / x * (1.0 / 6 - f * (1.0 / 30 - f * (1.0 / 42 - f * (1.0 / 30 - f * (
        5.0 / 66 - f * 691.0 / 2730))))))
    return r + series


def eta_step(lam, eta, rho, psi, min_eta=1e-6):
    """The stochastic Newton step on eta after an update (onlinelda.cpp:147-162), on the lambda the
    update left."""
    lam = np.asarray(lam, dtype=np.float64)
    K, N = lam.shape
    ps = np.vectorize(psi, otypes=[np.float64])
    g = ps(lam).sum() - N * ps(lam.sum(axis=1)).sum() - K * N * (psi(eta) - psi(N * eta))
    h = K * N * (trigamma(N * eta) - trigamma(eta))
    eta = eta - rho * g / h
    return max(eta, min_eta)


class Adaptive(object):
    """The adaptive learning rate (onlinelda.cpp:28-31, 61-62, 167-175): the state starts at
    tau = 1000, rho = 1 / tau, a squared norm of 1 and a zero running gradient."""

    def __init__(self, shape):
        self.tau = 1000.
        self.rho = 1. / self.tau
        self.sq_norm = 1.
        self.gradient = np.zeros(shape)

    def step(self, lambda_hat, lambda_prime):
        """after an update whose last E-step gave lambda_hat = eta + D / B sstats (eta before the
        update), lambda' the lambda before it"""
        upd = np.asarray(lambda_hat) - np.asarray(lambda_prime)
        t = self.tau
        self.gradient = (1. - 1. / t) * self.gradient + 1. / t * upd
        self.sq_norm = (1. - 1. / t) * self.sq_norm + 1. / t * float(np.sum(upd * upd))
        self.rho = float(np.sum(self.gradient * self.gradient)) / self.sq_norm
        self.tau = t * (1. - self.rho) + 1.
