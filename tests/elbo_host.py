"""NumPy/SciPy restatement of the variational lower bound as the library forms it (LDA::lowerBound,
lda.cpp:297-360, with the word's COLUMN of psi(lambda) read at :334: DESIGN.md 3.4), kept as its
separate terms so that a test can hold each part of the device result to its own bar.

With psiL = psi(lambda) (K x V), psiS_k = psi(sum_w lambda_kw), E_kw = psiL_kw - psiS_k and, per
document d, psiG_k = psi(gamma_dk), psiGS = psi(sum_k gamma_dk):

    dense    sum_kw (eta - lambda_kw) E_kw                                       (:317, eta part)
             + K lgamma(V eta) - sum_k lgamma(sum_w lambda_kw)                   (:356)
             - K V lgamma(eta) + sum_kw lgamma(lambda_kw)                        (:357)
    s_term   sum_kw sstats_kw E_kw                                               (:317, sstats part)
    pz       sum_d sum_{(w, c) in d} c sum_k [(psiG_k - psiGS) phi_k - phi_k log phi_k],
             phi = softmax_k(E_kw + psiG_k)                                      (:332-347)
    ptheta   sum_d sum_k [(alpha_k - gamma_dk)(psiG_k - psiGS) + lgamma(gamma_dk)]
             - lgamma(sum_k gamma_dk)                                            (:349-351)
    ptheta_const  (lgamma(sum alpha) - sum lgamma(alpha)) B                      (:355)

    bound(factor) = dense + factor (s_term + pz + ptheta + ptheta_const)         (:359)

`scale_dense` and `scale_batch` are the sums of the absolute values of every addend of the dense
and of the batch terms: the bound is small after cancellation, so tolerances are set against these.
Sums are math.fsum (exactly rounded), so the restatement's own error is that of psi / gammaln."""
import math

import numpy as np
from scipy.special import gammaln, psi


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel())


def _fsum_abs(a):
    return math.fsum(np.abs(np.asarray(a, dtype=np.float64)).ravel())


def terms(lam, alpha, eta, indptr, ids, cnts, gamma, sstats):
    """dict of the bound's terms for lambda K x V, alpha (K or scalar), the CSR batch, gamma K x B
    and sstats K x V (both the E-step's)."""
    lam = np.asarray(lam, dtype=np.float64)
    K, V = lam.shape
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64).ravel(), (K,))
    eta = float(eta)
    indptr = np.asarray(indptr, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    cnts = np.asarray(cnts, dtype=np.float64)
    gamma = np.asarray(gamma, dtype=np.float64).reshape(K, -1)
    sstats = np.asarray(sstats, dtype=np.float64)
    B = len(indptr) - 1
    assert gamma.shape == (K, B) and sstats.shape == (K, V)

    rows = np.array([math.fsum(r) for r in lam])          # sum_w lambda_kw
    E = psi(lam) - psi(rows)[:, None]                     # E[log beta]
    dense_eta = (eta - lam) * E
    lg_lam = gammaln(lam)
    consts = [K * gammaln(V * eta), -_fsum(gammaln(rows)), -K * V * gammaln(eta)]
    dense = math.fsum([_fsum(dense_eta), _fsum(lg_lam)] + consts)
    scale_dense = math.fsum([_fsum_abs(dense_eta), _fsum_abs(lg_lam)] + [abs(c) for c in consts])

    s_addends = sstats * E
    s_term = _fsum(s_addends)

    gsum = np.array([math.fsum(c) for c in gamma.T]) if B else np.zeros(0)
    psig = psi(gamma)                                     # K x B
    dpsig = psig - psi(gsum)[None, :]
    doc = np.repeat(np.arange(B), np.diff(indptr))
    pz_addends = np.zeros((0, K))
    if len(ids):
        phi = E[:, ids].T + psig[:, doc].T                # entries x K
        mx = phi.max(axis=1, keepdims=True)
        logp = phi - (mx + np.log(np.exp(phi - mx).sum(axis=1, keepdims=True)))
        p = np.exp(logp)
        pz_addends = cnts[:, None] * (dpsig[:, doc].T * p - p * logp)
    pz = _fsum(pz_addends)
    th_addends = [(alpha[:, None] - gamma) * dpsig, gammaln(gamma), -gammaln(gsum)]
    ptheta = math.fsum([_fsum(a) for a in th_addends])
    ptheta_const = (gammaln(math.fsum(alpha)) - _fsum(gammaln(alpha))) * B
    scale_batch = math.fsum([_fsum_abs(s_addends), _fsum_abs(pz_addends), abs(ptheta_const)] +
                            [_fsum_abs(a) for a in th_addends])
    return dict(dense=dense, s_term=s_term, pz=pz, ptheta=ptheta, ptheta_const=ptheta_const,
                scale_dense=scale_dense, scale_batch=scale_batch)


def batch_part(t):
    """the part that the factor multiplies: the slope of the bound in the factor"""
    return math.fsum([t["s_term"], t["pz"], t["ptheta"], t["ptheta_const"]])


def bound(t, factor=1.0):
    return math.fsum([t["dense"], factor * batch_part(t)])


def scale(t, factor=1.0):
    return t["scale_dense"] + abs(factor) * t["scale_batch"]


def lower_bound(lam, alpha, eta, indptr, ids, cnts, gamma, sstats, factor=1.0):
    """(bound, scale) in one call"""
    t = terms(lam, alpha, eta, indptr, ids, cnts, gamma, sstats)
    return bound(t, factor), scale(t, factor)
