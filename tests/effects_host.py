"""NumPy restatement of topic prevalence against document metadata (csrc/effects_kernels.h, DESIGN.md
3.34).  theta^ is tests/topicdocs_host.theta_hat of the stored rows, so on the device's own rows it is
the device's bit for bit.  On it:

  the group passes in the device's order, in float64: a group's members by ascending id in chunks of
  CHUNK = 256, the terms of a chunk one after the other from 0.0, the chunk sums in ascending order, one
  division -- what the device gives bit for bit;
  the same sums, the Gram matrix, the cross products and the residual sums of squares in np.longdouble,
  each with the sum of the absolute terms that a rounding error scales with;
  the bounds the GPU tests hold the device to."""
import numpy as np

import topicdocs_host as th

LD = np.longdouble
U = 2.0 ** -53
CHUNK = 256                                   # kClusterChunkRows
BLOCK = 64                                    # kEffectsBlockDocs
theta_hat = th.theta_hat


# -- the group passes, in the device's order -------------------------------------------------------------
def group_pass(theta, labels, G, weights=None, mean=None):
    """(sums K x G, W G) in float64 and the device's order.  Without `mean` the terms are w theta (theta
    without weights) and W_g the sum of the weights (the member count without); with `mean` (K x G)
    they are (w q) q, q = theta - mean_g (q q without weights), and W is None."""
    theta = np.asarray(theta, dtype=np.float64)
    labels = np.asarray(labels)
    K = theta.shape[1]
    out, W = np.zeros((K, G)), np.zeros(G)
    for g in range(G):
        ids = np.flatnonzero(labels == g)                # ascending: the sort is stable
        total, wtotal = np.zeros(K), 0.0
        for c0 in range(0, len(ids), CHUNK):
            part, wpart = np.zeros(K), 0.0
            for d in ids[c0:c0 + CHUNK]:
                if mean is None:
                    term = theta[d] if weights is None else weights[d] * theta[d]
                else:
                    q = theta[d] - mean[:, g]
                    term = q * q if weights is None else (weights[d] * q) * q
                part = part + term
                if weights is not None:
                    wpart = wpart + weights[d]
            if weights is None:
                wpart = float(len(ids[c0:c0 + CHUNK]))
            total, wtotal = total + part, wtotal + wpart
        out[:, g], W[g] = total, wtotal
    return out, (W if mean is None else None)


def group_prevalence(theta, labels, G, weights=None, ddof=1):
    """(mean K x G, counts G int64, variance K x G) as DocumentIndex.group_prevalence returns them."""
    labels = np.asarray(labels)
    S, W = group_pass(theta, labels, G, weights)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = S / W[None, :]
    counts = np.array([np.count_nonzero(labels == g) for g in range(G)], dtype=np.int64)
    SS, _ = group_pass(theta, labels, G, weights, mean)
    if weights is None:
        n = counts.astype(np.float64)
    else:
        n = np.array([np.count_nonzero((labels == g) & (np.asarray(weights) > 0)) for g in range(G)], dtype=np.float64)
    rest = n - ddof
    with np.errstate(divide="ignore", invalid="ignore"):
        var = SS / rest[None, :] if weights is None else (SS / W[None, :]) * n[None, :] / rest[None, :]
    var[:, ~(rest > 0)] = np.nan
    return mean, counts, var


def group_exact(theta, labels, G, weights=None, centre=None):
    """In longdouble: (mean K x G, A K x G, SS K x G, B K x G, W G, n G).  A_gk = sum |w theta| / W, what
    an error of the mean scales with; SS is taken about `centre` (K x G; default: the longdouble mean) and
    B_gk = sum |w q q| = SS.  n: the members."""
    t = np.asarray(theta, dtype=np.float64).astype(LD)
    labels = np.asarray(labels)
    K = t.shape[1]
    w = np.ones(t.shape[0], dtype=LD) if weights is None else np.asarray(weights, dtype=np.float64).astype(LD)
    mean, A, SS = np.full((K, G), np.nan, dtype=LD), np.zeros((K, G), dtype=LD), np.zeros((K, G), dtype=LD)
    W, n = np.zeros(G, dtype=LD), np.zeros(G, dtype=np.int64)
    for g in range(G):
        ids = np.flatnonzero(labels == g)
        n[g] = len(ids)
        W[g] = w[ids].sum()
        if W[g] > 0:
            mean[:, g] = (w[ids, None] * t[ids]).sum(axis=0) / W[g]
            A[:, g] = np.abs(w[ids, None] * t[ids]).sum(axis=0) / W[g]
        c = mean[:, g] if centre is None else np.asarray(centre)[:, g].astype(LD)
        q = t[ids] - c[None, :]
        SS[:, g] = (w[ids, None] * q * q).sum(axis=0)
    return mean, A, SS, SS.copy(), W, n


def group_mean_bound(A, n):
    """|mean_dev - mean_longdouble|: any order of n additions errs by (n - 1) u sum |terms|, each term
    carries u from its multiply by w, the division and the sum of the weights add about 2 u, and the
    allowance of 16 covers the longdouble side: (n + 16) 2 u sum |w theta| / W."""
    return (np.asarray(n, dtype=np.float64)[None, :] + 16) * 2 * U * np.asarray(A, dtype=np.float64)


def group_ss_bound(B, n):
    """|SS_dev - SS_longdouble| with both about the device's mean: a term (w q) q carries u from the
    subtraction in each q and u from each multiply, 4 u, and the n additions (n - 1) u: the matching form
    (n + 16) 4 u sum |w q q|."""
    return (np.asarray(n, dtype=np.float64)[None, :] + 16) * 4 * U * np.asarray(B, dtype=np.float64)


# -- the regression -----------------------------------------------------------------------------------------
def design(X, intercept=True):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    return np.hstack([np.ones((X.shape[0], 1)), X]) if intercept else X.copy()


def products(theta, Z, weights=None):
    """(G, AG, C, AC) in longdouble: G = Z^T W Z, C = Z^T W theta and the sums of their absolute terms."""
    t = np.asarray(theta, dtype=np.float64).astype(LD)
    z = np.asarray(Z, dtype=np.float64).astype(LD)
    wz = z if weights is None else np.asarray(weights, dtype=np.float64).astype(LD)[:, None] * z
    return wz.T.dot(z), np.abs(wz).T.dot(np.abs(z)), wz.T.dot(t), np.abs(wz).T.dot(np.abs(t))


def products_bound(A, N):
    """|dev - longdouble| of an element of G or C: any order of N additions errs by (N - 1) u sum
    |terms|, and each term carries about 2 u from w z and the product: (N + 16) 4 u sum_d |terms|, the
    scatter's form (tests/test_gpu_topicdocs.py)."""
    return (N + 16) * 4 * U * np.asarray(A, dtype=np.float64)


def residuals(theta, Z, coef, weights=None):
    """(rss K, E K) in longdouble for the float64 coefficients `coef` (P x K): rss_k = sum_d w_d r_dk^2,
    r = theta - Z coef, and the first-order rounding bound E of the device's rss (rss_bound)."""
    t = np.asarray(theta, dtype=np.float64).astype(LD)
    z = np.asarray(Z, dtype=np.float64).astype(LD)
    b = np.asarray(coef, dtype=np.float64).astype(LD)
    N, P = z.shape
    w = np.ones(N, dtype=LD) if weights is None else np.asarray(weights, dtype=np.float64).astype(LD)
    r = t - z.dot(b)
    rss = (w[:, None] * r * r).sum(axis=0)
    return rss, rss_bound(P, N, np.abs(z).dot(np.abs(b)), r, w, rss)


def rss_bound(P, N, absfit, r, w, rss):
    """First order in u = 2^-53.  fit is a sum of P products in some order: it errs by at most
    (P + 4) u sum_p |z b| =: e (the 4: the chain's zero tail and its grouping by four).  r^ = theta - fit^
    rounds once more: |dr| <= e + u |r|.  The term (w r^) r^ carries two more roundings:
    |d term| <= 2 w |r| |dr| + 2 u w r^2 <= 2 w |r| e + 4 u w r^2.  The N terms are added in some order:
    (N - 1) u sum w r^2.  Together, with the allowance of 16 for the longdouble side,
        E_k = 2 (P + 4) u sum_d w_d |r_dk| sum_p |z_dp b_pk|  +  (N + 16) u sum_d w_d r_dk^2."""
    first = 2 * (P + 4) * U * (w[:, None] * np.abs(r) * absfit).sum(axis=0)
    return (first + (N + 16) * U * rss).astype(np.float64)


def lstsq(theta, Z, weights=None):
    """float64 np.linalg.lstsq on Z sqrt(w): (coef P x K, rss K)."""
    t = np.asarray(theta, dtype=np.float64)
    z = np.asarray(Z, dtype=np.float64)
    s = np.ones(len(z)) if weights is None else np.sqrt(np.asarray(weights, dtype=np.float64))
    coef = np.linalg.lstsq(z * s[:, None], t * s[:, None], rcond=None)[0]
    r = (t - z.dot(coef)) * s[:, None]
    return coef, (r * r).sum(axis=0)


def equilibrated(G):
    """(A = D G D, d) with D = diag(G)^-1/2, float64."""
    G = np.asarray(G, dtype=np.float64)
    d = 1.0 / np.sqrt(np.diag(G))
    return G * d[:, None] * d[None, :], d


def coef_bound(G, bound_G, bound_C, coef, cond_max):
    """|beta_dev - beta_lstsq|_2 per topic in the equilibrated coordinates beta = coef / d, first order.
    The device's sums differ from the exact ones by dA = D dG D and dc = D dC (products_bound), so the
    solution of the normal equations moves by A^-1 (dc - dA beta): at most (|dc|_2 + |dA|_F |beta|_2) /
    lambda_min, and 1 / lambda_min <= cond_max / lambda_max with the condition number the test asserts.
    Solving A in float64 (LU) adds about P u cond |beta|, and lstsq's own error on Z sqrt(w) is of the
    same order at most (its condition number is sqrt(cond)); 64 P u cond_max |beta|_2 covers both."""
    A, d = equilibrated(G)
    P = A.shape[0]
    lam_max = float(np.linalg.eigvalsh(A)[-1])
    beta = np.asarray(coef) / d[:, None]
    dA = np.linalg.norm(np.asarray(bound_G) * d[:, None] * d[None, :])
    dc = np.linalg.norm(np.asarray(bound_C) * d[:, None], axis=0)
    nb = np.linalg.norm(beta, axis=0)
    return cond_max / lam_max * (dc + dA * nb) + 64 * P * U * cond_max * nb
