"""NumPy restatement of the map of an indexed corpus (csrc/tsne_kernels.h): the
k-nearest-neighbour graph from given rows, the perplexity calibration, the symmetrisation, the exact
t-SNE gradient, its KL divergence and the loop, in float64 or np.longdouble; and the error bounds the
device is held to, each with its derivation.  u = 2^-53 throughout."""
import numpy as np

import docindex_host as dh

U = 2.0 ** -53


# ---- neighbours ---------------------------------------------------------------------------------
def ranking(rows):
    """(s N x N longdouble, order N x N) of the rows against themselves."""
    s = dh.similarities(rows, rows)
    return s, dh.rank(s)


def knn(rows, top_n, ranked=None):
    """(ids N x top_n int64, s N x top_n longdouble, gap N) of the rows against themselves: the total
    order (s descending, id ascending) with the row's own id taken out.  gap: the smallest non-zero
    gap between consecutive ranked similarities among the first top_n + 2 of the full order (an exact
    tie is ranked by id on both sides, so it is no near tie).  ``ranked``: the pair (s, order) of an
    earlier call's ``ranking(rows)``, to share it among several top_n."""
    s, order = ranking(rows) if ranked is None else ranked
    N = s.shape[0]
    ids = np.stack([o[o != i][:top_n] for i, o in enumerate(order)])
    ranked = np.take_along_axis(s, order, axis=1)[:, :top_n + 2]
    step = (ranked[:, :-1] - ranked[:, 1:]).astype(np.float64)
    step[step == 0] = np.inf
    return ids, np.take_along_axis(s, ids, axis=1), step.min(axis=1) if N > 1 else np.full(N, np.inf)


def distances(s):
    """D = max(0, 1 - s) in float64, as the device forms it from its own s."""
    return np.maximum(0.0, 1.0 - np.asarray(s, dtype=np.float64))


# ---- calibration --------------------------------------------------------------------------------
def offsets(D):
    """d_j = D_j - D_first in float64 (what the device subtracts), per row."""
    D = np.asarray(D, dtype=np.float64)
    return D - D[..., :1]


def entropy(beta, d):
    """(H, w, S, T) of one row at beta, in d's dtype: w = exp(-beta d), H = log S + beta T / S."""
    w = np.exp(-(beta * d))
    S = w.sum()
    T = (w * d).sum()
    return np.log(S) + beta * T / S, w, S, T


def entropy_slope(beta, d):
    """dH / dbeta = -beta Var_w(d) at beta."""
    _, w, S, T = entropy(beta, d)
    return -beta * ((w * d * d).sum() / S - (T / S) ** 2)


def calibrate_row(D, perplexity, dtype=np.float64):
    """(p, beta) of one row of sorted distances D: the contract of tsne_calibrate_kernel."""
    d = offsets(D).astype(dtype)
    k = d.shape[0]
    target = np.log(dtype(perplexity))
    if np.log(dtype(k)) <= target:
        return np.full(k, dtype(1) / dtype(k)), dtype(0)
    m = int(np.sum(d == 0))
    if m >= perplexity:
        return np.where(d == 0, dtype(1) / dtype(m), dtype(0)), dtype(np.inf)
    lo, hi = dtype(0), dtype(1) / (d.sum() / dtype(k))
    for _ in range(1100):
        if not entropy(hi, d)[0] > target:
            break
        lo, hi = hi, hi * dtype(2)
    for _ in range(200):
        if not hi - lo > hi * dtype(2.0 ** -50):
            break
        mid = dtype(0.5) * (lo + hi)
        if entropy(mid, d)[0] > target:
            lo = mid
        else:
            hi = mid
    _, w, S, _ = entropy(hi, d)
    return w / S, hi


def calibrate(D, perplexity, dtype=np.float64):
    """(p N x k, beta N) of the rows of D."""
    out = [calibrate_row(row, perplexity, dtype) for row in np.asarray(D, dtype=np.float64)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=dtype)


def p_bound(k, beta, dmax):
    """|p_dev - p| / p of a calibrated row, p recomputed in longdouble from the device's beta and d.
    The argument beta d_j is rounded once (u / 2 relative, that is beta d_j u / 2 absolute, which the
    exponential turns into a relative error) and exp is within 1 ulp = 2 u: w_j is within
    (beta d_j / 2 + 2) u.  S adds k positive terms, lane pairs first and then six levels: at most
    (k - 1) u on top of the terms' own error.  The quotient adds u / 2.  Numerator and denominator
    together: (k + 4 + beta dmax) u + second order <= (k + 8) u (1 + beta dmax): c = 8 covers the
    constants twice over, the reference's own rounding and the second-order terms."""
    return (k + 8) * U * (1.0 + float(beta) * float(dmax))


def entropy_bound(k, beta, d):
    """|H_dev(beta) - H(beta)|: log S inherits S's relative error (k + 3 + beta dmax) u as an absolute
    one and adds u |log S|; T = sum w_j d_j carries the same per-term error plus u / 2 for the product
    and (k - 1) u for the sum, beta T and the quotient u / 2 each and S's error again:
    (beta T / S) (2 k + 2 beta dmax + 8) u."""
    d = np.asarray(d, dtype=np.longdouble)
    H, w, S, T = entropy(np.longdouble(beta), d)
    bd = float(beta) * float(d.max())
    return float(U * ((k + 4 + bd) * (1.0 + abs(float(np.log(S)))) + float(beta * T / S) * (2 * k + 2 * bd + 8)))


def symmetrise(ids, p, dtype=np.float64):
    """P (dense N x N, dtype) = (p_{j|i} + p_{i|j}) / (2 N) of the conditional rows."""
    N, k = ids.shape
    cond = np.zeros((N, N), dtype=dtype)
    if k:
        cond[np.arange(N)[:, None], ids] = np.asarray(p).astype(dtype)
    return (cond + cond.T) / dtype(2 * N)


def dense(indptr, ids, p, dtype=np.float64):
    """A CSR as a dense N x N matrix."""
    N = len(indptr) - 1
    out = np.zeros((N, N), dtype=dtype)
    out[np.repeat(np.arange(N), np.diff(indptr)), ids] = np.asarray(p).astype(dtype)
    return out


# ---- gradient -----------------------------------------------------------------------------------
def gradient(Y, P, exaggeration=1.0, dtype=np.float64, parts=False):
    """(grad N x 2, kl) of the map Y under the dense affinities P; with ``parts=True`` also a dict of
    what the bounds need: Z, R, the absolute sums of the terms of R, A and KL."""
    y = np.asarray(Y).astype(dtype)
    P = np.asarray(P).astype(dtype)
    diff = y[:, None, :] - y[None, :, :]
    one = dtype(1) + (diff * diff).sum(axis=2)
    q = dtype(1) / one
    np.fill_diagonal(q, 0)
    Z = q.sum()
    R = ((q * q)[:, :, None] * diff).sum(axis=1)
    A = ((P * q)[:, :, None] * diff).sum(axis=1)
    grad = dtype(4) * (dtype(exaggeration) * A - R / Z)
    hit = P > 0
    terms = P[hit] * np.log(P[hit] * Z * one[hit])
    kl = terms.sum()
    if not parts:
        return grad, kl
    return grad, kl, {"Z": Z, "R": R, "absR": ((q * q)[:, :, None] * np.abs(diff)).sum(axis=1),
                      "absA": ((P * q)[:, :, None] * np.abs(diff)).sum(axis=1), "abskl": np.abs(terms).sum(),
                      "sumP": P.sum()}


def z_rel(N):
    """The relative error of Z on the device.  Every q is positive, so the error of the sum is at most
    (depth of the longest chain of additions an element passes through) u plus the terms' own: a
    stripe's chain is at most N / 64 + 16 long, then at most 64 stripes, N / 1024 + 1 elements of a
    tree thread, 6 wave levels and 16 waves: N / 32 + 110 covers it; q itself (two differences, two
    squares, two sums, one division) is within 3 u."""
    return (N / 32.0 + 110 + 3) * U


def gradient_bound(N, parts, exaggeration=1.0):
    """Per component |grad_dev - grad| against the longdouble restatement (``parts`` from it).
    A term q^2 dx of R is within 8 u (q 3 u, its square 6.5 u, dx and the product u / 2 each ... ), a
    term P q dx of A within 4.5 u; a sum of n terms added in ANY fixed order errs by at most (n - 1) u
    sum |term| on top: u (N + 10) sum_j |term_j| for both (c = 10).  R / Z carries Z's relative error
    z_rel(N) and the division's u / 2; exaggeration A, the difference and the factor 4 add at most
    2 u (|exaggeration A| + |R / Z|), taken into c = 12 since |sum| <= sum |term|."""
    Z = float(parts["Z"])
    absR = parts["absR"].astype(np.float64)
    absA = parts["absA"].astype(np.float64)
    return 4.0 * (abs(exaggeration) * U * (N + 12) * absA + absR / Z * (U * (N + 12) + z_rel(N)))


def kl_bound(N, parts):
    """|kl_dev - kl|: the argument (P Z)(1 + d^2) is within z_rel(N) + 3.5 u, the logarithm turns that
    into an absolute error and adds 1 ulp of its own, u |log|; times P (u / 2).  The sum of the terms,
    in any fixed order: (nnz - 1) u sum |term| at most, but no chain here is longer than a row's
    entries / 64 + 6 + N / 1024 + 22 < N + 12."""
    return float(parts["sumP"]) * (z_rel(N) + 4 * U) + U * (N + 12) * float(parts["abskl"])


# ---- loop ---------------------------------------------------------------------------------------
def learning_rate(N, early_exaggeration=12.0):
    return max(N / early_exaggeration / 4.0, 50.0)


def loop(Y0, P, num_iterations, exaggeration_iterations=250, early_exaggeration=12.0, lr=None,
         momentum=(0.5, 0.8), dtype=np.float64, trace=False):
    """(Y, kl per iteration) of the descent; with ``trace=True`` also the list of the ``same``
    decisions (bool N x 2 per iteration) and the list of the iterates before each update."""
    y = np.asarray(Y0).astype(dtype)
    N = y.shape[0]
    lr = dtype(learning_rate(N, early_exaggeration) if lr is None else lr)
    v = np.zeros_like(y)
    gain = np.ones_like(y)
    kls, sames, iterates = [], [], []
    for t in range(num_iterations):
        early = t < exaggeration_iterations
        g, kl = gradient(y, P, early_exaggeration if early else 1.0, dtype)
        kls.append(kl)
        same = (g > 0) == (v > 0)
        if trace:
            sames.append(same)
            iterates.append(y.copy())
        gain = np.maximum(np.where(same, gain * dtype(0.8), gain + dtype(0.2)), dtype(0.01))
        v = dtype(momentum[0] if early else momentum[1]) * v - lr * gain * g
        y = y + v
        y = y - y.sum(axis=0) / dtype(N)
    kls = np.array(kls, dtype=dtype)
    return (y, kls, sames, iterates) if trace else (y, kls)


def pca_axes(theta):
    """(mean, axes 2 x K) of theta (N x K): the leading eigenvectors of the scatter, signed so that
    the largest-magnitude component is positive."""
    theta = np.asarray(theta, dtype=np.float64)
    mean = theta.mean(axis=0)
    c = theta - mean
    w, V = np.linalg.eigh(c.T.dot(c))
    K = theta.shape[1]
    axes = np.zeros((2, K))
    for a in range(min(2, K)):
        e = V[:, K - 1 - a]
        axes[a] = e if e[np.argmax(np.abs(e))] > 0 else -e
    return mean, axes


def pca_start(theta):
    """The start of init='pca': the projection scaled so that the first column's standard deviation
    is 1e-4."""
    mean, axes = pca_axes(theta)
    y = (np.asarray(theta, dtype=np.float64) - mean).dot(axes.T)
    sd = y[:, 0].std()
    return y * (1e-4 / sd if sd > 0 else 0.0)


def theta_of(rows, measure="hellinger"):
    rows = np.asarray(rows, dtype=np.float64)
    return rows * rows if measure == "hellinger" else rows / rows.sum(axis=1)[:, None]


def affinities(rows, perplexity, dtype=np.float64):
    """Dense P of the rows: knn, calibration and symmetrisation."""
    N = rows.shape[0]
    k = min(N - 1, int(np.floor(3.0 * perplexity)))
    ids, s, _ = knn(rows, k)
    p, _ = calibrate(distances(s), perplexity, dtype)
    return symmetrise(ids, p, dtype)


def embed(rows, perplexity=30.0, num_iterations=750, measure="hellinger", dtype=np.float64, **kw):
    """The whole of ``DocumentIndex.embed`` with init='pca'."""
    P = affinities(rows, perplexity, dtype)
    return loop(pca_start(theta_of(rows, measure)), P, num_iterations, dtype=dtype, **kw)


# ---- cases --------------------------------------------------------------------------------------
def planted(N, seed, K=6):
    """(gamma K x N, group N): theta ~ Dirichlet with mass 6 and 3 on topics 2 g and 2 g + 1 of group
    g = i mod 3 and 0.2 elsewhere."""
    rng = np.random.RandomState(seed)
    group = np.arange(N) % 3
    alpha = np.full((N, K), 0.2)
    alpha[np.arange(N), 2 * group] = 6.0
    alpha[np.arange(N), 2 * group + 1] = 3.0
    theta = np.stack([rng.dirichlet(a) for a in alpha])
    return np.asfortranarray(theta.T), group


TRAJECTORY = {"num_iterations": 5, "exaggeration_iterations": 2}
TRAJECTORY_SIZES = (300, 65)
TRAJECTORY_PERPLEXITY = 10.0


def trajectory_case(N):
    """(gamma K x N, Y0 N x 2) of a trajectory case: planted groups and a Gaussian start of scale 1e-4."""
    gamma, _ = planted(N, 700 + N)
    return gamma, np.random.RandomState(900 + N).normal(0.0, 1e-4, size=(N, 2))


def separation(Y, group):
    """(purity, smallest distance between group centroids, largest member-to-centroid distance):
    purity is the share of documents whose nearest neighbour in the map is of their own group."""
    Y = np.asarray(Y, dtype=np.float64)
    d2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    purity = float(np.mean(group[np.argmin(d2, axis=1)] == group))
    cent = np.stack([Y[group == g].mean(axis=0) for g in np.unique(group)])
    between = min(np.linalg.norm(cent[a] - cent[b]) for a in range(len(cent)) for b in range(a))
    within = max(np.linalg.norm(Y[group == g] - cent[i], axis=1).max() for i, g in enumerate(np.unique(group)))
    return purity, float(between), float(within)
