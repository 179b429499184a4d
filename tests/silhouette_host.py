"""NumPy restatement of the silhouette of an indexed corpus (csrc/silhouette_kernels.h)
in np.longdouble on the index's stored rows x (N x K, unit length):

    d(i, j)       sqrt(max(0, 1 - s_ij)) (hellinger) or max(0, 1 - s_ij) (cosine), s_ij = <x_i, x_j>
    a(i)          sum_{j in own, j != i} d(i, j) / (n_own - 1); 0 where n_own = 1
    mean(i, c)    sum_{j in c} d(i, j) / n_c for the non-empty c != own
    b(i)          the smallest mean; neighbour(i) the first c in the order (mean ascending, c ascending)
    s(i)          (b - a) / max(a, b); 0 where n_own = 1 or max(a, b) = 0

with the pair (i, i) left out by id; the error bounds of the device's figures, per scored document
(u = 2^-53, e = (K + 16) u the bound of s_ij as in DESIGN.md 3.26, x = 1 - s_ij from longdouble):

    pair          e + u (cosine); min(sqrt(e + u), (e + u) / sqrt(x)) + u sqrt(x) (hellinger: the root of
                  a value off by e + u moves by at most either, and is rounded once)
    mean over n   the mean of the pair bounds + (ceil(n / 16) + 8) u mean: a lane adds ceil(n / 16)
                  values, the tree four more, then the division; 8 covers those and the second order
    silhouette    2 (da + db) / max(a, b) + 4 u

and the near-tie report: per document the gap between the smallest and the second-smallest mean over
the other clusters (inf where there is only one), which says how far `neighbour` is from another
answer; `gap_bound` is the larger of those two means' bounds.

Also the inputs tests/test_silhouette_host.py and tests/test_gpu_silhouette.py share: gammas around
planted Dirichlet centres and the labels of one nearest-centroid assignment."""
import numpy as np

import cluster_host as ch
import docindex_host as dh

LD = np.longdouble
U = 2.0 ** -53
MEASURES = ["hellinger", "cosine"]
KS = [1, 3, 15, 16, 17, 63, 65, 130]
NCS = [(300, 2), (300, 7), (300, 17), (300, 65), (1100, 5), (17, 17), (33, 2), (2, 2)]


class Result(object):
    """s, a, b (longdouble, M), neighbour (int32, M); means (M x C longdouble, inf at the own and the
    empty clusters); the bounds da, db, ds (float64, M) and dmeans (M x C); gap, gap_bound (float64, M);
    sizes (C)."""


def pair_distances(xrows, measure, ids=None, e=None):
    """(d, bound): the distances of the scored rows to all rows, M x N longdouble, and the bound of
    the device's error on each; the self pair holds 0 / 0."""
    x = np.asarray(xrows, dtype=np.float64).astype(LD)
    N, K = x.shape
    rows = np.arange(N) if ids is None else np.asarray(ids, dtype=np.int64)
    e = (K + 16) * U if e is None else e
    rest = np.maximum(LD(0), LD(1) - x[rows].dot(x.T))
    if measure == "cosine":
        d, bound = rest, np.full(rest.shape, e + U)
    elif measure == "hellinger":
        d = np.sqrt(rest)
        with np.errstate(divide="ignore"):
            bound = np.minimum(np.sqrt(e + U), (e + U) / d.astype(np.float64)) + U * d.astype(np.float64)
    else:
        raise ValueError(measure)
    me = (rows[:, None] == np.arange(N)[None, :])
    d[me] = 0
    bound = np.array(bound, dtype=np.float64)
    bound[me] = 0.0
    return d, bound


def silhouette(xrows, labels, measure, ids=None):
    labels = np.asarray(labels)
    N = len(labels)
    C = int(labels.max()) + 1
    rows = np.arange(N) if ids is None else np.asarray(ids, dtype=np.int64)
    M = len(rows)
    d, pb = pair_distances(xrows, measure, ids)
    sizes = np.bincount(labels, minlength=C).astype(np.int64)
    assert np.count_nonzero(sizes) >= 2
    own = labels[rows]
    means = np.full((M, C), np.inf, dtype=LD)
    dmeans = np.zeros((M, C))
    a, da = np.zeros(M, dtype=LD), np.zeros(M)
    for c in np.flatnonzero(sizes):
        members = labels == c
        n = int(sizes[c])
        total, btotal = d[:, members].sum(axis=1), pb[:, members].sum(axis=1)
        inside = own == c
        if n > 1:
            a[inside] = total[inside] / (n - 1)
            da[inside] = btotal[inside] / (n - 1)
            da[inside] += (-(-n // 16) + 8) * U * a[inside].astype(np.float64)
        outside = ~inside
        means[outside, c] = total[outside] / n
        dmeans[outside, c] = btotal[outside] / n + (-(-n // 16) + 8) * U * means[outside, c].astype(np.float64)
    order = np.lexsort((np.broadcast_to(np.arange(C), (M, C)), means), axis=1)
    out = Result()
    out.neighbour = order[:, 0].astype(np.int32)
    at = np.arange(M)
    out.a, out.b, out.means, out.dmeans, out.sizes = a, means[at, order[:, 0]], means, dmeans, sizes
    out.da, out.db = da, dmeans[at, order[:, 0]]
    second = means[at, order[:, 1]]
    with np.errstate(invalid="ignore"):
        out.gap = np.where(np.isfinite(second), second - out.b, np.inf).astype(np.float64)
    out.gap_bound = np.maximum(out.db, np.where(np.isfinite(second), dmeans[at, order[:, 1]], 0.0))
    top = np.maximum(out.a, out.b)
    single = sizes[own] == 1
    flat = single | ~(top > 0)
    safe = np.where(flat, LD(1), top)
    out.s = np.where(flat, LD(0), (out.b - out.a) / safe)
    # (max(a, b) = 0 away from a singleton: the device's a and b are rounding alone, and ds is inf)
    with np.errstate(divide="ignore"):
        out.ds = np.where(single, 0.0, 2 * (out.da + out.db) / top.astype(np.float64) + 4 * U)
    return out


# ---- the shared inputs -------------------------------------------------------------------------------
def planted_gammas(K, N, seed=None, centres=5):
    """N gamma columns (K x N, Fortran order) around `centres` planted Dirichlet centres, of very
    different totals."""
    rng = np.random.RandomState(7000 + K if seed is None else seed)
    conc = rng.gamma(0.5, 1.0, size=(centres, K)) * 6.0 + 0.3
    which = rng.randint(centres, size=1100)
    g = np.stack([rng.dirichlet(conc[t]) * rng.uniform(5.0, 50.0) + 1e-3 for t in which], axis=1)
    return np.asfortranarray(g[:, :N])


def init_ids(N, C):
    return np.linspace(0, N - 1, C).astype(int)


def labels_of(xrows, C, measure):
    """The labels of one nearest-centroid assignment under the documents init_ids(N, C) -- what
    DocumentIndex.nearest_centroid(theta^ of those documents) returns (tests/cluster_host.py).  With
    one topic every row is [1] and that assignment knows one cluster only, which a silhouette
    refuses: K = 1 takes the labels id mod C."""
    x = np.asarray(xrows, dtype=np.float64)
    N, K = x.shape
    if K == 1:
        return (np.arange(N) % C).astype(np.int32)
    picked = x[init_ids(N, C)]
    theta = picked ** 2 if measure == "hellinger" else picked / picked.sum(axis=1)[:, None]
    return ch.assign(x, dh.rows(theta.T, measure))[0]
