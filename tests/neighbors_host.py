"""NumPy restatement of the radius join of an indexed corpus (csrc/neighbors_kernels.h)
in np.longdouble on the index's stored rows x (N x K, unit length), built from
silhouette_host.pair_distances -- the distances d(i, j) and the bound of the device's error on each:

    hit           d(i, j) <= radius, the pair (i, i) left out by id
    CSR           indptr (M + 1), ids (ascending within a row), dist (longdouble), bound (float64)

and its *near-threshold report*: the smallest |d(i, j) - radius| / bound(i, j) over all pairs but the
self pairs, which says how far any pair is from the other answer.  Where it is above 1 the device must
find exactly these hits.

Also an independent DBSCAN (Ester et al. 1996) on a CSR input, written as plain breadth-first search
over the core documents -- not the product's union-find: a core has at least min_samples - 1 hits, a
cluster is a connected component of the cores (numbered by ascending smallest core id), a border
document takes the cluster of its first core hit in the order (distance ascending, id ascending), the
rest is noise (-1).  Its report is the smallest gap between a border document's two nearest core hits,
in units of the larger of the two pairs' bounds where bounds are given.

Also the shapes and radii tests/test_neighbors_host.py and tests/test_gpu_neighbors.py share."""
import numpy as np

import silhouette_host as sh

LD = np.longdouble
MEASURES = sh.MEASURES
KS = [1, 3, 15, 17, 33, 130]
NS = [2, 17, 300, 1100]
DBSCAN_CASES = {"hellinger": (0.15, 12), "cosine": (0.015, 12)}      # radius, min_samples on planted_groups()


class Result(object):
    """indptr (int64, M + 1), ids (int64), dist (longdouble), bound (float64); report (float)."""


def radii(d, K):
    """The radii of the shared shapes: the 2 % and the 20 % quantile of the off-diagonal distances,
    rounded to three decimals and at least 0.001; with one topic every distance is 0 and the radius 0.5."""
    if K == 1:
        return [0.5]
    N = d.shape[0]
    away = d[~np.eye(N, dtype=bool)].astype(np.float64)
    return [max(0.001, round(float(np.quantile(away, q)), 3)) for q in (0.02, 0.2)]


def join(d, bound, radius, ids=None):
    """The CSR of the hits among the distances d (M x N, as pair_distances(xrows, measure, ids) gives
    them) and the near-threshold report."""
    M, N = d.shape
    rows = np.arange(N) if ids is None else np.asarray(ids, dtype=np.int64)
    other = rows[:, None] != np.arange(N)[None, :]
    hit = (d <= LD(radius)) & other
    out = Result()
    out.indptr = np.concatenate(([0], np.cumsum(hit.sum(axis=1)))).astype(np.int64)
    at = np.nonzero(hit)                                     # (row-major: ascending id within a row)
    out.ids = at[1].astype(np.int64)
    out.dist, out.bound = d[at], bound[at]
    off = np.abs(d - LD(radius)).astype(np.float64)[other]
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(off > 0, off / bound[other], 0.0)
    out.report = float(share.min()) if share.size else np.inf
    return out


def neighbors(xrows, measure, radius, ids=None):
    d, bound = sh.pair_distances(xrows, measure, ids)
    return join(d, bound, radius, ids)


def dbscan(indptr, ids, dist, min_samples, bound=None):
    """(labels int32, core bool, gap): breadth-first search over a CSR hit list of all N documents."""
    N = len(indptr) - 1
    core = np.diff(indptr) + 1 >= min_samples
    labels = np.full(N, -1, dtype=np.int32)
    clusters = 0
    for start in range(N):
        if not core[start] or labels[start] >= 0:
            continue
        labels[start] = clusters
        queue = [start]
        while queue:
            u = queue.pop(0)
            for v in ids[indptr[u]:indptr[u + 1]]:
                if core[v] and labels[v] < 0:
                    labels[v] = clusters
                    queue.append(int(v))
        clusters += 1
    gap = np.inf
    for i in np.flatnonzero(~core):
        span = np.arange(indptr[i], indptr[i + 1])
        span = span[core[ids[span]]]
        if not len(span):
            continue
        span = span[np.lexsort((ids[span], dist[span]))]
        labels[i] = labels[ids[span[0]]]
        if len(span) > 1:
            step = float(dist[span[1]] - dist[span[0]])
            unit = 1.0 if bound is None else float(max(bound[span[0]], bound[span[1]]))
            gap = min(gap, step / unit if unit > 0 else (np.inf if step > 0 else 0.0))
    return labels, core, gap


def planted_groups(K=23, groups=4, per=40, outliers=5, seed=321):
    """gamma (K x N, Fortran order) of `groups` well-separated Dirichlet groups of `per` documents,
    shuffled, and `outliers` documents far from all of them and from each other at the end: each holds
    nearly all its mass on one topic that no group and no other outlier uses."""
    assert 4 * groups + outliers <= K
    rng = np.random.RandomState(seed)
    truth = np.repeat(np.arange(groups), per)
    rng.shuffle(truth)
    centre = np.full((groups, K), 0.2)
    for c in range(groups):
        centre[c, 4 * c:4 * c + 4] = 25.0
    cols = [rng.dirichlet(centre[t]) * rng.uniform(5.0, 50.0) + 1e-3 for t in truth]
    for o in range(outliers):
        far = np.full(K, 1e-3)
        far[4 * groups + o] = 30.0
        cols.append(far)
    return np.asfortranarray(np.stack(cols, axis=1)), truth
