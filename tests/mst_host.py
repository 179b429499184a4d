"""NumPy restatement of the minimum spanning tree of an indexed corpus and of HDBSCAN* on it
(csrc/mst_kernels.h), in np.longdouble on the index's stored rows x (N x K, unit length).

    d(i, j)       silhouette_host.pair_distances: sqrt(max(0, 1 - s)) (hellinger) or max(0, 1 - s) (cosine)
    core(i)       the (min_samples - 1)-th smallest d(i, j) over j != i; 0 for min_samples = 1
    w(i, j)       max(d(i, j), core(i), core(j)): the mutual-reachability distance
    tree          Kruskal on all N (N - 1) / 2 pairs in the order (w, lo, hi)

The bound of the device's error on a tree weight (u = 2^-53, e = (K + 16) u the bound of s as in
silhouette_host, eps = e + u):

    b(x) = eps (cosine);  min(sqrt(eps), eps / x) + u x (hellinger)

is silhouette_host's pair bound as a function of the restated distance x; for Hellinger it grows as
x -> 0, up to sqrt(eps): the root of a value off by eps.  Why the pair bound carries over to the t-th
smallest weight of the tree: the device's distance of a pair lies in [g(x), f(x)] with f(x) = x + b(x)
and g(x) = x - b(x), and both are non-decreasing in x (hellinger: f' = 1 - eps / x^2 + u >= 0 from
x = sqrt(eps) on and 1 + u below it, continuous there; g' > 0 everywhere).  A non-decreasing map
commutes with every order statistic and with max, so the device's core(i) lies in [g(core), f(core)]
and its w(i, j) in [g(w), f(w)].  The t-th smallest weight W_t of a minimum spanning tree is the
smallest threshold at which the graph of the edges not heavier than it has at most N - t components;
every edge with restated weight <= W_t has device weight <= f(W_t), and every edge heavier than W_t has
device weight >= g of its own, so the device's W'_t lies in [g(W_t), f(W_t)]: |W'_t - W_t| <= b(W_t),
whatever tree either side picked among equal weights.  The sums differ by at most the sum of the
bounds (the device's weights are added exactly, with math.fsum).

Also a brute-force HDBSCAN* (Campello, Moulavi & Sander 2013) on an explicit edge list, written from the
definitions with recursive sets: the heaviest edge of a component is taken out -- among equal weights
the last in the order (w, lo, hi), so one edge at a time -- and the component falls into two sets found
by breadth-first search; lambda = 1 / max(w, 2^-52).  Both sets of at least min_cluster_size points: two
new clusters are born.  One such set: the cluster goes on as that set and the points of the other leave
at lambda.  None: all leave and the cluster ends.  Stability is the sum over a cluster's points of
lambda_leave - lambda_birth; 'eom' keeps a cluster when its stability is at least the sum of the best
of its two children's subtrees, 'leaf' keeps the clusters without children; the root only with
allow_single_cluster.  A point carries the topmost kept cluster it was born into.  O(N^2).

Also the inputs tests/test_mst_host.py and tests/test_gpu_mst.py share."""
import math
import sys

import numpy as np

import silhouette_host as sh

LD = np.longdouble
U = sh.U
MEASURES = sh.MEASURES
NS = [1, 2, 17, 130, 257, 300]
KS = [3, 33, 100]
MIN_SAMPLES = [1, 2, 5]
FLOOR = LD(2.0) ** -52


def weight_bound(w, K, measure):
    """b(w) of the module docstring, float64, elementwise."""
    w = np.asarray(w, dtype=np.float64)
    eps = (K + 16) * U + U
    if measure == "cosine":
        return np.full(w.shape, eps)
    with np.errstate(divide="ignore"):
        return np.minimum(math.sqrt(eps), eps / w) + U * w


def core_distances(d, min_samples):
    """Per row of the dense distances d (any dtype, the diagonal ignored) the (min_samples - 1)-th
    smallest off-diagonal entry; zeros for min_samples = 1."""
    N = d.shape[0]
    if min_samples == 1:
        return np.zeros(N, dtype=d.dtype)
    away = d[~np.eye(N, dtype=bool)].reshape(N, N - 1)
    return np.sort(away, axis=1)[:, min_samples - 2]


def mutual_reachability(d, core):
    return np.maximum(d, np.maximum(core[:, None], core[None, :]))


def kruskal(wm):
    """(u, v, w) of the minimum spanning tree of the dense symmetric weights wm under the edge order
    (w, lo, hi): u < v, sorted by that order."""
    N = wm.shape[0]
    lo, hi = np.triu_indices(N, 1)
    w = wm[lo, hi]
    order = np.lexsort((hi, lo, w))
    top = list(range(N))

    def find(a):
        while top[a] != a:
            top[a] = top[top[a]]
            a = top[a]
        return a
    picked = []
    for e in order.tolist():
        if len(picked) == N - 1:
            break
        a, b = find(int(lo[e])), find(int(hi[e]))
        if a != b:
            top[max(a, b)] = min(a, b)
            picked.append(e)
    picked = np.array(picked, dtype=np.int64)
    return lo[picked].astype(np.int64), hi[picked].astype(np.int64), w[picked]


def restated_tree(xrows, measure, min_samples):
    """(u, v, w longdouble, core longdouble) from the stored rows."""
    d = sh.pair_distances(xrows, measure)[0]
    core = core_distances(d, min_samples)
    return kruskal(mutual_reachability(d, core)) + (core,)


def dense_from_csr(indptr, ids, val, N):
    """The N x N matrix of a CSR that holds every off-diagonal pair (neighbors_within(radius=2.0))."""
    assert np.array_equal(np.diff(indptr), np.full(N, N - 1))
    out = np.zeros((N, N), dtype=val.dtype)
    out[np.repeat(np.arange(N), N - 1), ids] = val
    return out


# ---- the brute-force HDBSCAN* ---------------------------------------------------------------------------
class _Cluster(object):
    def __init__(self, points, birth):
        self.points, self.birth = frozenset(points), birth
        self.stability, self.children, self.left_at = LD(0), [], {}


def _sides(points, edges):
    """The two sets the points fall into once the last of `edges` is taken out."""
    a, b = edges[-1][1], edges[-1][2]
    near = {p: [] for p in points}
    for _, p, q in edges[:-1]:
        near[p].append(q)
        near[q].append(p)
    seen, queue = {a}, [a]
    while queue:
        for q in near[queue.pop()]:
            if q not in seen:
                seen.add(q)
                queue.append(q)
    assert b not in seen
    return seen, set(points) - seen


def _grow(cluster, edges, mcs):
    """Follows `cluster` down from its birth: `edges` is the sorted edge list of its points."""
    points = set(cluster.points)
    while edges:
        lam = 1 / max(LD(edges[-1][0]), FLOOR)
        one, two = _sides(points, edges)
        e1 = [e for e in edges[:-1] if e[1] in one]
        e2 = [e for e in edges[:-1] if e[1] in two]
        if len(one) >= mcs and len(two) >= mcs:
            cluster.stability += len(points) * (lam - cluster.birth)
            for side, es in ((one, e1), (two, e2)):
                child = _Cluster(side, lam)
                cluster.children.append(child)
                _grow(child, es, mcs)
            return
        for side in (one, two):
            if len(side) < mcs:
                cluster.stability += len(side) * (lam - cluster.birth)
                for p in side:
                    cluster.left_at[p] = lam
        if len(one) >= mcs:
            points, edges = one, e1
        elif len(two) >= mcs:
            points, edges = two, e2
        else:
            return
    assert len(points) <= 1                                  # (a lone point of a root below min_cluster_size)


def _best(cluster, selection, kept, is_root, allow_single):
    """The best total stability of the subtree; fills `kept` with the clusters chosen in it."""
    if not cluster.children:
        if not is_root or allow_single:
            kept.append(cluster)
        return cluster.stability
    below, total = [], LD(0)
    for child in cluster.children:
        total += _best(child, selection, below, False, allow_single)
    allowed = (not is_root or allow_single) and selection == "eom"
    if allowed and cluster.stability >= total:
        kept.append(cluster)
        return cluster.stability
    kept.extend(below)
    return total


def _last_lambda(cluster, out):
    out.update(cluster.left_at)
    for child in cluster.children:
        _last_lambda(child, out)


def hdbscan(u, v, w, N, min_cluster_size, selection="eom", allow_single_cluster=False):
    """(labels int32, probabilities longdouble, stabilities longdouble) of the brute-force HDBSCAN*."""
    assert min_cluster_size >= 2 and selection in ("eom", "leaf")
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * N + 1000))
    edges = sorted((wt, min(a, b), max(a, b)) for a, b, wt in zip(np.asarray(u).tolist(), np.asarray(v).tolist(),
                                                                   list(w)))
    root = _Cluster(range(N), LD(0))
    _grow(root, edges, min_cluster_size)
    kept = []
    _best(root, selection, kept, True, allow_single_cluster)
    kept.sort(key=lambda c: min(c.points))
    labels = np.full(N, -1, dtype=np.int32)
    prob = np.zeros(N, dtype=LD)
    for number, c in enumerate(kept):
        lam = {}
        _last_lambda(c, lam)
        peak = max(lam.values()) if lam else LD(0)
        for p in c.points:
            labels[p] = number
            if N == 1:
                prob[p] = 1
            elif peak > 0:
                prob[p] = lam[p] / peak
    return labels, prob, np.array([c.stability for c in kept], dtype=LD)


# ---- the shared inputs --------------------------------------------------------------------------------
def gammas(K, N, seed=None):
    """N gamma columns (K x N) around planted Dirichlet centres (silhouette_host.planted_gammas)."""
    return sh.planted_gammas(K, N, seed)


def with_repeats(g):
    """The same gamma with its column 1 (0 where there is only one) three times more, at the end and in
    the middle: four equal rows."""
    c = g[:, min(1, g.shape[1] - 1)]
    half = g.shape[1] // 2
    return np.asfortranarray(np.concatenate((g[:, :half], c[:, None], g[:, half:], c[:, None], c[:, None]), axis=1))


def planted_blobs(K=33, per=90, noise=30, seed=2013):
    """gamma (K x N, Fortran order) of three Dirichlet blobs of `per` documents around distinct topic
    mixtures, shuffled among `noise` documents drawn uniformly from the simplex; truth holds 0, 1, 2 and
    -1 for the noise.  N = 3 per + noise."""
    rng = np.random.RandomState(seed)
    truth = np.concatenate((np.repeat(np.arange(3), per), np.full(noise, -1)))
    rng.shuffle(truth)
    centre = np.full((3, K), 0.05)
    for c in range(3):
        centre[c, 5 * c:5 * c + 5] = (12.0, 9.0, 6.0, 4.0, 3.0)
    cols = []
    for t in truth:
        theta = rng.dirichlet(centre[t] * 8.0) if t >= 0 else rng.dirichlet(np.ones(K))
        cols.append(theta * rng.uniform(20.0, 200.0) + 1e-3)
    return np.asfortranarray(np.stack(cols, axis=1)), truth


def blob_points(seed=5, per=40, noise=12):
    """Points in the plane for the host tests: two tight blobs far apart and scattered noise; the dense
    Euclidean distances (float64) and the truth (0, 1, -1)."""
    rng = np.random.RandomState(seed)
    pts = np.concatenate((rng.normal((0.0, 0.0), 0.05, size=(per, 2)), rng.normal((4.0, 4.0), 0.05, size=(per, 2)),
                          rng.uniform(-8.0, 12.0, size=(noise, 2))))
    truth = np.concatenate((np.zeros(per, int), np.ones(per, int), np.full(noise, -1)))
    order = rng.permutation(len(pts))
    pts, truth = pts[order], truth[order]
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2))
    return d, truth
