"""The host parts of the spanning-tree entry points (trlda_amd/index.py) and their
restatement (tests/mst_host.py), without a GPU: the linkage matrix and its cuts on hand-made edge lists,
one round of Boruvka's algorithm, the restated tree and its bound, and HDBSCAN* -- the product's closing
arithmetic (`_hdbscan_labels`: edge list in, labels out, the function `DocumentIndex.hdbscan` calls)
against the brute-force restatement, SciPy and scikit-learn."""
import math

import numpy as np
import pytest

import mst_host as mh
from trlda_amd import index as ti
from trlda_amd.index import DocumentIndex

LD = np.longdouble


def _tree_of(d, min_samples=1):
    """The restated tree of dense float64 distances, as float64."""
    core = mh.core_distances(d, min_samples)
    u, v, w = mh.kruskal(mh.mutual_reachability(d, core))
    return u, v, np.asarray(w, dtype=np.float64)


# ---- the linkage matrix ------------------------------------------------------------------------------
def test_linkage_of_a_path():
    # 0 - 1 - 2 - 3 with rising weights: a chain of merges, each taking one more document in
    Z = ti._linkage([0, 1, 2], [1, 2, 3], [1.0, 2.0, 3.0], 4)
    assert Z.dtype == np.float64
    assert Z.tolist() == [[0, 1, 1.0, 2], [2, 4, 2.0, 3], [3, 5, 3.0, 4]]
    # the same path given backwards and unsorted: the order (w, u, v) is the function's own
    Z2 = ti._linkage([3, 2, 1], [2, 1, 0], [3.0, 2.0, 1.0], 4)
    assert np.array_equal(Z, Z2)
    # falling weights along the path: the far end merges first
    Z3 = ti._linkage([0, 1, 2], [1, 2, 3], [3.0, 2.0, 1.0], 4)
    assert Z3.tolist() == [[2, 3, 1.0, 2], [1, 4, 2.0, 3], [0, 5, 3.0, 4]]


def test_linkage_of_a_star():
    # the centre 2 joined to 0, 1, 3, 4: every merge takes the centre's cluster and one leaf
    Z = ti._linkage([2, 2, 2, 2], [0, 1, 3, 4], [0.4, 0.1, 0.3, 0.2], 5)
    assert Z.tolist() == [[1, 2, 0.1, 2], [4, 5, 0.2, 3], [3, 6, 0.3, 4], [0, 7, 0.4, 5]]


def test_linkage_of_equal_weights_follows_the_edge_order():
    # a square's tree 0-1, 0-2, 1-3 at one weight: (w, u, v) decides
    Z = ti._linkage([1, 0, 0], [3, 2, 1], [0.5, 0.5, 0.5], 4)
    assert Z.tolist() == [[0, 1, 0.5, 2], [2, 4, 0.5, 3], [3, 5, 0.5, 4]]
    assert np.all(Z[:, 0] < Z[:, 1])


def test_linkage_refuses_what_is_no_tree():
    with pytest.raises(ValueError):
        ti._linkage([0, 1, 0], [1, 2, 2], [1.0, 1.0, 1.0], 4)         # a cycle
    with pytest.raises(ValueError):
        ti._linkage([0, 1], [1, 2], [1.0, 1.0], 4)                     # too few edges
    with pytest.raises(ValueError):
        ti._linkage([0, 1, 2], [1, 2, 4], [1.0, 1.0, 1.0], 4)         # an unknown document
    assert ti._linkage([], [], [], 1).shape == (0, 4)


def test_cut_linkage_numbers_by_smallest_member():
    # two pairs far apart and a loner: 3-4 merge first, then 0-2, then 1 joins {3, 4}, then all
    Z = ti._linkage([3, 0, 1, 0], [4, 2, 3, 1], [0.1, 0.2, 0.5, 0.9], 5)
    cut = DocumentIndex.cut_linkage
    assert cut(Z, num_clusters=5).tolist() == [0, 1, 2, 3, 4]
    assert cut(Z, num_clusters=4).tolist() == [0, 1, 2, 3, 3]
    assert cut(Z, num_clusters=3).tolist() == [0, 1, 0, 2, 2]
    assert cut(Z, num_clusters=2).tolist() == [0, 1, 0, 1, 1]
    assert cut(Z, num_clusters=1).tolist() == [0, 0, 0, 0, 0]
    assert cut(Z, num_clusters=3).dtype == np.int32
    # by height: a merge AT the distance is applied
    assert cut(Z, distance=0.05).tolist() == [0, 1, 2, 3, 4]
    assert cut(Z, distance=0.2).tolist() == [0, 1, 0, 2, 2]
    assert cut(Z, distance=0.49).tolist() == [0, 1, 0, 2, 2]
    assert cut(Z, distance=0.5).tolist() == [0, 1, 0, 1, 1]
    assert cut(Z, distance=math.inf).tolist() == [0, 0, 0, 0, 0]
    for bad in (dict(), dict(num_clusters=2, distance=0.3)):
        with pytest.raises(ValueError):
            cut(Z, **bad)
    for bad in (0, 6):
        with pytest.raises(ValueError):
            cut(Z, num_clusters=bad)
    with pytest.raises(ValueError):
        cut(np.zeros((3, 3)), num_clusters=2)
    assert cut(np.zeros((0, 4)), num_clusters=1).tolist() == [0]


# ---- Boruvka on the host -----------------------------------------------------------------------------
def _host_sweep(wm, comp):
    """What the device's sweep returns, from dense weights: the first candidate in the order (w, j)."""
    N = wm.shape[0]
    best_j, best_w = np.full(N, -1, dtype=np.int64), np.full(N, np.inf)
    for i in range(N):
        cand = np.flatnonzero(comp != comp[i])
        if len(cand):
            j = cand[np.lexsort((cand, wm[i, cand]))[0]]
            best_j[i], best_w[i] = j, wm[i, j]
    return best_j, best_w


def _host_boruvka(wm):
    """DocumentIndex.spanning_tree's loop with the sweep on the host."""
    N = wm.shape[0]
    parent, comp, parts = np.arange(N, dtype=np.int64), np.arange(N, dtype=np.int32), []
    rounds = 0
    while len(np.unique(comp)) > 1:
        lo, hi, w = ti._boruvka_edges(comp, *_host_sweep(wm, comp))
        parts.append((lo, hi, w))
        ti._union(parent, lo, hi)
        comp = ti._roots(parent).astype(np.int32)
        rounds += 1
    assert rounds <= max(N - 1, 0).bit_length()
    return ti._sorted_edges(parts)


@pytest.mark.parametrize("N", [1, 2, 3, 17, 64, 130])
def test_boruvka_rounds_give_kruskals_tree(N):
    rng = np.random.RandomState(N)
    d = rng.uniform(0.1, 1.0, size=(N, N))
    d = np.minimum(d, d.T)
    np.fill_diagonal(d, 0.0)
    for wm in (d, np.round(d, 1), np.full((N, N), 0.25)):             # distinct, many ties, all equal
        u, v, w = _host_boruvka(wm)
        ku, kv, kw = mh.kruskal(wm)
        assert u.dtype == v.dtype == np.int64 and w.dtype == np.float64 and len(u) == N - 1
        assert np.array_equal(u, ku) and np.array_equal(v, kv) and np.array_equal(w, kw)
        assert np.all(u < v)


def test_boruvka_edges_keeps_an_edge_chosen_twice_once():
    comp = np.array([0, 0, 2, 2], dtype=np.int32)
    best_j = np.array([2, 3, 0, -1], dtype=np.int64)
    best_w = np.array([0.5, 0.7, 0.5, np.inf])
    lo, hi, w = ti._boruvka_edges(comp, best_j, best_w)
    assert lo.tolist() == [0] and hi.tolist() == [2] and w.tolist() == [0.5]
    lo, hi, w = ti._boruvka_edges(comp, np.full(4, -1, dtype=np.int64), best_w)
    assert len(lo) == len(hi) == len(w) == 0


# ---- the restatement itself --------------------------------------------------------------------------
def test_restated_tree_and_bound():
    import docindex_host as dh
    K, N = 33, 60
    for measure in mh.MEASURES:
        x = dh.rows(mh.gammas(K, N), measure)
        d, pair_bound = mh.sh.pair_distances(x, measure)
        assert np.array_equal(d, d.T)
        for ms in mh.MIN_SAMPLES:
            u, v, w, core = mh.restated_tree(x, measure, ms)
            assert w.dtype == LD and len(w) == N - 1 and np.all(np.diff(w) >= 0) and np.all(u < v)
            # a tree: N - 1 edges that join everything
            assert ti._linkage(u, v, np.asarray(w, dtype=np.float64), N)[-1, 3] == N
            # no lighter tree by exchanging: every non-tree pair is at least as heavy as the tree's path
            wm = mh.mutual_reachability(d, core)
            assert np.all(w >= np.sort(wm[~np.eye(N, dtype=bool)])[0])
            if ms > 1:
                assert np.all(core > 0) and np.all(w >= core[u]) and np.all(w >= core[v])
            # b(w) is the pair bound at that distance
            b = mh.weight_bound(w, K, measure)
            at = (u, v)
            plain = np.asarray(d[at] == w)
            assert np.allclose(b[plain], pair_bound[at][plain], rtol=1e-12, atol=0)
    eps = (K + 16) * mh.U + mh.U
    grid = np.concatenate(([0.0], np.logspace(-12, 0, 400)))
    b = mh.weight_bound(grid, K, "hellinger")
    assert b[0] == math.sqrt(eps) and np.all(np.diff(grid + b) >= 0) and np.all(np.diff(grid - b) > 0)
    assert np.all(mh.weight_bound(grid, K, "cosine") == eps)


def test_core_distances_count_the_document_itself():
    d = np.array([[0.0, 1.0, 3.0, 7.0], [1.0, 0.0, 2.0, 6.0], [3.0, 2.0, 0.0, 4.0], [7.0, 6.0, 4.0, 0.0]])
    assert mh.core_distances(d, 1).tolist() == [0, 0, 0, 0]
    assert mh.core_distances(d, 2).tolist() == [1, 1, 2, 4]
    assert mh.core_distances(d, 3).tolist() == [3, 2, 3, 6]
    assert mh.core_distances(d, 4).tolist() == [7, 6, 4, 7]
    wm = mh.mutual_reachability(d, mh.core_distances(d, 3))
    assert wm[0, 1] == 3 and wm[1, 2] == 3 and wm[2, 3] == 6 and np.array_equal(wm, wm.T)


# ---- HDBSCAN* ----------------------------------------------------------------------------------------
def test_hdbscan_by_hand():
    # two tight triples joined by a long edge, and a far loner: 0-1-2 at 1, 3-4-5 at 1, 2-3 at 10, 5-6 at 40
    u, v, w = [0, 1, 3, 4, 2, 5], [1, 2, 4, 5, 3, 6], [1.0, 1.0, 1.0, 1.0, 10.0, 40.0]
    labels, prob, stab = ti._hdbscan_labels(u, v, w, 7, 3)
    assert labels.tolist() == [0, 0, 0, 1, 1, 1, -1] and labels.dtype == np.int32
    # each triple is born at 1 / 10 and its documents leave at 1 / 1
    assert np.allclose(stab, [3 * (1 - 0.1), 3 * (1 - 0.1)], rtol=1e-15)
    assert prob.tolist() == [1, 1, 1, 1, 1, 1, 0]
    # the root itself: everything, the loner with the smallest lambda
    labels, prob, stab = ti._hdbscan_labels(u, v, w, 7, 4, allow_single_cluster=True)
    assert labels.tolist() == [0] * 7 and prob[6] == (1 / 40.0) / (1 / 10.0) and len(stab) == 1
    assert ti._hdbscan_labels(u, v, w, 7, 4)[0].tolist() == [-1] * 7
    assert ti._hdbscan_labels([], [], [], 1, 2)[0].tolist() == [-1]
    assert ti._hdbscan_labels([], [], [], 1, 2, allow_single_cluster=True)[0].tolist() == [0]
    for bad in (dict(min_cluster_size=1), dict(min_cluster_size=3, selection="best")):
        with pytest.raises(ValueError):
            ti._hdbscan_labels(u, v, w, 7, **bad)


def test_lambda_floor_keeps_equal_rows_finite():
    # weights of 0 and of rounding size: lambda = 2^52 for both, no division by zero, no inf - inf
    u, v, w = [0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [0.0, 1e-17, 0.5, 0.0, 2.0 ** -53]
    labels, prob, stab = ti._hdbscan_labels(u, v, w, 6, 3)
    assert labels.tolist() == [0, 0, 0, 1, 1, 1] and np.all(np.isfinite(stab)) and np.all(np.isfinite(prob))
    assert np.all(stab == 3 * (2.0 ** 52 - 2.0)) and np.all(prob == 1.0)


@pytest.mark.parametrize("allow_single", [False, True])
@pytest.mark.parametrize("selection", ["eom", "leaf"])
@pytest.mark.parametrize("mcs,ms", [(5, 5), (10, 3), (3, 1), (40, 5)])
def test_hdbscan_matches_the_brute_force_on_planted_blobs(mcs, ms, selection, allow_single):
    d, truth = mh.blob_points()
    N = len(truth)
    u, v, w = _tree_of(d, ms)
    labels, prob, stab = ti._hdbscan_labels(u, v, w, N, mcs, selection, allow_single)
    ref_labels, ref_prob, ref_stab = mh.hdbscan(u, v, w, N, mcs, selection, allow_single)
    assert np.array_equal(labels, ref_labels)
    assert len(stab) == len(ref_stab) == labels.max() + 1
    assert np.allclose(stab, ref_stab.astype(np.float64), rtol=1e-12, atol=0)
    assert np.allclose(prob, ref_prob.astype(np.float64), rtol=1e-14, atol=0)
    assert np.all((prob >= 0) & (prob <= 1)) and np.all(prob[labels < 0] == 0)
    if (mcs, ms) == (5, 5) and selection == "eom" and not allow_single:
        # the two planted blobs, whole and apart
        for t in (0, 1):
            assert len(np.unique(labels[truth == t])) == 1 and labels[truth == t][0] >= 0
        assert labels[truth == 0][0] != labels[truth == 1][0]


def test_hdbscan_matches_the_brute_force_with_ties_in_bulk():
    # distances rounded to one decimal: most weights are equal to some other, the edge order decides
    rng = np.random.RandomState(3)
    pts = np.concatenate((rng.normal(0, 0.3, size=(25, 2)), rng.normal(3, 0.3, size=(25, 2))))
    d = np.round(np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(axis=2)), 1)
    for ms in (1, 4):
        u, v, w = _tree_of(d, ms)
        assert len(np.unique(w)) < len(w) // 2
        for mcs in (2, 5):
            for selection in ("eom", "leaf"):
                got = ti._hdbscan_labels(u, v, w, 50, mcs, selection)[0]
                assert np.array_equal(got, mh.hdbscan(u, v, w, 50, mcs, selection)[0]), (ms, mcs, selection)


def test_single_linkage_heights_are_scipys():
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    rng = np.random.RandomState(11)
    N = 40
    d = rng.uniform(0.1, 1.0, size=(N, N))
    d = np.minimum(d, d.T)
    np.fill_diagonal(d, 0.0)
    assert len(np.unique(d[np.triu_indices(N, 1)])) == N * (N - 1) // 2    # distinct entries
    Z = ti._linkage(*_tree_of(d), N)
    ref = hierarchy.linkage(squareform(d), "single")
    assert np.array_equal(Z[:, 2], ref[:, 2]) and np.array_equal(Z[:, 3], ref[:, 3])
    assert hierarchy.is_valid_linkage(Z)
    for k in (2, 3, 7):
        mine = DocumentIndex.cut_linkage(Z, num_clusters=k)
        theirs = hierarchy.fcluster(Z, k, criterion="maxclust")
        assert len(set(zip(mine.tolist(), theirs.tolist()))) == k == len(np.unique(mine))


def test_hdbscan_labels_are_sklearns_on_separated_groups():
    cluster = pytest.importorskip("sklearn.cluster")
    if not hasattr(cluster, "HDBSCAN"):
        pytest.skip("this scikit-learn has no HDBSCAN")
    rng = np.random.RandomState(17)
    centres = np.array([(0.0, 0.0), (10.0, 0.0), (0.0, 10.0), (10.0, 10.0)])
    pts = np.concatenate([rng.normal(c, 0.5, size=(30, 2)) for c in centres])
    pts = pts[rng.permutation(len(pts))]
    d = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(axis=2))
    N = len(pts)
    for mcs, ms in ((5, 5), (10, 4)):
        theirs = cluster.HDBSCAN(min_cluster_size=mcs, min_samples=ms, metric="precomputed").fit(d.copy()).labels_
        mine = ti._hdbscan_labels(*_tree_of(d, ms), N, mcs)[0]
        pairs = set(zip(mine.tolist(), theirs.tolist()))
        assert len(pairs) == len(np.unique(mine)) == len(np.unique(theirs)), pairs     # equal up to renumbering
        assert (-1, -1) in pairs or (np.all(mine >= 0) and np.all(theirs >= 0))
        assert len(np.unique(mine[mine >= 0])) == 4
