"""The restatement of the radius join and of DBSCAN (tests/neighbors_host.py) itself, without a GPU:
the join against a dense brute-force pass in float64; DBSCAN on a hand-made graph with a chain, a
border document tied between two clusters, and noise; the product's own host arithmetic (the union-find,
the nearest core hit, the labels) on the same graph; what DocumentIndex.neighbors_within and dbscan
refuse before they need a device; the symbol and the two kernels' resources; and -- what
tests/test_gpu_neighbors.py rests on -- on every shape of that file no pair is closer than 100 of its
bounds to the radius, and no border document of the DBSCAN inputs is closer than 100 bounds to another
answer, so the GPU tests let nothing off."""
import math

import numpy as np
import pytest

import docindex_host as dh
import neighbors_host as nh
import silhouette_host as sh


@pytest.mark.parametrize("measure", nh.MEASURES)
def test_restatement_is_a_dense_pass(measure):
    x = dh.rows(sh.planted_gammas(5, 23), measure)
    N = len(x)
    d = np.zeros((N, N))
    for i in range(N):
        for j in range(N):
            rest = max(0.0, 1.0 - float(np.dot(x[i], x[j])))
            d[i, j] = math.sqrt(rest) if measure == "hellinger" else rest
    radius = float(np.quantile(d[~np.eye(N, dtype=bool)], 0.3))
    radius = round(radius, 3)
    got = nh.neighbors(x, measure, radius)
    assert got.report > 1e6
    want = [[j for j in range(N) if j != i and d[i, j] <= radius] for i in range(N)]
    assert got.indptr.tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist()
    assert got.ids.tolist() == [j for w in want for j in w]
    assert 0 < len(got.ids) < N * (N - 1)
    flat = np.array([d[i, j] for i, w in enumerate(want) for j in w])
    assert np.max(np.abs(got.dist.astype(np.float64) - flat)) < 1e-14
    assert np.all(got.bound > 0) and got.bound.max() < 1e-7
    # a permuted subset with repeats: the same lists per id
    ids = np.array([7, 0, 22, 7, 5])
    part = nh.neighbors(x, measure, radius, ids=ids)
    for q, i in enumerate(ids):
        assert part.ids[part.indptr[q]:part.indptr[q + 1]].tolist() == want[i]
    # the report is the nearest pair to the radius, in bounds: at a pair's own distance it is (about) 0
    at = nh.neighbors(x, measure, float(got.dist[0]))
    assert at.report < 1.0


def _csr(N, edges):
    """A symmetric CSR hit list from undirected edges {(i, j): distance}."""
    lists = [[] for _ in range(N)]
    for (i, j), dist in edges.items():
        lists[i].append((j, dist))
        lists[j].append((i, dist))
    lists = [sorted(row) for row in lists]
    indptr = np.concatenate(([0], np.cumsum([len(row) for row in lists]))).astype(np.int64)
    ids = np.array([j for row in lists for j, _ in row], dtype=np.int64)
    dist = np.array([v for row in lists for _, v in row], dtype=np.float64)
    return indptr, ids, dist


def _hand_made(tie=True):
    """min_samples = 4: a core has at least three hits.  A chain of cores 1 - 2 - 3, each with a third
    hit (1: 0 and 4, 2: 5, 3: 6 and 10); a triangle of cores 7, 8, 9, each with a third hit (7: 6, 8: 10,
    9: 11).  The border documents: 0, 4, 5 (chain) and 11 (triangle) by their only core hit; 6 hits core 3
    and core 7 at the same distance -- tied between the two clusters, the smaller id wins; 10 hits 3 at
    0.3 and 8 at 0.2 -- the nearer one wins although its id is larger.  Noise: 12 hits only the border
    document 0, 13 nothing."""
    edges = {(1, 2): .1, (2, 3): .1, (0, 1): .1, (1, 4): .1, (2, 5): .1, (3, 6): .25 if tie else .15, (3, 10): .3,
             (7, 8): .1, (8, 9): .1, (7, 9): .1, (6, 7): .25, (8, 10): .2, (9, 11): .1, (0, 12): .3}
    want = np.array([0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, -1, -1], dtype=np.int32)
    core = np.zeros(14, dtype=bool)
    core[[1, 2, 3, 7, 8, 9]] = True
    return _csr(14, edges), want, core


def test_dbscan_restatement_on_a_hand_made_graph():
    (indptr, ids, dist), want, core = _hand_made()
    labels, got_core, gap = nh.dbscan(indptr, ids, dist, 4)
    assert np.array_equal(got_core, core) and np.array_equal(labels, want) and labels.dtype == np.int32
    assert gap == 0.0                                        # (document 6 is tied)
    # without the tie the smallest gap is 0.1, of documents 6 and 10
    (indptr, ids, dist), want, core = _hand_made(tie=False)
    labels, got_core, gap = nh.dbscan(indptr, ids, dist, 4)
    assert np.array_equal(labels, want) and abs(gap - 0.1) < 1e-12
    # min_samples = 1: every document is a core, the clusters are the components, in order of first id
    labels, got_core, _ = nh.dbscan(indptr, ids, dist, 1)
    assert got_core.all() and labels.tolist() == [0] * 13 + [1]
    # nobody is a core
    labels, got_core, _ = nh.dbscan(indptr, ids, dist, 9)
    assert not got_core.any() and np.all(labels == -1)


def test_the_products_host_arithmetic_on_the_same_graph():
    """DocumentIndex.dbscan's closing arithmetic (union-find over core-core hits, the nearest core
    hit, the numbering) fed the hand-made hit list whole and in chunks of rows."""
    from trlda_amd import index
    (indptr, ids, dist), want, core = _hand_made()
    N = len(indptr) - 1
    for cuts in ([0, N], [0, 3, 4, 9, N], list(range(N + 1))):
        parent = np.arange(N, dtype=np.int64)
        nearest = np.full(N, -1, dtype=np.int64)
        for a, b in zip(cuts[:-1], cuts[1:]):
            rows = np.repeat(np.arange(a, b), np.diff(indptr[a:b + 1]))
            hit, away = ids[indptr[a]:indptr[b]], dist[indptr[a]:indptr[b]]
            link = core[hit] & core[rows]
            index._union(parent, rows[link], hit[link])
            border = core[hit] & ~core[rows]
            index._nearest(nearest, rows[border], hit[border], away[border])
        labels, got_core = index._dbscan_labels(parent, core, nearest, True)
        assert labels.dtype == np.int32 and np.array_equal(labels, want) and got_core is core
        assert nearest[6] == 3 and nearest[10] == 8 and nearest[0] == 1 and nearest[12] == -1 and nearest[2] == -1
    # a long chain of cores joined by shuffled edges: one tree, rooted at its smallest member
    n = 500
    order = np.random.RandomState(3).permutation(n - 1)
    parent = np.arange(n + 2, dtype=np.int64)
    index._union(parent, order + 1, order + 2)
    assert np.all(index._roots(parent)[1:n + 1] == 1) and parent[0] == 0 and parent[n + 1] == n + 1


def test_arguments_are_checked_in_python():
    """What needs no device: the checks run before the handle is used for any GPU work."""
    from trlda_amd.index import DocumentIndex
    ix = DocumentIndex.__new__(DocumentIndex)
    ix._handle = None
    for call in (lambda: ix.neighbors_within(0.1), lambda: ix.dbscan(0.1)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    assert callable(DocumentIndex.neighbors_within) and callable(DocumentIndex.dbscan)


def test_symbol_is_bound():
    import ctypes as C
    from trlda_amd import _ffi
    assert "trlda_docindex_neighbors" in _ffi.EXPORTED_SYMBOLS
    restype, argtypes = _ffi._SIGNATURES["trlda_docindex_neighbors"]
    assert restype is C.c_int and len(argtypes) == 10
    assert argtypes[1] is C.c_double and argtypes[4] is C.c_int64 and argtypes[6] is C.c_int64


def test_symbol_is_exported(hip_lib):
    assert hasattr(hip_lib, "trlda_docindex_neighbors")


def test_kernels_use_no_scratch_and_spill_nothing(hip_lib):
    import os
    from helpers import kernel_resources
    from trlda_amd import _ffi
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    res = kernel_resources(_ffi.LIB_PATH)
    for kernel in ("neighbors_count_kernel", "neighbors_fill_kernel", "neighbors_scan_kernel"):
        found = [v for k, v in res.items() if kernel in k]
        assert len(found) == 1, (kernel, sorted(res)[:3])
        f = found[0]
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (kernel, f)
        assert f["vgpr_count"] <= 256


@pytest.mark.parametrize("measure", nh.MEASURES)
@pytest.mark.parametrize("N", nh.NS)
@pytest.mark.parametrize("K", nh.KS)
def test_no_pair_is_near_the_radius_on_the_shapes_of_the_gpu_test(K, N, measure):
    x = dh.rows(sh.planted_gammas(K, N), measure)
    d, bound = sh.pair_distances(x, measure)
    radii = nh.radii(d, K)
    assert len(radii) == (1 if K == 1 else 2) and all(r >= 0.001 for r in radii)
    for radius in radii:
        got = nh.join(d, bound, radius)
        assert got.report > 100, (radius, got.report)
        total = int(got.indptr[-1])
        if K == 1:
            assert total == N * (N - 1)                      # (every distance is 0)
        else:
            assert 0 <= total <= N * (N - 1) and (total < N * (N - 1) or N == 2)
    if K > 1 and N >= 300:
        # the two radii are different questions: the larger one finds more, and both find something
        few, many = (int(nh.join(d, bound, r).indptr[-1]) for r in radii)
        assert 0 < few < many


@pytest.mark.parametrize("measure", nh.MEASURES)
def test_dbscan_inputs_have_no_near_tie(measure):
    """The planted groups of tests/test_gpu_neighbors.py: four clusters, border documents, the planted
    outliers (and a few stragglers) noise; every pair and every border choice 100 bounds from another answer."""
    radius, min_samples = nh.DBSCAN_CASES[measure]
    g, truth = nh.planted_groups()
    x = dh.rows(g, measure)
    ref = nh.neighbors(x, measure, radius)
    assert ref.report > 100
    labels, core, gap = nh.dbscan(ref.indptr, ref.ids, ref.dist, min_samples, ref.bound)
    assert gap > 100
    border = ~core & (labels >= 0)
    assert labels.max() == 3 and core.sum() > 50 and border.sum() > 10 and np.all(labels[-5:] == -1)
    kept = labels[:len(truth)] >= 0
    assert len(set(zip(labels[:len(truth)][kept].tolist(), truth[kept].tolist()))) == 4      # the planted groups
