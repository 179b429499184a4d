"""The restatement of the silhouette (tests/silhouette_host.py) itself, without a GPU: against a plain
double loop on tiny inputs; singletons, label values without members, one topic and duplicates; the
closed form of the cosine sums; what DocumentIndex.silhouette refuses before it needs a device; and --
what tests/test_gpu_silhouette.py rests on -- on every shape of that file no document's `neighbour` is
closer than 100 of its bounds to a different answer, so the GPU test lets no document off."""
import math

import numpy as np
import pytest

import docindex_host as dh
import silhouette_host as sh

LD = np.longdouble
U = 2.0 ** -53


def _plain(x, labels, measure):
    """The definition in float64, one pair at a time."""
    N = len(labels)
    d = np.zeros((N, N))
    for i in range(N):
        for j in range(N):
            rest = max(0.0, 1.0 - float(np.dot(x[i], x[j])))
            d[i, j] = math.sqrt(rest) if measure == "hellinger" else rest
    s, a, b, nb = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N, dtype=int)
    for i in range(N):
        own = [j for j in range(N) if labels[j] == labels[i] and j != i]
        a[i] = sum(d[i, j] for j in own) / len(own) if own else 0.0
        means = {c: np.mean([d[i, j] for j in range(N) if labels[j] == c]) for c in set(labels) if c != labels[i]}
        nb[i] = min(means, key=lambda c: (means[c], c))
        b[i] = means[nb[i]]
        s[i] = (b[i] - a[i]) / max(a[i], b[i]) if own and max(a[i], b[i]) > 0 else 0.0
    return s, a, b, nb


@pytest.mark.parametrize("measure", sh.MEASURES)
def test_restatement_is_the_definition(measure):
    x = dh.rows(sh.planted_gammas(5, 23), measure)
    labels = np.array([0, 3, 3, 1, 0, 5, 1, 1, 0, 3, 0, 1, 3, 3, 0, 1, 1, 0, 3, 0, 1, 3, 0])   # 5: a singleton; 2, 4: empty
    want = _plain(x, labels, measure)
    got = sh.silhouette(x, labels, measure)
    for w, g in zip(want[:3], (got.s, got.a, got.b)):
        assert np.max(np.abs(w - g.astype(np.float64))) < 1e-14
    assert np.array_equal(want[3], got.neighbour)
    assert got.s[5] == 0 and got.a[5] == 0 and got.b[5] > 0 and got.neighbour[5] in (0, 1, 3)
    assert np.all(np.isinf(got.means[:, [2, 4]])) and np.array_equal(got.sizes, [8, 7, 0, 7, 0, 1])
    assert np.all(np.abs(got.s) <= 1) and np.all(got.gap >= 0) and np.all(np.delete(got.ds, 5) > 0)
    # a permuted subset with repeats: the same figures per id
    ids = np.array([7, 0, 22, 7, 5, 13])
    part = sh.silhouette(x, labels, measure, ids=ids)
    for name in ("s", "a", "b", "neighbour", "gap", "ds"):
        assert np.array_equal(getattr(part, name), getattr(got, name)[ids]), name


@pytest.mark.parametrize("measure", sh.MEASURES)
def test_one_topic(measure):
    """K = 1: every row is [1], every distance exactly 0, every silhouette 0, the neighbour the
    smallest other label with members."""
    x = dh.rows(sh.planted_gammas(1, 12), measure)
    labels = np.array([2, 2, 4, 4, 5, 2, 4, 5, 5, 2, 7, 4])
    got = sh.silhouette(x, labels, measure)
    assert np.all(got.s == 0) and np.all(got.a == 0) and np.all(got.b == 0) and np.all(got.gap == 0)
    assert np.array_equal(got.neighbour, np.where(labels == 2, 4, 2))


@pytest.mark.parametrize("measure", sh.MEASURES)
def test_duplicates_are_pairs_and_only_the_own_id_is_left_out(measure):
    g = sh.planted_gammas(6, 12).copy(order="F")
    g[:, 4] = g[:, 1]                                       # a duplicate inside cluster 0
    g[:, 9] = g[:, 1]                                       # and one in cluster 1
    g[:, 11] = g[:, 10]                                     # cluster 2 is two equal rows
    x = dh.rows(g, measure)
    labels = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2])
    got = sh.silhouette(x, labels, measure)
    d, _ = sh.pair_distances(x, measure)
    assert d[1, 4] < 1e-8 and d[1, 9] < 1e-8 and np.all(np.diag(d) == 0)
    # the duplicate counts in the mean: a(1) has four terms, one of them (about) zero
    assert abs(float(got.a[1] - (d[1, 0] + d[1, 2] + d[1, 3] + d[1, 4]) / 4)) < 1e-18
    assert got.a[10] < 1e-8 and got.s[10] > 1 - 1e-7        # a pair at distance 0, far from the rest
    want = _plain(x, labels, measure)
    assert np.max(np.abs(want[0] - got.s.astype(np.float64))) < 1e-7 and np.array_equal(want[3], got.neighbour)


def test_cosine_sums_have_a_closed_form():
    """sum_{j in c} (1 - s_ij) = n_c - <x_i, S_c> with S_c the sum of the members' rows (no clamp bites
    on these inputs)."""
    K, N, C = 17, 300, 7
    x = dh.rows(sh.planted_gammas(K, N), "cosine")
    labels = sh.labels_of(x, C, "cosine")
    got = sh.silhouette(x, labels, "cosine")
    xl = x.astype(LD)
    for c in range(C):
        members = labels == c
        n = int(members.sum())
        total = n - xl.dot(xl[members].sum(axis=0))
        others = ~members
        assert np.max(np.abs(got.means[others, c] - total[others] / n)) < 1e-17
        if n > 1:
            # (the own pair: 1 - <x_i, x_i>, left out by id)
            own = (total[members] - (1 - (xl[members] * xl[members]).sum(axis=1))) / (n - 1)
            assert np.max(np.abs(got.a[members] - own)) < 1e-17


@pytest.mark.parametrize("measure", sh.MEASURES)
@pytest.mark.parametrize("N,C", sh.NCS)
@pytest.mark.parametrize("K", sh.KS)
def test_no_neighbour_is_a_near_tie_on_the_shapes_of_the_gpu_test(K, N, C, measure):
    x = dh.rows(sh.planted_gammas(K, N), measure)
    labels = sh.labels_of(x, C, measure)
    sizes = np.bincount(labels, minlength=C)
    assert np.count_nonzero(sizes) >= 2
    got = sh.silhouette(x, labels, measure)
    assert np.all(np.abs(got.s) <= 1) and np.all(got.a >= 0) and np.all(got.b >= 0)
    assert np.all(got.s[sizes[labels] == 1] == 0)
    if K == 1:
        assert np.all(got.s == 0) and np.all(got.gap[np.isfinite(got.gap)] == 0)
        return
    finite = np.isfinite(got.gap)
    assert np.all(finite == (np.count_nonzero(sizes) > 2))  # (two clusters: one other mean, no runner-up)
    if finite.any():
        share = got.gap[finite] / got.gap_bound[finite]
        assert share.min() > 100, (float(share.min()), float(got.gap[finite].min()))
    # nothing is degenerate here: the silhouette's own bound stays far below what is compared
    assert got.ds.max() < 1e-9, got.ds.max()


# ---- what DocumentIndex.silhouette refuses before it needs a device -----------------------------------
def test_labels_and_ids_are_checked_in_python():
    from trlda_amd import index
    lab, C = index._silhouette_labels([0, 2, 2, 0, 5], 5)
    assert lab.dtype == np.int32 and lab.flags.c_contiguous and C == 6 and lab.tolist() == [0, 2, 2, 0, 5]
    lab, C = index._silhouette_labels(np.array([1, 0], dtype=np.uint8)[::1], 2)
    assert C == 2 and lab.dtype == np.int32
    assert index._silhouette_labels(np.array([0, index.MAX_CLUSTERS - 1]), 2)[1] == index.MAX_CLUSTERS
    for bad in ([0.0, 1.0], ["a", "b"], [True, False], None):
        with pytest.raises(TypeError):
            index._silhouette_labels(bad, 2)
    for bad, n in (([0, 1, 1], 2), ([0], 2), ([[0, 1]], 2), ([0, -1], 2), ([0, index.MAX_CLUSTERS], 2), ([], 0)):
        with pytest.raises(RuntimeError):
            index._silhouette_labels(np.array(bad, dtype=np.int64), n)
    for bad in ([0, 0, 0], [3, 3, 3], [7]):
        with pytest.raises(ValueError):
            index._silhouette_labels(bad, len(bad))
    assert index._silhouette_ids(None, 5) is None
    ids = index._silhouette_ids([4, 0, 4], 5)
    assert ids.dtype == np.int64 and ids.tolist() == [4, 0, 4]
    for bad in ([0.5], ["a"]):
        with pytest.raises(TypeError):
            index._silhouette_ids(bad, 5)
    for bad in ([5], [-1], [[0, 1]], np.array([], dtype=np.int64), 3):
        with pytest.raises(RuntimeError):
            index._silhouette_ids(bad, 5)


def test_symbol_is_bound():
    import ctypes as C
    from trlda_amd import _ffi
    assert "trlda_docindex_silhouette" in _ffi.EXPORTED_SYMBOLS
    restype, argtypes = _ffi._SIGNATURES["trlda_docindex_silhouette"]
    assert restype is C.c_int and len(argtypes) == 9 and argtypes[4] is C.c_int64
    from trlda_amd.index import DocumentIndex
    assert callable(DocumentIndex.silhouette) and callable(DocumentIndex.select_num_clusters)
