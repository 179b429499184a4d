"""The silhouette of a DocumentIndex on the GPU (csrc/silhouette_kernels.h): s, a, b and
neighbour against the longdouble restatement (tests/silhouette_host.py) on the device's own rows within
the derived per-document bounds; the bitwise invariances -- slabs, how the index was filled, two calls,
a subset of rows, the clusters' names, the other clusters; duplicates, singletons, one topic; the model's
state, the buffers and the errors; and select_num_clusters on planted groups.

Every array is small: at most 1100 indexed documents, 130 topics and 65 clusters.  The restatement's
near-tie report -- how far any neighbour is from a different answer -- stays above 100 bounds on the
shapes here (tests/test_silhouette_host.py asserts it on the host's rows, the tests here on the
device's), so no document is let off on them: every neighbour is compared.

With one topic every row is [1]: one nearest-centroid assignment knows a single cluster, which a
silhouette refuses, so K = 1 takes the labels id mod C (silhouette_host.labels_of).

Observed on the MI355X, as shares of the bounds of tests/silhouette_host.py: every
neighbour equal to the restatement's on all 128 shapes; a at most 5.5 % of its bound (K = 17, N = 300,
C = 65, cosine), b at most 6.7 % (K = 15, N = 2, C = 2, cosine), s at most 1.8 % (K = 17, N = 300, C = 65,
cosine); the smallest near-tie gap 4.6e-7 (K = 15, N = 300, C = 65, hellinger), 3.2e7 of that document's
bounds; with planted duplicates a and b at most 21 % (hellinger)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import silhouette_host as sh

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
MAX_CLUSTERS = 4096


@pytest.fixture(scope="module")
def hip():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


def _model(K, V=8, lam=None, alpha=.1, eta=.3):
    """An OnlineLDA holding `lam` without the constructor's K V 100 draws."""
    from trlda_amd.models import OnlineLDA
    if lam is None:
        lam = np.random.RandomState(77).gamma(2.0, 1.0, size=(K, V)) + 0.05
    m = OnlineLDA.__new__(OnlineLDA)
    m._num_documents = 1000
    m._update_count = 0
    m._ada_tau = 1000.
    m._ada_rho = 1. / m._ada_tau
    m._ada_sq_norm = 1.
    m._setup(V, K, alpha, eta, None, _lambda=np.asfortranarray(lam))
    return m


def _filled(m, measure, g):
    ix = m.document_index(measure)
    ix.add_gamma(g)
    return ix


def _labels(ix, C):
    """One nearest-centroid assignment under the documents init_ids(N, C) (id mod C with one topic)."""
    N = len(ix)
    if ix._K == 1:
        return (np.arange(N) % C).astype(np.int32)
    ids = sh.init_ids(N, C)
    return ix.nearest_centroid(np.asfortranarray(np.stack([ix._theta(int(i)) for i in ids], axis=1)))


def _state():
    from trlda_amd import _ffi
    s = np.zeros(33, dtype=np.uint32)
    _ffi.lib().trlda_rng_get_state(s)
    return s


def _live():
    from trlda_amd import _ffi
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return live.value


def _same(p, q):
    return all(np.array_equal(v, w) for v, w in zip(p, q))


def _check_neighbours(neighbour, ref, cap):
    """`neighbour` is the restatement's; a document is let off only if its gap is below twice its
    bound, and then the device's choice is a cluster whose mean is within the bound of the smallest.
    At most `cap` documents are let off."""
    off = np.flatnonzero(neighbour != ref.neighbour)
    for i in off:
        c = int(neighbour[i])
        assert ref.gap[i] < 2 * ref.gap_bound[i], (i, ref.gap[i], ref.gap_bound[i])
        assert np.isfinite(ref.means[i, c]) and float(ref.means[i, c] - ref.b[i]) <= ref.dmeans[i, c] + ref.db[i], i
    assert len(off) <= cap, (len(off), cap)


def _shares(got, ref, keep=None):
    """The largest |device - restatement| / bound of a, b and s (s over `keep` only)."""
    s, a, b, _ = got
    single = ref.sizes[ref.own] == 1
    assert np.all(s[single] == 0.0) and np.all(a[single] == 0.0)
    many = ~single
    out = []
    for name, dev, want, bound, where in (("a", a, ref.a, ref.da, many), ("b", b, ref.b, ref.db, np.ones(len(a), bool)),
                                          ("s", s, ref.s, ref.ds, many if keep is None else many & keep)):
        if not where.any():
            out.append(0.0)
            continue
        err = np.abs(dev.astype(LD) - want).astype(np.float64)[where]
        share = float(np.max(err / bound[where]))
        assert share <= 1.0, (name, share, int(np.argmax(err / bound[where])))
        out.append(share)
    return out


def _reference(ix, labels, ids=None):
    ref = sh.silhouette(ix.rows(), labels, ix.measure, ids=ids)
    ref.own = labels if ids is None else labels[np.asarray(ids)]
    return ref


# 1. against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("measure", sh.MEASURES)
@pytest.mark.parametrize("N,C", sh.NCS)
@pytest.mark.parametrize("K", sh.KS)
def test_against_the_restatement(hip, K, N, C, measure):
    m = _model(K)
    ix = _filled(m, measure, sh.planted_gammas(K, N))
    labels = _labels(ix, C)
    ref = _reference(ix, labels)
    got = ix.silhouette(labels, return_parts=True)
    s, a, b, neighbour = got
    assert s.dtype == a.dtype == b.dtype == np.float64 and neighbour.dtype == np.int32
    assert s.shape == a.shape == b.shape == neighbour.shape == (N,)
    assert np.array_equal(ix.silhouette(labels), s)
    assert np.all(np.abs(s) <= 1.0) and np.all(a >= 0.0) and np.all(b >= 0.0)
    if K == 1:
        # (every row is [1], every s_ij exactly 1, every distance exactly 0)
        assert np.all(s == 0.0) and np.all(a == 0.0) and np.all(b == 0.0)
        assert np.array_equal(neighbour, ref.neighbour)
        m.close()
        return
    finite = np.isfinite(ref.gap)
    if finite.any():
        assert np.min(ref.gap[finite] / ref.gap_bound[finite]) > 100
    _check_neighbours(neighbour, ref, 0)                     # (planted shapes: nobody is let off)
    assert ref.ds.max() <= 1e-3                              # (and no silhouette is skipped)
    share = _shares(got, ref)
    print("K = %d N = %d C = %d %s: err / bound a %.3f b %.3f s %.3f, smallest gap %.2e (%.0f bounds), sizes %d..%d"
          % (K, N, C, measure, share[0], share[1], share[2], ref.gap.min(),
             np.min(ref.gap / ref.gap_bound) if finite.any() else np.inf, ref.sizes.min(), ref.sizes.max()))
    m.close()


# 2. the bitwise invariances ---------------------------------------------------------------------------
@pytest.mark.parametrize("measure", sh.MEASURES)
def test_results_do_not_depend_on_slabs_fill_subset_names_or_other_clusters(hip, measure):
    """1100 documents at K = 17 in 5 clusters of more than 16 members: slabs of 16, 64 and 2048 rows;
    ragged adds of 7 without reserve (the table is copied as it grows) and the device-pointer form; two
    calls; a permuted subset with repeats; the label values renamed (with values without members among
    them); and an index of two of the clusters only."""
    from trlda_amd import _ffi
    K, N, n_clusters = 17, 1100, 5
    g = sh.planted_gammas(K, N)
    m = _model(K)
    whole = m.document_index(measure)
    whole.reserve(N)
    whole.add_gamma(g)
    labels = _labels(whole, n_clusters)
    sizes = np.bincount(labels, minlength=n_clusters)
    assert sizes.min() > 16 and np.any(sizes % 16)
    base = whole.silhouette(labels, return_parts=True)
    assert _same(whole.silhouette(labels, return_parts=True), base)
    for slab in (16, 64, 0):
        whole.set_slab_rows(slab)
        assert _same(whole.silhouette(labels, return_parts=True), base)
    parts = m.document_index(measure)
    for at in range(0, N, 7):
        assert parts.add_gamma(g[:, at:at + 7]) == at
    dev = m.document_index(measure)
    ptr = _ffi.vp()
    _ffi.check(hip.trlda_dev_alloc(0, g.nbytes, C.byref(ptr)))
    try:
        _ffi.check(hip.trlda_dev_upload(0, ptr, g.ctypes.data, g.nbytes))
        assert dev.add_gamma_device(ptr, N) == 0
        _ffi.check(hip.trlda_model_synchronize(m._handle))
    finally:
        hip.trlda_dev_free(0, ptr)
    for other in (parts, dev):
        assert len(other) == N and np.array_equal(other.rows(), whole.rows())
        assert _same(other.silhouette(labels, return_parts=True), base)
    # a permuted subset with repeats, across more than one block of 128 rows and a single row
    rng = np.random.RandomState(8)
    for ids in (rng.permutation(N)[:301], np.concatenate([rng.randint(N, size=140), [N - 1, 0, N - 1]]), [513]):
        ids = np.asarray(ids)
        sub = whole.silhouette(labels, ids=ids, return_parts=True)
        assert sub[0].shape == (len(ids),) and _same(sub, [v[ids] for v in base])
        assert np.array_equal(whole.silhouette(labels, ids=list(ids)), base[0][ids])
    # the clusters renamed: 0..4 -> 40, 3, 17, 0, 64 (most values in [0, 65) have no member)
    ref = _reference(whole, labels)
    assert np.all(ref.gap > 0)                               # (no exact tie: the names cannot show)
    names = np.array([40, 3, 17, 0, 64], dtype=np.int32)
    renamed = whole.silhouette(names[labels], return_parts=True)
    assert _same(renamed[:3], base[:3]) and np.array_equal(renamed[3], names[base[3]])
    # an index of the members of two of the clusters: the same a; the same b where the other of the
    # two was the neighbour
    pair = [int(c) for c in np.argsort(-sizes, kind="stable")[:2]]
    keep = np.flatnonzero((labels == pair[0]) | (labels == pair[1]))
    assert len(keep) < N
    small = _filled(m, measure, g[:, keep])
    got = small.silhouette(np.where(labels[keep] == pair[0], 0, 1), return_parts=True)
    assert np.array_equal(got[1], base[1][keep])
    other = np.where(labels[keep] == pair[0], pair[1], pair[0])
    there = base[3][keep] == other
    assert there.sum() > 10
    assert np.array_equal(got[2][there], base[2][keep][there]) and np.array_equal(got[0][there], base[0][keep][there])
    assert np.array_equal(got[3], np.where(labels[keep] == pair[0], 1, 0))
    m.close()


# 3. duplicates, singletons ----------------------------------------------------------------------------
@pytest.mark.parametrize("measure", sh.MEASURES)
def test_duplicates_and_singletons(hip, measure):
    """40 documents at K = 6.  Cluster 0 holds document 1 and a copy of it (4); cluster 1 holds another
    copy (9); cluster 2 is document 10 and two equal rows 11, 12 (10 is its only non-duplicate);
    clusters 3 = {13, 14} and 4 = {15, 16} are four copies of one row that is nobody else's, so for
    those four a and b are rounding alone and the silhouette is not compared; 5 and 7 are singletons
    (17, 18), 6 has no member."""
    K, N = 6, 40
    g = sh.planted_gammas(K, N).copy(order="F")
    g[:, 4] = g[:, 1]
    g[:, 9] = g[:, 1]
    g[:, 12] = g[:, 11]
    for i in (14, 15, 16):
        g[:, i] = g[:, 13]
    labels = np.array([0] * 5 + [1] * 5 + [2] * 3 + [3] * 2 + [4] * 2 + [5, 7] + [0] * 11 + [1] * 10, dtype=np.int32)
    m = _model(K)
    ix = _filled(m, measure, g)
    ref = _reference(ix, labels)
    got = ix.silhouette(labels, return_parts=True)
    s, a, b, neighbour = got
    # the pair of copies is a pair: a(1) counts document 4 at distance (about) 0, and leaves out 1 alone
    d, _ = sh.pair_distances(ix.rows(), measure)
    assert d[1, 4] < 1e-7 and abs(a[1] - float(d[1, labels == 0].sum() / 15)) <= ref.da[1]
    _check_neighbours(neighbour, ref, 0)
    skipped = np.flatnonzero(ref.ds > 1e-3)
    assert np.array_equal(skipped, [13, 14, 15, 16])
    keep = np.ones(N, dtype=bool)
    keep[skipped] = False
    share = _shares(got, ref, keep)
    assert np.all(a[[13, 14, 15, 16]] < 1e-7) and np.all(b[[13, 14, 15, 16]] < 1e-7)
    assert np.all(np.abs(s) <= 1.0)
    assert neighbour[13] == neighbour[14] == 4 and neighbour[15] == neighbour[16] == 3
    # equal rows of one cluster: the same sums but for the partner's place
    assert b[11] == b[12] and neighbour[11] == neighbour[12] and a[11] == a[12]
    assert a[11] < a[10]                                    # (10 is far from the two copies, they are not from each other)
    # singletons
    assert s[17] == s[18] == 0.0 and a[17] == a[18] == 0.0 and b[17] > 0.0 and b[18] > 0.0
    assert neighbour[17] != 5 and neighbour[18] != 7 and np.all(neighbour != 6)
    print("%s: err / bound a %.3f b %.3f s %.3f" % (measure, share[0], share[1], share[2]))
    # two singletons are an index
    two = _filled(m, measure, g[:, :2])
    r = two.silhouette([1, 0], return_parts=True)
    assert np.all(r[0] == 0.0) and np.all(r[1] == 0.0) and r[2][0] == r[2][1] > 0 and r[3].tolist() == [0, 1]
    m.close()


# 4. the model's state ---------------------------------------------------------------------------------
def test_state_is_left_alone(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K, N = 16, 40
    m = _model(K, alpha=.2, eta=.05)
    ix = _filled(m, "hellinger", sh.planted_gammas(K, N))
    rows = ix.rows()
    rng = np.random.RandomState(31)
    docs = [[(int(w), int(rng.randint(1, 5))) for w in rng.choice(8, size=rng.randint(2, 7), replace=False)]
            for _ in range(9)]
    _, sstats = m.update_variables(docs, latents=np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 9)) + 0.1),
                                   max_iter=20)
    held = np.empty((K, 8), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, held))
    assert np.array_equal(held, sstats) and np.any(held > 0)
    before = (np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count)
    labels = _labels(ix, 4)
    kept = labels.copy()
    trlda_amd.seed(9)
    state = _state()
    ix.silhouette(labels)
    ix.silhouette(labels, ids=[3, 3, 39], return_parts=True)
    assert np.array_equal(state, _state()) and np.array_equal(labels, kept)
    assert len(ix) == N and np.array_equal(ix.rows(), rows)
    assert np.array_equal(np.asarray(m.lambdas), before[0]) and np.array_equal(np.asarray(m.alpha), before[1])
    assert m.eta == before[2] and m.update_count == before[3]
    after_stats = np.empty((K, 8), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, after_stats))
    assert np.array_equal(after_stats, held)                      # the model's statistics: no E-step ran
    m.close()


def test_no_buffer_is_kept_by_the_calls(hip):
    """A fresh process (the count is the process's): the calls, the refused ones included, leave the
    live count as it was, and after close() the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "silhouette_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout


# 5. the errors ----------------------------------------------------------------------------------------
def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K, N = 8, 12
    m = _model(K)
    ix = m.document_index("cosine")
    g = sh.planted_gammas(K, N)
    labels = (np.arange(N) % 3).astype(np.int32)
    trlda_amd.seed(3)
    before = _state()
    s, a, b = np.full(N + 1, -7.), np.full(N + 1, -7.), np.full(N + 1, -7.)
    nbr = np.full(N + 1, -7, dtype=np.int32)

    def call(handle, lab, n_clusters, ids=None, count=0, out=s):
        return hip.trlda_docindex_silhouette(handle, None if lab is None else lab.ctypes.data, n_clusters,
                                             None if ids is None else ids.ctypes.data, count,
                                             None if out is None else out.ctypes.data, a.ctypes.data, b.ctypes.data,
                                             nbr.ctypes.data)

    live = _live()
    # an empty index
    assert call(ix._handle, labels, 3) == _ffi.ERR_ARG
    with pytest.raises(RuntimeError, match="empty"):
        ix.silhouette(labels)
    assert _live() == live
    ix.add_gamma(g)
    live = _live()
    ids = np.array([0, 5], dtype=np.int64)
    # NULL arguments, the number of label values, ids without an id
    assert call(None, labels, 3) == _ffi.ERR_ARG and call(ix._handle, None, 3) == _ffi.ERR_ARG
    assert call(ix._handle, labels, 3, out=None) == _ffi.ERR_ARG
    for n_clusters in (1, 0, -1, MAX_CLUSTERS + 1):
        assert call(ix._handle, labels, n_clusters) == _ffi.ERR_ARG
    assert call(ix._handle, labels, 3, ids, 0) == _ffi.ERR_ARG and call(ix._handle, labels, 3, ids, -1) == _ffi.ERR_ARG
    assert _live() == live
    # values: a label outside [0, C), an id outside [0, N), fewer than two clusters with members
    for at, bad in ((0, 3), (N - 1, -1), (4, MAX_CLUSTERS)):
        lab = labels.copy()
        lab[at] = bad
        assert call(ix._handle, lab, 3) == _ffi.ERR_VALUE
    for bad in (N, -1):
        assert call(ix._handle, labels, 3, np.array([0, bad], dtype=np.int64), 2) == _ffi.ERR_VALUE
    assert call(ix._handle, np.full(N, 2, dtype=np.int32), 3) == _ffi.ERR_VALUE
    assert call(ix._handle, np.full(N, 2, dtype=np.int32), MAX_CLUSTERS) == _ffi.ERR_VALUE
    assert _live() == live
    # the same through Python
    for bad, error in ((labels[:-1], RuntimeError), (np.append(labels, 0), RuntimeError), (labels - 1, RuntimeError),
                       (labels * 2048, RuntimeError), (labels.reshape(1, N), RuntimeError),
                       (labels.astype(np.float64), TypeError), (["a"] * N, TypeError),
                       (np.zeros(N, dtype=np.int64), ValueError), (np.full(N, 5), ValueError)):
        with pytest.raises(error):
            ix.silhouette(bad)
        assert _live() == live
    for bad, error in (([N], RuntimeError), ([-1, 0], RuntimeError), ([], RuntimeError), ([[0]], RuntimeError),
                       ([0.5], TypeError)):
        with pytest.raises(error):
            ix.silhouette(labels, ids=np.array(bad) if bad else np.array([], dtype=np.int64))
        assert _live() == live
    # nothing was drawn or written
    assert np.all(s == -7.) and np.all(a == -7.) and np.all(b == -7.) and np.all(nbr == -7)
    assert len(ix) == N and np.array_equal(before, _state()) and _live() == live
    with pytest.raises(ValueError):
        ix.select_num_clusters(())
    with pytest.raises(RuntimeError, match="num_clusters"):
        ix.select_num_clusters((N + 1, 2))
    assert np.array_equal(before, _state()) and _live() == live
    # the largest label value allowed; the index still works after the refusals
    lab = labels.copy()
    lab[lab == 2] = MAX_CLUSTERS - 1
    top = ix.silhouette(lab, return_parts=True)
    plain = ix.silhouette(labels, return_parts=True)
    assert _same(top[:3], plain[:3]) and set(top[3]) <= {0, 1, MAX_CLUSTERS - 1}
    assert _live() == live
    ix.close()
    live = _live()
    for refused in (lambda: ix.silhouette(labels), lambda: ix.select_num_clusters((2, 3))):
        with pytest.raises(RuntimeError, match="closed"):
            refused()
        assert _live() == live
    m.close()


# 6. choosing C ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", sh.MEASURES)
def test_select_num_clusters_finds_the_planted_four(hip, measure):
    """240 gammas around 4 well-separated Dirichlet centres at K = 17 (those of tests/test_gpu_cluster.py).
    Seed 1: under the restatement of the loop (tests/cluster_host.py) the draws of this seed let
    C = 4 recover the four groups for both measures, where other seeds end with a group split."""
    import trlda_amd
    from trlda_amd.utils import random_select
    K, groups, per = 17, 4, 60
    rng = np.random.RandomState(123)
    truth = np.repeat(np.arange(groups), per)
    rng.shuffle(truth)
    centre = np.full((groups, K), 0.2)
    for c in range(groups):
        centre[c, 4 * c:4 * c + 4] = 25.0
    g = np.asfortranarray(np.stack([rng.dirichlet(centre[t]) * rng.uniform(5., 50.) + 1e-3 for t in truth], axis=1))
    N = groups * per
    m = _model(K)
    ix = _filled(m, measure, g)
    candidates = (2, 3, 4, 6, 8)
    trlda_amd.seed(1)
    best, scores = ix.select_num_clusters(candidates)
    after = _state()
    assert best == 4 and list(scores) == list(candidates)
    assert scores[4] > 0.8 and all(scores[c] < scores[4] - 0.1 for c in candidates if c != 4), scores
    # by hand from the same seed: one random_select per candidate, in the order given, and nothing else
    trlda_amd.seed(1)
    for n_clusters in candidates:
        labels, _ = ix.cluster(n_clusters, init=random_select(n_clusters, N), max_iter=50)
        s = ix.silhouette(labels)
        assert scores[n_clusters] == math.fsum(s) / N
        if n_clusters == 4:
            assert len(set(zip(labels.tolist(), truth.tolist()))) == 4      # the planted groups
    assert np.array_equal(after, _state())
    # a subsample, and fewer updates
    trlda_amd.seed(1)
    ids = np.arange(0, N, 5)
    best_s, scores_s = ix.select_num_clusters(candidates, max_iter=50, ids=ids)
    assert best_s == 4 and np.array_equal(after, _state())
    trlda_amd.seed(1)
    labels, _ = ix.cluster(2, init=random_select(2, N))
    assert scores_s[2] == math.fsum(ix.silhouette(labels, ids=ids)) / len(ids)
    # mean descending, C ascending: a candidate that cannot be scored comes last
    trlda_amd.seed(1)
    best_1, scores_1 = ix.select_num_clusters((1, 2))
    assert scores_1[1] == -math.inf and best_1 == 2
    m.close()
