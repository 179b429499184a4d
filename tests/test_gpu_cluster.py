"""The document groups of a DocumentIndex on the GPU (csrc/cluster_kernels.h): one
assignment and the whole trajectory of the loop against the restatement (tests/cluster_host.py) on the
device's own rows; exact ties, independence of the slab, of how the index was filled and of the other
clusters, the model's state, the buffers and the errors, and planted groups.

Every array is small: at most 1100 indexed documents, 130 topics and 65 clusters.  The restatement's
margin -- how far any label of any assignment is from a different answer -- stays above GAP_FLOOR on
these inputs (tests/test_cluster_host.py asserts it on the host's rows, the tests here on the
device's), so every label of every document is compared: none is left out.

Observed on the MI355X, as shares of the bounds below: every label, `iterations`,
`converged` and size equal to the restatement's on all 160 cases; a similarity at most 11 % of
(K + 16) u from the longdouble dot (K = 16, N = 300, C = 65, hellinger); a centroid at most 2.6 % of
4 (n_c + K + 16) u from the restated theta^ (K = 3, N = 300, C = 65, hellinger); the objective never
rose between the prefixes (largest rise 0.0); at most 42 updates (K = 17, N = 1100, C = 5, hellinger);
the smallest margin 4.8e-8 (K = 63, N = 1100, C = 5, cosine)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_host as ch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
GAP_FLOOR = 1e-9
MEASURES = ["hellinger", "cosine"]
KS = [1, 3, 15, 16, 17, 63, 65, 130]               # the Kp tail, the MFMA edge, the chunk-of-32 edge, several chunks
# centroid tile edges, more than one group of 64, C = N, the growth copy at 1100
NCS = [(300, 1), (300, 2), (300, 7), (300, 16), (300, 17), (300, 65), (1100, 5), (17, 17), (2, 2), (1, 1)]
MAX_CLUSTERS = 4096


def sim_bound(K):
    """|s_dev - longdouble dot|: a chain of Kp / 4 + 3 roundings on sum |x m| <= 1 (Cauchy-Schwarz on
    unit rows)."""
    return (K + 16) * U


def centroid_bound(n_c, K):
    """|theta^_dev - theta^_restated| per column: n_c additions on S, K on the norm and the division
    give a relative (2 n_c + K + ...) u on m, doubled by the Hellinger square (or by the cosine's
    division by sum m), on values <= 1."""
    return 4 * (n_c + K + 16) * U


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


def _gammas(K, n, seed):
    """n gamma columns: sparse-ish topic weights of very different totals."""
    rng = np.random.RandomState(seed)
    g = rng.gamma(0.3, 1.0, size=(K, n)) + 0.01
    return np.asfortranarray(g * rng.uniform(0.5, 40.0, size=n))


def _case(K, N):
    return _gammas(K, 1100, 4000 + K)[:, :N]


def _init_ids(N, C):
    return np.linspace(0, N - 1, C).astype(int)


def _filled(m, measure, g):
    ix = m.document_index(measure)
    ix.add_gamma(g)
    return ix


def _theta(ix, ids):
    """theta^ of the documents `ids`, K x C, as DocumentIndex.cluster forms it from given ids."""
    return np.asfortranarray(np.stack([ix._theta(int(i)) for i in ids], axis=1))


def _rows_of(m, measure, centroids):
    """The device's rows of the centroid columns: what add_gamma stores for them."""
    other = _filled(m, measure, centroids)
    rows = other.rows()
    other.close()
    return rows


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


def _same(a, b):
    """Two results of cluster(..., return_info=True), bitwise."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]["iterations"] == b[2]["iterations"]
            and a[2]["converged"] == b[2]["converged"] and np.array_equal(a[2]["sizes"], b[2]["sizes"])
            and np.array_equal(a[2]["similarity"], b[2]["similarity"]) and a[2]["objective"] == b[2]["objective"])


# 1. one assignment ------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("N,C", NCS)
@pytest.mark.parametrize("K", KS)
def test_one_assignment(hip, K, N, C, measure):
    g = _case(K, N)
    m = _model(K)
    ix = _filled(m, measure, g)
    ids = _init_ids(N, C)
    c0 = _theta(ix, ids)
    x, crows = ix.rows(), _rows_of(m, measure, c0)
    want, s, margin = ch.assign(x, crows)
    labels, sim = ix.nearest_centroid(c0, return_similarity=True)
    assert labels.dtype == np.int32 and sim.dtype == np.float64 and labels.shape == sim.shape == (N,)
    if K == 1:
        # (the one topic holds every document whole: every row is [1], every s exactly 1, every label 0)
        assert np.all(sim == 1.0) and np.all(labels == 0)
    else:
        assert margin.min() > GAP_FLOOR, margin.min()
    assert np.array_equal(labels, want)
    err = float(np.max(np.abs(sim.astype(LD) - s)))
    print("K = %d N = %d C = %d %s: sim err / bound %.3f, smallest margin %.2e"
          % (K, N, C, measure, err / sim_bound(K), margin.min()))
    assert err <= sim_bound(K), err / U
    assert np.array_equal(ix.nearest_centroid(c0), labels)
    # the same columns, given rather than indexed
    labels_g, sim_g = ix.nearest_centroid(c0, gamma=g, return_similarity=True)
    assert np.array_equal(labels_g, labels) and np.array_equal(sim_g, sim)
    one = ix.nearest_centroid(c0, gamma=g[:, N - 1])
    assert one.shape == (1,) and one[0] == labels[N - 1]
    # the loop without an update, from the array and from the ids
    for init in (c0, ids):
        labels_0, cent_0, info = ix.cluster(C, init=init, max_iter=0, return_info=True)
        assert np.array_equal(labels_0, labels) and np.array_equal(info["similarity"], sim)
        assert info["iterations"] == 0 and info["converged"] is False
        assert np.array_equal(info["sizes"], np.bincount(want, minlength=C)) and info["sizes"].dtype == np.int64
        assert cent_0.shape == (K, C) and cent_0.flags.f_contiguous and cent_0.dtype == np.float64
        assert np.max(np.abs(cent_0.astype(LD) - ch.theta_hat(crows, measure))) <= centroid_bound(0, K)
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_initial_centroids_from_ids_are_the_documents_theta(hip, measure):
    """theta^ read back from a stored row is gamma / sum(gamma) again.  A stored row is within
    ROW_BOUND of tests/test_gpu_docindex.py of the NumPy row, relatively: 4 u (hellinger), 8 u (cosine).
    hellinger squares it, 2 * 4 u and the product's u / 2; cosine divides it by the sum of the row,
    which carries the rows' 8 u and its own order of addition (5 u, as there) and the quotient's u / 2:
    10 u and 24 u cover these.  Through the rows kernel and back a second time: twice that."""
    K, N = 17, 40
    bound = {"hellinger": 10 * U, "cosine": 24 * U}[measure]
    g = _case(K, N)
    m = _model(K)
    ix = _filled(m, measure, g)
    theta = g / g.sum(axis=0)
    for i in (0, 7, N - 1):
        got = ix._theta(i)
        assert got.shape == (K,) and np.max(np.abs(got - theta[:, i]) / theta[:, i]) <= bound
    ids = [3, 0, 39]
    _, cent = ix.cluster(3, init=ids, max_iter=0)
    assert np.max(np.abs(cent - theta[:, ids]) / theta[:, ids]) <= 2 * bound
    m.close()


# 2. the trajectory ------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("N,C", NCS)
@pytest.mark.parametrize("K", KS)
def test_trajectory(hip, K, N, C, measure):
    g = _case(K, N)
    m = _model(K)
    ix = _filled(m, measure, g)
    c0 = _theta(ix, _init_ids(N, C))
    x, crows = ix.rows(), _rows_of(m, measure, c0)
    ref = ch.run(x, crows, 50)
    assert ref.converged
    if K > 1:
        assert ref.margin > GAP_FLOOR, ref.margin
    objective, share = [], 0.0
    for max_iter in (0, 1, 2, 3, 50):
        labels, cent, info = ix.cluster(C, init=c0, max_iter=max_iter, return_info=True)
        j, iterations, converged = ref.after(max_iter)
        assert np.array_equal(labels, ref.labels[j]), (max_iter, int(np.sum(labels != ref.labels[j])))
        assert info["iterations"] == iterations and info["converged"] is converged
        assert np.array_equal(info["sizes"], ref.sizes(j))
        # the members that made centroid c: those of the assignment before the last update
        n_c = ref.sizes(j - 1) if j else np.zeros(C)
        err = np.max(np.abs(cent.astype(LD) - ch.theta_hat(ref.rows[j], measure)), axis=0).astype(np.float64)
        assert np.all(err <= centroid_bound(n_c, K)), (max_iter, float(np.max(err / centroid_bound(n_c, K))))
        share = max(share, float(np.max(err / centroid_bound(n_c, K))))
        # (s moves by no more than its centroid row does: |<x, dm>| <= |dm| on a unit row x)
        s_err = float(np.max(np.abs(info["similarity"].astype(LD) - ref.similarity[j])))
        assert s_err <= sim_bound(K) + centroid_bound(n_c.max(), K), s_err / U
        objective.append(info["objective"])
    rise = max(b - a for a, b in zip(objective, objective[1:]))
    assert rise <= N * sim_bound(K), (objective, rise)
    print("K = %d N = %d C = %d %s: %d updates, centroid err / bound %.3f, objective %.6g -> %.6g (largest rise %.2e), "
          "smallest margin %.2e" % (K, N, C, measure, ref.iterations, share, objective[0], objective[-1], rise,
                                    ref.margin))
    m.close()


# 3. exact ties ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
def test_duplicate_centroids_leave_the_later_one_empty(hip, measure):
    """Clusters 7 and 8 start as copies of 2 and 0: every tie goes to the smaller c, so the first
    assignment leaves the copies empty, and an empty cluster keeps its row through the update.  (Once
    the original has moved, the copy -- still where it started -- may win documents: that is Lloyd's
    algorithm, and nothing is asked of the later labels here.)"""
    K, N = 17, 300
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    c7 = _theta(ix, _init_ids(N, 7))
    c9 = np.asfortranarray(np.concatenate([c7, c7[:, 2:3], c7[:, 0:1]], axis=1))
    labels, cent, info = ix.cluster(9, init=c9, max_iter=0, return_info=True)
    labels_7, cent_7, info_7 = ix.cluster(7, init=c7, max_iter=0, return_info=True)
    assert labels.max() <= 6 and info["sizes"][7] == info["sizes"][8] == 0
    assert np.array_equal(ix.nearest_centroid(c9), labels)
    # the others do not know of the copies
    assert np.array_equal(labels, labels_7) and np.array_equal(info["similarity"], info_7["similarity"])
    assert np.array_equal(info["sizes"][:7], info_7["sizes"]) and np.array_equal(cent[:, :7], cent_7)
    # the copies' columns: theta^ of the rows they came with, which are the originals' rows
    assert np.array_equal(cent[:, 7], cent[:, 2]) and np.array_equal(cent[:, 8], cent[:, 0])
    # one update: the empty clusters keep their rows bit for bit, the others sum the same members
    _, cent_1, info_1 = ix.cluster(9, init=c9, max_iter=1, return_info=True)
    _, cent_71, info_71 = ix.cluster(7, init=c7, max_iter=1, return_info=True)
    assert info_1["iterations"] == info_71["iterations"] == 1
    assert np.array_equal(cent_1[:, 7:], cent[:, 7:]) and np.array_equal(cent_1[:, :7], cent_71)
    assert not np.array_equal(cent_1[:, :7], cent[:, :7])
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_duplicate_documents_share_label_and_similarity(hip, measure):
    K, N = 20, 300
    g = _gammas(K, N, 4000 + K).copy(order="F")
    g[:, 40] = g[:, 3]
    g[:, 299] = g[:, 3]
    m = _model(K)
    ix = _filled(m, measure, g)
    for slab in (16, 0):
        ix.set_slab_rows(slab)
        for max_iter in (0, 2, 50):
            labels, _, info = ix.cluster(7, init=_init_ids(N, 7), max_iter=max_iter, return_info=True)
            assert labels[3] == labels[40] == labels[299]
            assert info["similarity"][3] == info["similarity"][40] == info["similarity"][299]
    m.close()


# 4. independence --------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
def test_results_do_not_depend_on_slabs_or_on_how_the_index_was_filled(hip, measure):
    """1100 documents at K = 17: slabs of 16, 64 and 2048 rows; one add into reserved room, ragged adds
    of 7 without reserve -- the table starts at 1024 rows and is copied into 2048 -- and the
    device-pointer form."""
    from trlda_amd import _ffi
    K, N, n_clusters = 17, 1100, 5
    g = _case(K, N)
    m = _model(K)
    whole = m.document_index(measure)
    whole.reserve(N)
    whole.add_gamma(g)
    c0 = _theta(whole, _init_ids(N, n_clusters))
    base = whole.cluster(n_clusters, init=c0, max_iter=50, return_info=True)
    base_a = whole.nearest_centroid(base[1], return_similarity=True)
    assert base[2]["converged"] and base[2]["iterations"] > 2
    assert _same(whole.cluster(n_clusters, init=c0, max_iter=50, return_info=True), base)
    for slab in (16, 64, 0):
        whole.set_slab_rows(slab)
        assert _same(whole.cluster(n_clusters, init=c0, max_iter=50, return_info=True), base)
        again = whole.nearest_centroid(base[1], return_similarity=True)
        assert np.array_equal(again[0], base_a[0]) and np.array_equal(again[1], base_a[1])
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
        assert _same(other.cluster(n_clusters, init=c0, max_iter=50, return_info=True), base)
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_a_centroid_does_not_depend_on_the_other_clusters(hip, measure):
    """An index of the members of two clusters only, started from their final centroids: one update
    sums the same members in the same order and returns the same bits."""
    K, N, n_clusters = 17, 1100, 5
    g = _case(K, N)
    m = _model(K)
    ix = _filled(m, measure, g)
    labels, cent, info = ix.cluster(n_clusters, init=_init_ids(N, n_clusters), max_iter=50, return_info=True)
    assert info["converged"] and info["sizes"].min() > 0
    # (two clusters whose members lie in more than one chunk of 256 where there are such)
    pair = [int(c) for c in np.argsort(-info["sizes"], kind="stable")[:2]]
    keep = np.flatnonzero((labels == pair[0]) | (labels == pair[1]))
    assert len(keep) < N
    small = _filled(m, measure, g[:, keep])
    labels_s, cent_s, info_s = small.cluster(2, init=cent[:, pair], max_iter=1, return_info=True)
    assert np.array_equal(labels_s, np.where(labels[keep] == pair[0], 0, 1))
    assert info_s["iterations"] == 1 and info_s["converged"] is True
    assert np.array_equal(cent_s, cent[:, pair])
    assert np.array_equal(info_s["similarity"], info["similarity"][keep])
    m.close()


# 5. the model's state ---------------------------------------------------------------------------------
def test_state_is_left_alone(hip):
    import trlda_amd
    from trlda_amd import _ffi
    from trlda_amd.utils import random_select
    K, N = 16, 40
    m = _model(K, alpha=.2, eta=.05)
    ix = _filled(m, "cosine", _case(K, N))
    rows = ix.rows()
    # an E-step first, so that the model's statistics are not trivial
    rng = np.random.RandomState(31)
    docs = [[(int(w), int(rng.randint(1, 5))) for w in rng.choice(8, size=rng.randint(2, 7), replace=False)]
            for _ in range(9)]
    _, sstats = m.update_variables(docs, latents=np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 9)) + 0.1),
                                   max_iter=20)
    held = np.empty((K, 8), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, held))
    assert np.array_equal(held, sstats) and np.any(held > 0)
    before = (np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count)
    c0 = _theta(ix, _init_ids(N, 4))
    kept = c0.copy(order="F")
    trlda_amd.seed(9)
    state = _state()
    labels, cent = ix.cluster(4, init=c0, max_iter=50)
    ix.cluster(4, init=_init_ids(N, 4), max_iter=1)
    ix.nearest_centroid(cent)
    ix.nearest_centroid(cent, gamma=_case(K, 3), return_similarity=True)
    assert np.array_equal(state, _state()) and np.array_equal(c0, kept)
    assert len(ix) == N and np.array_equal(ix.rows(), rows)
    assert np.array_equal(np.asarray(m.lambdas), before[0]) and np.array_equal(np.asarray(m.alpha), before[1])
    assert m.eta == before[2] and m.update_count == before[3]
    after_stats = np.empty((K, 8), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, after_stats))
    assert np.array_equal(after_stats, held)                      # the model's statistics: no E-step ran
    # init=None: one random_select(C, N) from the seeded stream, on the host, and nothing else
    trlda_amd.seed(21)
    first = ix.cluster(4, return_info=True)
    after = _state()
    trlda_amd.seed(21)
    ids = random_select(4, N)
    assert np.array_equal(after, _state()) and not np.array_equal(after, state)
    assert len(set(ids)) == 4
    assert _same(ix.cluster(4, init=ids, return_info=True), first)
    trlda_amd.seed(21)
    assert _same(ix.cluster(4, return_info=True), first)
    m.close()


def test_no_buffer_is_kept_by_the_calls(hip):
    """A fresh process (the count is the process's): the calls, the refused ones included, leave the
    live count as it was, and after close() the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cluster_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout


# 6. the errors ----------------------------------------------------------------------------------------
def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K, N = 8, 12
    m = _model(K)
    ix = m.document_index("cosine")
    g = _case(K, N)
    cent = np.asfortranarray(g[:, :3] / g[:, :3].sum(axis=0))
    trlda_amd.seed(3)
    before = _state()
    labels = np.full(N + 1, -7, dtype=np.int32)
    sim = np.full(N + 1, -7.)
    sizes = np.full(4, -7, dtype=np.int64)
    its, conv = C.c_int(-7), C.c_int(-7)

    def cluster(handle, n_clusters, c, max_iter, labels_out=labels.ctypes.data, its_out=C.byref(its),
                conv_out=C.byref(conv)):
        return hip.trlda_docindex_cluster(handle, n_clusters, None if c is None else c.ctypes.data, max_iter,
                                          labels_out, sim.ctypes.data, sizes.ctypes.data, its_out, conv_out)

    def assign(handle, c, n_clusters, gamma, B, labels_out=labels.ctypes.data):
        return hip.trlda_docindex_assign(handle, None if c is None else c.ctypes.data, n_clusters,
                                         None if gamma is None else gamma.ctypes.data, B, labels_out,
                                         sim.ctypes.data)

    live = _live()
    # an empty index
    assert cluster(ix._handle, 1, cent, 5) == _ffi.ERR_ARG and assign(ix._handle, cent, 1, None, 0) == _ffi.ERR_ARG
    assert assign(ix._handle, cent, 1, g, N) == _ffi.ERR_ARG
    with pytest.raises(RuntimeError, match="num_clusters"):
        ix.cluster(1)
    with pytest.raises(RuntimeError, match="num_clusters"):
        ix.nearest_centroid(cent)
    assert _live() == live
    ix.add_gamma(g)
    live = _live()
    big = np.asfortranarray(np.ones((K, MAX_CLUSTERS + 1)))
    for n_clusters, c in ((0, cent), (-1, cent), (N + 1, big), (MAX_CLUSTERS + 1, big)):
        assert cluster(ix._handle, n_clusters, c, 5) == _ffi.ERR_ARG
        assert assign(ix._handle, c, n_clusters, None, 0) == _ffi.ERR_ARG
        assert assign(ix._handle, c, n_clusters, g, N) == _ffi.ERR_ARG
        with pytest.raises(RuntimeError, match="num_clusters"):
            ix.cluster(n_clusters, init=None)
        assert _live() == live
    with pytest.raises(RuntimeError, match="num_clusters"):
        ix.nearest_centroid(big[:, :N + 1])
    with pytest.raises(TypeError):
        ix.cluster(2.5)
    # max_iter, NULL arguments, a gamma without documents
    assert cluster(ix._handle, 3, cent, -1) == _ffi.ERR_ARG
    with pytest.raises(ValueError, match="max_iter"):
        ix.cluster(3, max_iter=-1)
    assert cluster(None, 3, cent, 5) == _ffi.ERR_ARG and cluster(ix._handle, 3, None, 5) == _ffi.ERR_ARG
    assert cluster(ix._handle, 3, cent, 5, labels_out=None) == _ffi.ERR_ARG
    assert cluster(ix._handle, 3, cent, 5, its_out=None) == _ffi.ERR_ARG
    assert cluster(ix._handle, 3, cent, 5, conv_out=None) == _ffi.ERR_ARG
    assert assign(None, cent, 3, None, 0) == _ffi.ERR_ARG and assign(ix._handle, None, 3, None, 0) == _ffi.ERR_ARG
    assert assign(ix._handle, cent, 3, None, 0, labels_out=None) == _ffi.ERR_ARG
    assert assign(ix._handle, cent, 3, g, 0) == _ffi.ERR_ARG and assign(ix._handle, cent, 3, g, -1) == _ffi.ERR_ARG
    assert _live() == live
    # a centroid array of the wrong K
    for call in (lambda: ix.cluster(3, init=np.ones((K + 1, 3))), lambda: ix.nearest_centroid(np.ones((K + 1, 3))),
                 lambda: ix.nearest_centroid(cent, gamma=np.ones((K - 1, 2))),
                 lambda: ix.cluster(3, init=np.ones((K, 2)))):
        with pytest.raises(RuntimeError):
            call()
        assert _live() == live
    # values that are not finite and positive
    for bad in (0.0, -1.0, np.nan, np.inf):
        c = cent.copy(order="F")
        c[K - 1, 2] = bad
        gb = g.copy(order="F")
        gb[0, N - 1] = bad
        assert cluster(ix._handle, 3, c, 5) == _ffi.ERR_VALUE and assign(ix._handle, c, 3, None, 0) == _ffi.ERR_VALUE
        assert assign(ix._handle, cent, 3, gb, N) == _ffi.ERR_VALUE
        assert c[K - 1, 2] == bad or (bad != bad and c[K - 1, 2] != c[K - 1, 2])
        for call in (lambda: ix.cluster(3, init=c), lambda: ix.nearest_centroid(c),
                     lambda: ix.nearest_centroid(cent, gamma=gb)):
            with pytest.raises(_ffi.TrldaError) as caught:
                call()
            assert caught.value.code == _ffi.ERR_VALUE
        assert _live() == live
    # ids that are not distinct ids of indexed documents: refused in Python
    for ids in ([0, 0, 1], [0, 1, N], [-1, 0, 1]):
        with pytest.raises(ValueError, match="distinct"):
            ix.cluster(3, init=ids)
        assert _live() == live
    # nothing was drawn or written
    assert len(ix) == N and np.array_equal(before, _state()) and _live() == live
    assert np.all(labels == -7) and np.all(sim == -7.) and np.all(sizes == -7) and its.value == conv.value == -7
    # the index still works after the refusals
    got, _ = ix.cluster(3, init=cent)
    assert got.shape == (N,) and set(got) <= {0, 1, 2}
    assert _live() == live
    ix.close()
    live = _live()                                           # (the index's own buffers went with it)
    for call in (lambda: ix.cluster(3, init=cent), lambda: ix.nearest_centroid(cent),
                 lambda: ix.nearest_centroid(cent, gamma=g)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
        assert _live() == live
    m.close()


# 7. planted structure ---------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
def test_planted_groups_are_recovered(hip, measure):
    """240 gammas around 4 well-separated Dirichlet centres at K = 17: each group's weight sits on its
    own four topics."""
    K, groups, per = 17, 4, 60
    rng = np.random.RandomState(123)
    truth = np.repeat(np.arange(groups), per)
    rng.shuffle(truth)
    centre = np.full((groups, K), 0.2)
    for c in range(groups):
        centre[c, 4 * c:4 * c + 4] = 25.0
    g = np.asfortranarray(np.stack([rng.dirichlet(centre[t]) * rng.uniform(5., 50.) + 1e-3 for t in truth], axis=1))
    m = _model(K)
    ix = _filled(m, measure, g)
    init = [int(np.flatnonzero(truth == c)[0]) for c in range(groups)]
    labels, cent, info = ix.cluster(groups, init=init, return_info=True)
    assert info["converged"] and np.array_equal(labels, truth)
    assert np.array_equal(info["sizes"], np.full(groups, per))
    assert np.all(np.argsort(-cent, axis=0)[:4].min(axis=0) == 4 * np.arange(groups))
    ids, _ = ix.query_gamma(cent, top_n=1)
    assert np.array_equal(truth[ids[:, 0]], np.arange(groups))
    # the centroids index like any gamma
    other = m.document_index(measure)
    assert other.add_gamma(cent) == 0 and len(other) == groups
    m.close()
