"""DocumentIndex on the GPU (csrc/docindex_kernels.h): the stored rows, the similarities
and ids against the restatement (tests/docindex_host.py) of the device's own rows, exact ties,
independence of the partition, the forms, the model's state and the errors.

Every array is small: at most 300 indexed documents (2100 once, at K = 8, to cross the growth copy)
and 33 queries (150 once, to cross the query tiles of 64 and 128 rows)."""
import ctypes as C

import numpy as np
import pytest

import docindex_host as dh

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GAP_FLOOR = 1e-9                         # three orders above the similarity bound at K = 2276 (5e-13)
MEASURES = ["hellinger", "cosine"]
N_MAX, B_MAX = 300, 33

# rows(): r = sqrt(g / S) on both sides.  The two sums S differ in order only: relatively by d_S, a
# few u (numpy adds pairwise, the device 64 lane sums and six levels; neither comes near its worst
# case of about log2(K) + K / 64 u on positive terms).  The quotient adds u / 2 on each side, the square
# root halves what it is given and adds u / 2 on each side: |r_dev - r_np| / r <= d_S / 2 + 3 u / 2 + second
# order, which is 4 u with d_S <= 5 u.
ROW_BOUND = {"hellinger": 4 * U,
             # r = t / sqrt(T): S cancels (a common factor of t and sqrt(T)) up to the rounding of t, u / 2 each
             # side; T = sum t^2 carries the squares' 3 u / 2 and its own order, d_T of a few u, halved by the
             # root, which adds u / 2, and the last quotient u / 2, each side: u + (3 u + d_T) / 2 + 2 u <= 8 u
             "cosine": 8 * U}


def sim_bound(K):
    """|s_dev - s_longdouble| for rows of the device: each of the K products is rounded once (or
    kept exact inside a fused multiply-add) and each of the K additions once, on a running value that
    never exceeds 1 + K u (Cauchy-Schwarz on unit rows): K u for the chain, and the same again as
    allowance for the products, the longdouble reference's own rounding and the row norms' excess
    over 1 -- (K + 8) u 2."""
    return (K + 8) * U * 2


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


def _case(K):
    """(index gammas K x 300, query gammas K x 33) of a case."""
    return _gammas(K, N_MAX, 4000 + K), _gammas(K, B_MAX, 9000 + K)


def _state():
    from trlda_amd import _ffi
    s = np.zeros(33, dtype=np.uint32)
    _ffi.lib().trlda_rng_get_state(s)
    return s


def _device_rows(m, measure, gamma):
    """The rows the device makes of `gamma` (they depend on the column and K alone)."""
    ix = m.document_index(measure)
    ix.add_gamma(gamma)
    r = ix.rows()
    ix.close()
    return r


def _docs(V, n, seed, length=12):
    from trlda_amd.documents import CSRDocuments
    rng = np.random.RandomState(seed)
    indptr = np.arange(n + 1) * length
    return CSRDocuments(indptr, rng.randint(0, V, size=indptr[-1]), rng.randint(1, 5, size=indptr[-1]))


# 1. rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", [3, 4, 5, 64, 65, 100, 513])
def test_rows(hip, K, measure):
    gi, _ = _case(K)
    m = _model(K)
    whole = m.document_index(measure)
    assert whole.add_gamma(gi) == 0 and len(whole) == N_MAX
    r = whole.rows()
    assert r.shape == (N_MAX, K) and r.dtype == np.float64          # the pad is never returned
    want = dh.rows(gi, measure)
    err = float(np.max(np.abs(r - want) / want))
    print("K = %d %s: max rel err of rows %.2f u" % (K, measure, err / U))
    assert err <= ROW_BOUND[measure], err / U
    assert np.array_equal(whole.rows(1, 2), r[1:3]) and np.array_equal(whole.rows(N_MAX - 1), r[-1:])
    assert whole.rows(5, 0).shape == (0, K)
    # in calls of 7, 1 and 292 documents, and a document alone: the same bits
    parts = m.document_index(measure)
    assert [parts.add_gamma(gi[:, :7]), parts.add_gamma(gi[:, 7]), parts.add_gamma(gi[:, 8:])] == [0, 7, 8]
    assert len(parts) == N_MAX and np.array_equal(parts.rows(), r)
    alone = m.document_index(measure)
    alone.add_gamma(gi[:, 5:6])
    assert np.array_equal(alone.rows(), r[5:6])
    m.close()                                                        # (closes its indexes first)
    with pytest.raises(RuntimeError, match="closed"):
        len(whole)


def test_growth_keeps_the_rows(hip):
    """300 then 1800 documents at K = 8: the table starts at 1024 rows and is copied into 4096."""
    K = 8
    g = _gammas(K, 2100, 11)
    m = _model(K)
    ix = m.document_index()
    ix.add_gamma(g[:, :300])
    early = ix.rows()
    assert ix.add_gamma(g[:, 300:]) == 300 and len(ix) == 2100
    assert np.array_equal(ix.rows(0, 300), early)
    roomy = m.document_index()
    roomy.reserve(2100)
    roomy.add_gamma(g)
    assert np.array_equal(roomy.rows(), ix.rows())
    ids_a, s_a = ix.query_gamma(g[:, 2090:], top_n=5, return_similarity=True)
    ids_b, s_b = roomy.query_gamma(g[:, 2090:], top_n=5, return_similarity=True)
    assert np.array_equal(ids_a, ids_b) and np.array_equal(s_a, s_b)
    assert np.array_equal(ids_a[:, 0], np.arange(2090, 2100))
    m.close()


# 2. similarities and ids -------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", [3, 5, 64, 65, 100, 513])
def test_similarities_and_ids(hip, K, measure):
    """Every N in 1, 15, 16, 17, 300, B in 1, 16, 17, 33 and top_n in 1, 3, min(N, 100).  The inputs
    have no near ties: the restatement's smallest gap among the first top_n + 1 stays above
    GAP_FLOOR for every query of every case (checked on the CPU when the seeds were chosen, asserted
    here first, on the device's rows), so no row is left out of the id comparison."""
    gi, gq = _case(K)
    m = _model(K)
    qrows = _device_rows(m, measure, gq)
    worst, least = 0.0, np.inf
    for N in (1, 15, 16, 17, 300):
        ix = m.document_index(measure)
        ix.add_gamma(gi[:, :N])
        irows = ix.rows()
        for B in (1, 16, 17, 33):
            for top_n in sorted({1, min(3, N), min(N, 100)}):
                want_ids, want_s, gap = dh.search(qrows[:B], irows, top_n)
                assert gap.min() > GAP_FLOOR, (N, B, top_n, gap.min())
                ids, s = ix.query_gamma(gq[:, :B], top_n=top_n, return_similarity=True)
                assert ids.dtype == np.int64 and s.dtype == np.float64 and ids.shape == s.shape == (B, top_n)
                assert np.array_equal(ids, want_ids), (N, B, top_n)
                err = float(np.max(np.abs(s.astype(np.longdouble) - want_s)))
                worst, least = max(worst, err), min(least, float(gap.min()))
                assert err <= sim_bound(K), (N, B, top_n, err)
                ids2, dist = ix.query_gamma(gq[:, :B], top_n=top_n)
                assert np.array_equal(ids2, ids) and np.array_equal(dist, dh.distance(s, measure))
                assert np.all(dist >= 0)
        ix.close()
    print("K = %d %s: max |s - longdouble| %.2e (bound %.2e), smallest gap %.2e"
          % (K, measure, worst, sim_bound(K), least))
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_many_topics_through_the_estep(hip, measure):
    """K = 2276, N = 40, B = 5 through add and query (the E-step forms)."""
    K, V, N, B = 2276, 50, 40, 5
    rng = np.random.RandomState(2276)
    lam = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    m = _model(K, V, lam)
    docs, queries = _docs(V, N, 1), _docs(V, B, 2)
    g0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, N)) + 0.1)
    q0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)
    ix = m.document_index(measure)
    first, gamma = ix.add(docs, latents=g0, max_iter=5, return_gamma=True)
    assert first == 0 and len(ix) == N and gamma.shape == (K, N)
    irows = ix.rows()
    for top_n in (1, 3, N):
        ids, s, gq = ix.query(queries, top_n=top_n, latents=q0, max_iter=5, return_gamma=True,
                              return_similarity=True)
        want_ids, want_s, gap = dh.search(_device_rows(m, measure, gq), irows, top_n)
        assert gap.min() > GAP_FLOOR, gap.min()
        err = float(np.max(np.abs(s.astype(np.longdouble) - want_s)))
        print("K = %d %s top_n = %d: max |s - longdouble| %.2e (bound %.2e), smallest gap %.2e"
              % (K, measure, top_n, err, sim_bound(K), gap.min()))
        assert np.array_equal(ids, want_ids)
        assert err <= sim_bound(K), err
    m.close()


# 3. exact ties ------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
def test_exact_ties_rank_by_id(hip, measure):
    """The same gamma column at ids 3, 40 and 299, slabs of 64 rows: three slabs, three tiles."""
    K = 20
    gi, gq = _case(K)
    gi = gi.copy(order="F")
    gi[:, 40] = gi[:, 3]
    gi[:, 299] = gi[:, 3]
    m = _model(K)
    ix = m.document_index(measure)
    ix.add_gamma(gi)
    ix.set_slab_rows(64)
    ids, s = ix.query_gamma(gi[:, [3, 40, 299, 7]], top_n=5, return_similarity=True)
    for q in range(3):
        assert list(ids[q, :3]) == [3, 40, 299]
        assert s[q, 0] == s[q, 1] == s[q, 2] and s[q, 3] < s[q, 2]
    # every indexed document by its own gamma: itself first, or its smallest duplicate
    for at in range(0, N_MAX, 30):
        cols = np.arange(at, at + 30)
        ids, s = ix.query_gamma(gi[:, cols], top_n=1, return_similarity=True)
        want = np.where(np.isin(cols, (40, 299)), 3, cols)
        assert np.array_equal(ids[:, 0], want)
        assert np.all(s >= 1 - sim_bound(K))
        _, dist = ix.query_gamma(gi[:, cols], top_n=1)
        assert np.all(dist >= 0) and np.all(dist <= np.sqrt(sim_bound(K)))
    m.close()


# 4. partition independence ------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
def test_partition_independence(hip, measure):
    """Bitwise: slabs of 16, 64 and the default at N = 300 and top_n = 100 (more than a slab of 64
    holds); the queries one at a time and all 33 together; top_n = 3 and the first three of 100
    (workgroups of 128 and of 64 query rows); 150 queries, which is more than one query tile."""
    K = 37
    gi, gq = _case(K)
    m = _model(K)
    ix = m.document_index(measure)
    ix.add_gamma(gi)
    ids, s = ix.query_gamma(gq, top_n=100, return_similarity=True)
    for rows in (16, 64, 0):
        ix.set_slab_rows(rows)
        for top_n in (100, 3):
            ids_r, s_r = ix.query_gamma(gq, top_n=top_n, return_similarity=True)
            assert np.array_equal(ids_r, ids[:, :top_n]) and np.array_equal(s_r, s[:, :top_n]), (rows, top_n)
    ix.set_slab_rows(64)
    for q in range(B_MAX):
        ids_1, s_1 = ix.query_gamma(gq[:, q], top_n=100, return_similarity=True)
        assert np.array_equal(ids_1[0], ids[q]) and np.array_equal(s_1[0], s[q]), q
    many = _gammas(K, 150, 5)
    for top_n in (3, 100):
        ids_m, s_m = ix.query_gamma(many, top_n=top_n, return_similarity=True)
        for at in (0, 50, 100):
            ids_c, s_c = ix.query_gamma(many[:, at:at + 50], top_n=top_n, return_similarity=True)
            assert np.array_equal(ids_c, ids_m[at:at + 50]) and np.array_equal(s_c, s_m[at:at + 50])
        want_ids, _, gap = dh.search(_device_rows(m, measure, many), ix.rows(), top_n)
        assert gap.min() > GAP_FLOOR, gap.min()
        assert np.array_equal(ids_m, want_ids)
    m.close()


# 5. forms ------------------------------------------------------------------------------------------
def test_forms_agree(hip):
    """query / query_gamma, add / add_gamma, add_gamma_dev / add_gamma: the same bits."""
    from trlda_amd import _ffi
    K, V, N, B = 24, 60, 50, 9
    rng = np.random.RandomState(8)
    lam = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    m = _model(K, V, lam)
    docs, queries = _docs(V, N, 3), _docs(V, B, 4)
    g0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, N)) + 0.1)
    q0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)
    a = m.document_index()
    first, gamma = a.add(docs, latents=g0, max_iter=20, return_gamma=True)
    want_gamma, _ = m.update_variables(docs, latents=g0, max_iter=20)
    assert np.array_equal(gamma, want_gamma)
    b = m.document_index()
    b.add_gamma(gamma)
    assert np.array_equal(a.rows(), b.rows())
    # the device-pointer form
    c = m.document_index()
    ptr = _ffi.vp()
    _ffi.check(hip.trlda_dev_alloc(0, gamma.nbytes, C.byref(ptr)))
    try:
        _ffi.check(hip.trlda_dev_upload(0, ptr, gamma.ctypes.data, gamma.nbytes))
        assert c.add_gamma_device(ptr, N) == 0
        _ffi.check(hip.trlda_model_synchronize(m._handle))
    finally:
        hip.trlda_dev_free(0, ptr)
    assert len(c) == N and np.array_equal(c.rows(), a.rows())
    ids, dist, gq = a.query(queries, top_n=7, latents=q0, max_iter=20, return_gamma=True)
    ids_g, dist_g = b.query_gamma(gq, top_n=7)
    assert np.array_equal(ids, ids_g) and np.array_equal(dist, dist_g)
    ids_s, sim = a.query(queries, top_n=7, latents=q0, max_iter=20, return_similarity=True)
    assert np.array_equal(ids_s, ids) and np.array_equal(dh.distance(sim), dist)
    # B = 0
    ids_0, dist_0 = a.query([], top_n=2)
    assert ids_0.shape == dist_0.shape == (0, 2) and ids_0.dtype == np.int64
    ids_0, dist_0 = a.query_gamma(np.empty((K, 0)), top_n=2)
    assert ids_0.shape == dist_0.shape == (0, 2)
    assert a.add([]) == N and a.add_gamma(np.empty((K, 0))) == N and len(a) == N
    m.close()


# 6. the model's state ------------------------------------------------------------------------------
def test_state_is_left_alone(hip):
    import trlda_amd
    K, V, N, B = 16, 80, 30, 6
    rng = np.random.RandomState(21)
    lam = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    docs, queries = _docs(V, N, 5), _docs(V, B, 6)
    g0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, N)) + 0.1)
    g1 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)

    def run(between):
        m = _model(K, V, lam, alpha=.2, eta=.05)
        out = [m.do_e_step(docs, latents=g0, max_iter=20)]
        if between:
            before = (np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count)
            ix = m.document_index()
            # the gamma forms draw nothing
            trlda_amd.seed(9)
            state = _state()
            ix.add_gamma(g0)
            ix.query_gamma(g1, top_n=4)
            ix.rows()
            assert np.array_equal(state, _state())
            # the E-step forms with latents=None draw the K B values of update_variables
            ix.add(docs)
            after_add = _state()
            ix.query(queries, top_n=4)
            after_query = _state()
            trlda_amd.seed(9)
            m.update_variables(docs)
            assert np.array_equal(after_add, _state())
            m.update_variables(queries)
            assert np.array_equal(after_query, _state())
            # ... and with latents nothing
            ix.query(queries, top_n=4, latents=g1)
            assert np.array_equal(after_query, _state())
            assert np.array_equal(np.asarray(m.lambdas), before[0])
            assert np.array_equal(np.asarray(m.alpha), before[1])
            assert m.eta == before[2] and m.update_count == before[3]
        out.append(m.do_e_step(queries, latents=g1, max_iter=20))
        m.close()
        return out

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


# 7. errors -----------------------------------------------------------------------------------------
def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    from trlda_amd import _ffi
    from trlda_amd.documents import DeviceBatch
    K, V, N, B = 8, 40, 12, 4
    m = _model(K, V)
    docs = _docs(V, B, 7)
    gi, gq = _gammas(K, N, 1), _gammas(K, B, 2)
    ix = m.document_index("COSINE")
    assert ix.measure == "cosine"
    trlda_amd.seed(3)
    before = _state()
    ids = np.full((B, 101), -7, dtype=np.int64)
    sim = np.full((B, 101), -7.)
    g = np.array(gq, order="F")
    mine = m.upload(docs)
    other = DeviceBatch(docs, V + 1, 0)

    def refused(top_n, batch=mine):
        handle = batch.handle if batch is not None else None
        assert hip.trlda_docindex_query(ix._handle, handle, g.ctypes.data, 20, 1e-3, top_n, ids.ctypes.data,
                                        sim.ctypes.data) == _ffi.ERR_ARG
        if batch is mine:
            assert hip.trlda_docindex_query_gamma(ix._handle, g.ctypes.data, B, top_n, ids.ctypes.data,
                                                  sim.ctypes.data) == _ffi.ERR_ARG

    # an empty index
    refused(1)
    with pytest.raises(RuntimeError, match="top_n"):
        ix.query(docs, top_n=1)
    with pytest.raises(RuntimeError, match="top_n"):
        ix.query_gamma(gq, top_n=1)
    assert len(ix) == 0
    ix.add_gamma(gi)
    for top_n in (0, -1, N + 1, 101):
        refused(top_n)
        with pytest.raises(RuntimeError, match="top_n"):
            ix.query(docs, top_n=top_n)
        with pytest.raises(RuntimeError, match="top_n"):
            ix.query_gamma(gq, top_n=top_n)
    with pytest.raises(TypeError):
        ix.query_gamma(gq, top_n=2.5)
    # a batch of another V, no batch
    refused(1, other)
    refused(1, None)
    assert hip.trlda_docindex_add(ix._handle, other.handle, g.ctypes.data, 20, 1e-3) == _ffi.ERR_ARG
    assert hip.trlda_docindex_add(ix._handle, None, g.ctypes.data, 20, 1e-3) == _ffi.ERR_ARG
    with pytest.raises(RuntimeError, match="different model"):
        ix.query(other, top_n=1)
    with pytest.raises(RuntimeError, match="different model"):
        ix.add(other)
    # latents and gamma of the wrong shape; gamma that is not finite and positive
    with pytest.raises(RuntimeError, match="Initial gamma has wrong dimensionality."):
        ix.query(docs, top_n=1, latents=np.ones((K, B + 1)))
    with pytest.raises(RuntimeError, match="Initial gamma has wrong dimensionality."):
        ix.add(docs, latents=np.ones((K + 1, B)))
    with pytest.raises(RuntimeError, match="Gamma has wrong dimensionality."):
        ix.add_gamma(np.ones((K + 1, 2)))
    for bad in (0.0, -1.0, np.inf, np.nan):
        spoiled = np.array(gq, order="F")
        spoiled[K - 1, B - 1] = bad
        with pytest.raises(_ffi.TrldaError, match="finite and positive") as info:
            ix.add_gamma(spoiled)
        assert info.value.code == _ffi.ERR_VALUE
        with pytest.raises(_ffi.TrldaError, match="finite and positive"):
            ix.query_gamma(spoiled, top_n=1)
    # rows outside the index, slab rows that are no multiple of 16
    for first, count in ((0, N + 1), (N, 1), (-1, 1)):
        with pytest.raises(_ffi.TrldaError):
            ix.rows(first, count)
    for rows in (-16, 8, 17):
        with pytest.raises(_ffi.TrldaError):
            ix.set_slab_rows(rows)
    with pytest.raises(_ffi.TrldaError):
        m.document_index().reserve(-1)
    assert hip.trlda_docindex_create(m._handle, 2, C.byref(_ffi.vp())) == _ffi.ERR_ARG
    # nothing was added, drawn or written
    assert len(ix) == N and np.array_equal(before, _state())
    assert np.array_equal(g, gq) and np.all(ids == -7) and np.all(sim == -7.)
    # the index still works after the refusals
    got, dist = ix.query(mine, top_n=N)
    assert got.shape == (B, N) and np.array_equal(np.sort(got, axis=1), np.tile(np.arange(N), (B, 1)))
    assert np.all(np.diff(dist, axis=1) >= 0)
    # use after close()
    ix.close()
    ix.close()
    for call in (lambda: len(ix), lambda: ix.add_gamma(gi), lambda: ix.query_gamma(gq, top_n=1),
                 lambda: ix.query(docs, top_n=1), lambda: ix.add(docs), lambda: ix.rows(), lambda: ix.reserve(5)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    for b in (mine, other):
        b.close()
    m.close()
    with pytest.raises(RuntimeError, match="closed"):
        m.document_index()


def test_above_the_vi_bound(hip):
    """The E-step forms refuse K above TRLDA_VI_MAX_TOPICS before they draw; the gamma forms take it."""
    import trlda_amd
    from trlda_amd import _ffi
    K = _ffi.vi_max_topics() + 1
    m = _model(K, 3, np.ones((K, 3)))
    try:
        ix = m.document_index()
        gi = _gammas(K, 5, 3)
        ix.add_gamma(gi)
        trlda_amd.seed(3)
        before = _state()
        with pytest.raises(_ffi.TrldaError, match="TRLDA_VI_MAX_TOPICS"):
            ix.add([[(0, 1)]])
        with pytest.raises(_ffi.TrldaError, match="TRLDA_VI_MAX_TOPICS"):
            ix.query([[(0, 1)]], top_n=1)
        batch = m.upload([[(0, 1)]])
        g, ids, sim = np.ones((K, 1), order="F"), np.zeros(1, dtype=np.int64), np.zeros(1)
        assert hip.trlda_docindex_add(ix._handle, batch.handle, g.ctypes.data, 10, 1e-3) == _ffi.ERR_ARG
        assert hip.trlda_docindex_query(ix._handle, batch.handle, g.ctypes.data, 10, 1e-3, 1, ids.ctypes.data,
                                        sim.ctypes.data) == _ffi.ERR_ARG
        batch.close()
        assert np.array_equal(before, _state()) and len(ix) == 5
        got, s = ix.query_gamma(gi, top_n=2, return_similarity=True)
        want_ids, want_s, gap = dh.search(ix.rows(), ix.rows(), 2)
        assert gap.min() > GAP_FLOOR
        assert np.array_equal(got, want_ids) and np.array_equal(got[:, 0], np.arange(5))
        assert float(np.max(np.abs(s.astype(np.longdouble) - want_s))) <= sim_bound(K)
    finally:
        m.close()
