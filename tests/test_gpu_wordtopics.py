"""LDA.word_topics on the GPU (csrc/wordtopics_kernels.h): the ranked rows against the
restatement (tests/wordtopics_host.py) from the gamma the call returns, the full posterior, the tie
order, independence of the batch, the fixed point of gamma, the model's state, the errors and the
device-pointer form.

Every case scores the same seven documents: an empty one, one entry, one with a c = 0 entry, 63, 64
and 65 entries (a wave takes an entry at a time, four waves per workgroup) and 300 entries, which
is three of the kernel's chunks of 128."""
import ctypes as C

import numpy as np
import pytest

import wordtopics_host as wh

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 20, 63, 64, 65, 300]
B = len(LENGTHS)
ZERO_AT = 1 + 7                                      # the c = 0 entry: the eighth of the third document
# V per K of the parity cases (between 50 and 300; small where the table is tall)
PARITY_V = {3: 300, 64: 200, 65: 150, 100: 300, 513: 120, 2276: 50}
GAP_FLOOR = 1e-6


@pytest.fixture(scope="module")
def hip():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


def _docs(V, seed):
    from trlda_amd.documents import CSRDocuments
    rng = np.random.RandomState(seed)
    indptr = np.concatenate([[0], np.cumsum(LENGTHS)])
    ids = rng.randint(0, V, size=indptr[-1])
    cnts = rng.randint(1, 5, size=indptr[-1])
    cnts[ZERO_AT] = 0
    return CSRDocuments(indptr, ids, cnts)


def _case(K, V, seed=None):
    """(lambda K x V, the seven documents, gamma0 K x B) of a case."""
    seed = K if seed is None else seed
    rng = np.random.RandomState(1000 + seed)
    lam = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    g0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)
    return lam, _docs(V, seed), g0


def _model(K, V, lam, alpha=.1, eta=.3):
    """An OnlineLDA holding `lam` without the constructor's K V 100 draws."""
    from trlda_amd.models import OnlineLDA
    m = OnlineLDA.__new__(OnlineLDA)
    m._num_documents = 1000
    m._update_count = 0
    m._ada_tau = 1000.
    m._ada_rho = 1. / m._ada_tau
    m._ada_sq_norm = 1.
    m._setup(V, K, alpha, eta, None, _lambda=np.asfortranarray(lam))
    return m


def _state():
    from trlda_amd import _ffi
    s = np.zeros(33, dtype=np.uint32)
    _ffi.lib().trlda_rng_get_state(s)
    return s


def _device_form(hip, m, docs, gamma, top_n):
    """trlda_model_word_topics_dev on a gamma the caller uploaded: (topics, probs)."""
    from trlda_amd import _ffi
    gamma = np.asfortranarray(gamma, dtype=np.float64)
    nnz = int(docs.indptr[-1])
    topics = np.full((nnz, top_n), -7, dtype=np.int32)
    probs = np.full((nnz, top_n), np.nan)
    batch = m.upload(docs)
    ptrs = [_ffi.vp() for _ in range(3)]
    sizes = (gamma.nbytes, topics.nbytes, probs.nbytes)
    try:
        for q, nbytes in zip(ptrs, sizes):
            _ffi.check(hip.trlda_dev_alloc(0, max(nbytes, 8), C.byref(q)))
        _ffi.check(hip.trlda_dev_upload(0, ptrs[0], gamma.ctypes.data, gamma.nbytes))
        _ffi.check(hip.trlda_model_word_topics_dev(m._handle, batch.handle, ptrs[0], top_n, ptrs[1], ptrs[2]))
        _ffi.check(hip.trlda_model_synchronize(m._handle))
        if nnz:
            _ffi.check(hip.trlda_dev_download(0, topics.ctypes.data, ptrs[1], topics.nbytes))
            _ffi.check(hip.trlda_dev_download(0, probs.ctypes.data, ptrs[2], probs.nbytes))
    finally:
        for q in ptrs:
            if q.value:
                hip.trlda_dev_free(0, q)
        batch.close()
    return topics, probs


# 1. parity over K -------------------------------------------------------------------------------
@pytest.mark.parametrize("top_n", [1, 3])
@pytest.mark.parametrize("K", sorted(PARITY_V))
def test_parity_with_the_restatement(hip, K, top_n):
    """probs to the project's parity bound (1e-9 relative) and topics exactly, the restatement fed
    the gamma the call returned.  The inputs have no near-ties: the restatement's gap report stays
    above 1e-6 for every entry (checked on the CPU with the oracle's gamma when the seeds were
    chosen; asserted here with the device's)."""
    V = PARITY_V[K]
    lam, docs, g0 = _case(K, V)
    m = _model(K, V, lam)
    indptr, topics, probs, gamma = m.word_topics(docs, top_n=top_n, latents=g0, max_iter=20, return_gamma=True)
    m.close()
    assert indptr.dtype == np.int64 and np.array_equal(indptr, docs.indptr)
    assert topics.dtype == np.int32 and topics.shape == probs.shape == (sum(LENGTHS), top_n)
    _, want_t, want_p, gap = wh.word_topics(docs.indptr, docs.ids, gamma, lam, top_n)
    assert gap.min() > GAP_FLOOR, gap.min()
    err = float(np.max(np.abs(probs - want_p) / want_p))
    print("K = %d top_n = %d: max rel err of probs %.2e, smallest gap %.2e" % (K, top_n, err, gap.min()))
    assert np.array_equal(topics, want_t)
    assert err < 1e-9, err


# 2. the full posterior ----------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 32])
def test_full_posterior(hip, K):
    V = 200
    lam, docs, g0 = _case(K, V, seed=50 + K)
    m = _model(K, V, lam)
    _, topics, probs = m.word_topics(docs, top_n=K, latents=g0, max_iter=20)
    m.close()
    assert np.all(np.abs(probs.sum(axis=1) - 1) <= 4 * K * np.finfo(np.float64).eps)
    assert np.all(np.diff(probs, axis=1) <= 0) and np.all(probs > 0)
    assert np.array_equal(np.sort(topics, axis=1), np.tile(np.arange(K), (len(topics), 1)))


# 3. ties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [6, 600])
def test_equal_probabilities_go_by_smaller_topic_id(hip, K):
    """Two topics with identical lambda rows and identical alpha (and gamma0): wherever two returned
    probabilities of a row are bitwise equal, the smaller id comes first.  On the output alone."""
    V, top_n = 80, min(K, 32)
    lam, docs, g0 = _case(K, V, seed=70 + K)
    lam[4] = lam[1]
    g0[4] = g0[1]
    m = _model(K, V, lam)
    _, topics, probs = m.word_topics(docs, top_n=top_n, latents=g0, max_iter=20)
    m.close()
    same = probs[:, :-1] == probs[:, 1:]
    assert np.all(topics[:, :-1][same] < topics[:, 1:][same])
    if K == 6:                                       # (every topic is returned: the pair is in every row)
        at1 = np.argmax(topics == 1, axis=1)
        assert same[np.arange(len(topics)), at1].all() and np.all(topics[np.arange(len(topics)), at1 + 1] == 4)


# 4. independence of the batch ------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch(hip):
    """Each document scored alone, its column of gamma0 as latents, gives bitwise its rows of the
    batch call (the 300-entry document: three workgroups in either).  K = 513: the E-step runs the
    general kernel, a workgroup per document whatever the batch, so gamma itself is a function of
    the document; at K <= 128 the E-step picks its kernels per batch (split documents, the fused
    preamble), which agree to a few ulp only -- there the scoring stage is checked on its own, from a
    given gamma, in test_device_pointer_form."""
    K, V, top_n = 513, 120, 3
    lam, docs, g0 = _case(K, V)
    m = _model(K, V, lam)
    indptr, topics, probs, gamma = m.word_topics(docs, top_n=top_n, latents=g0, max_iter=20, return_gamma=True)
    for d in range(B):
        ip, t, p, g = m.word_topics(docs.slice(d, d + 1), top_n=top_n, latents=g0[:, d], max_iter=20,
                                    return_gamma=True)
        assert np.array_equal(ip, [0, LENGTHS[d]])
        assert np.array_equal(g[:, 0], gamma[:, d])
        assert np.array_equal(t, topics[indptr[d]:indptr[d + 1]])
        assert np.array_equal(p, probs[indptr[d]:indptr[d + 1]])
    m.close()


# 5. the fixed point --------------------------------------------------------------------------------
def test_rows_reproduce_gamma_at_the_fixed_point(hip):
    """gamma_dk = alpha_k + sum_p c_p phi_pk at convergence (src/lda.cpp:189-197).  K = 10, V = 200,
    threshold 1e-10: the oracle's E-step converges on these documents in 2 .. 1111 iterations (the
    cap is 5000) and its gamma then misses the identity by 7.3e-11 relative at most; the tolerance
    is ten times that."""
    K, V, alpha = 10, 200, .1
    tol = 10 * 7.3e-11
    lam, docs, g0 = _case(K, V)
    m = _model(K, V, lam, alpha=alpha)
    indptr, topics, probs, gamma = m.word_topics(docs, top_n=K, latents=g0, max_iter=5000, threshold=1e-10,
                                                 return_gamma=True)
    m.close()
    phi = np.empty_like(probs)
    np.put_along_axis(phi, topics.astype(np.int64), probs, axis=1)
    doc = np.repeat(np.arange(B), np.diff(indptr))
    want = np.full((K, B), alpha)
    np.add.at(want.T, doc, docs.cnts[:, None] * phi)
    err = float(np.max(np.abs(want - gamma) / gamma))
    print("fixed point: max rel residual %.2e" % err)
    assert err < tol, err
    assert np.array_equal(gamma[:, 0], np.full(K, alpha))        # the empty document


# 6. the model's state ------------------------------------------------------------------------------
def test_state_is_left_alone(hip):
    from trlda_amd import _ffi
    K, V = 32, 200
    lam, docs, g0 = _case(K, V)
    rng = np.random.RandomState(5)
    g1 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)

    def run(between):
        m = _model(K, V, lam, alpha=.2, eta=.05)
        out = [m.do_e_step(docs, latents=g0, max_iter=20)]
        if between:
            before = (np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count)
            m.word_topics(docs, top_n=2, latents=g1, max_iter=20)
            held = np.empty((K, V), order="F")
            _ffi.check(hip.trlda_model_get_sstats(m._handle, held))
            out.append(held)
            assert np.array_equal(np.asarray(m.lambdas), before[0])
            assert np.array_equal(np.asarray(m.alpha), before[1])
            assert m.eta == before[2] and m.update_count == before[3]
        out.append(m.do_e_step(docs, latents=g1, max_iter=20))
        m.close()
        return out

    a, b = run(False), run(True)
    for x, y in ((a[0], b[0]), (a[1], b[2])):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    assert np.array_equal(b[1], a[1][1])             # the statistics of that E-step from the same gamma0


# 7. errors -----------------------------------------------------------------------------------------
def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    from trlda_amd import _ffi
    from trlda_amd.documents import DeviceBatch
    K, V = 8, 100
    lam, docs, g0 = _case(K, V)
    m = _model(K, V, lam)
    wide = _model(40, V, _case(40, V)[0])
    trlda_amd.seed(3)
    before = _state()
    for model, top_n in ((m, 0), (m, K + 1), (wide, 33)):
        with pytest.raises(RuntimeError, match="top_n"):
            model.word_topics(docs, top_n=top_n)
    with pytest.raises(RuntimeError, match="Initial gamma has wrong dimensionality."):
        m.word_topics(docs, latents=np.ones((K, B + 1)))
    other = DeviceBatch(docs, V + 1, 0)
    with pytest.raises(RuntimeError, match="different model"):
        m.word_topics(other)
    # the C checks
    nnz = int(docs.indptr[-1])
    g = np.array(g0, order="F")
    t, p = np.full((nnz, 33), -7, dtype=np.int32), np.full((nnz, 33), -7.)
    mine = m.upload(docs)
    wide_b = wide.upload(docs)
    for model, batch, top_n in ((m, mine, 0), (m, mine, K + 1), (wide, wide_b, 33), (m, other, 1), (m, None, 1)):
        handle = batch.handle if batch is not None else None
        assert hip.trlda_model_word_topics(model._handle, handle, g.ctypes.data, top_n, 20, 1e-3,
                                           t.ctypes.data, p.ctypes.data) == _ffi.ERR_ARG
        assert hip.trlda_model_word_topics_dev(model._handle, handle, None, top_n, None, None) == _ffi.ERR_ARG
    assert np.array_equal(g, g0) and np.all(t == -7) and np.all(p == -7.)
    assert np.array_equal(before, _state())          # nothing was drawn
    # the model still works after the refusals
    _, topics, probs = m.word_topics(mine)
    assert topics.shape == (nnz, 1) and np.all(probs > 0)
    for b in (mine, wide_b, other):
        b.close()
    m.close()
    wide.close()


def test_above_the_vi_bound(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K = _ffi.vi_max_topics() + 1
    m = _model(K, 3, np.ones((K, 3)))
    try:
        trlda_amd.seed(3)
        before = _state()
        with pytest.raises(_ffi.TrldaError, match="TRLDA_VI_MAX_TOPICS"):
            m.word_topics([[(0, 1)]])
        batch = m.upload([[(0, 1)]])
        g, t, p = np.ones((K, 1), order="F"), np.zeros(1, dtype=np.int32), np.zeros(1)
        assert hip.trlda_model_word_topics(m._handle, batch.handle, g.ctypes.data, 1, 10, 1e-3, t.ctypes.data,
                                           p.ctypes.data) == _ffi.ERR_ARG
        assert hip.trlda_model_word_topics_dev(m._handle, batch.handle, None, 1, None, None) == _ffi.ERR_ARG
        batch.close()
        assert np.array_equal(before, _state())
    finally:
        m.close()


def test_empty_inputs(hip):
    K, V = 5, 50
    m = _model(K, V, _case(K, V)[0])
    indptr, topics, probs = m.word_topics([], top_n=2)
    assert np.array_equal(indptr, [0]) and topics.shape == probs.shape == (0, 2)
    indptr, topics, probs, gamma = m.word_topics([[], []], top_n=2, latents=np.ones((K, 2)), return_gamma=True)
    assert np.array_equal(indptr, [0, 0, 0]) and topics.shape == (0, 2)
    assert np.array_equal(gamma, np.full((K, 2), .1))            # alpha: the E-step of an empty document
    m.close()


# 8. the device-pointer form -----------------------------------------------------------------------
@pytest.mark.parametrize("K,V", [(100, 300), (2276, 50)])
def test_device_pointer_form(hip, K, V):
    """From the gamma the host form returned: the same bits (products in registers at K = 100, formed
    again per pass at K = 2276); a document alone, from its column of that gamma, its rows of the
    batch; the model's statistics are not touched (no E-step runs)."""
    from trlda_amd import _ffi
    top_n = 3
    lam, docs, g0 = _case(K, V)
    m = _model(K, V, lam)
    indptr, topics, probs, gamma = m.word_topics(docs, top_n=top_n, latents=g0, max_iter=20, return_gamma=True)
    held = np.empty((K, V), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, held))
    t, p = _device_form(hip, m, docs, gamma, top_n)
    assert np.array_equal(t, topics) and np.array_equal(p, probs)
    for d in (1, 2, 5, 6):
        t1, p1 = _device_form(hip, m, docs.slice(d, d + 1), gamma[:, d:d + 1], top_n)
        assert np.array_equal(t1, topics[indptr[d]:indptr[d + 1]])
        assert np.array_equal(p1, probs[indptr[d]:indptr[d + 1]])
    after = np.empty((K, V), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, after))
    m.close()
    assert np.array_equal(held, after)
