"""The entry points that run an E-step and then score share one host path (estep_from_host in
csrc/trlda_hip.hip): on one batch, from one gamma0, with one max_iter and one
threshold, the gamma each of them hands back is bitwise the gamma of trlda_model_estep_host, and the
documents went through the same kernel.

The other tests compare an entry point with update_variables on shapes of their own; this one holds
all ten to one E-step on one batch.  K = 5 (the register document body) and K = 130 (the wide body),
7 documents over 40 words: an empty one, a single entry, and one of 150 entries (ids repeat), which
is past what a workgroup keeps in registers."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V, B = 40, 7
LENGTHS = (9, 0, 150, 1, 23, 40, 5)
MAX_ITER, THRESHOLD = 20, 1e-3


@pytest.fixture(scope="module")
def L():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


def _docs(lengths, seed):
    from trlda_amd.documents import CSRDocuments
    rng = np.random.RandomState(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ids = rng.randint(0, V, size=indptr[-1]).astype(np.int32)
    cnts = rng.randint(1, 6, size=indptr[-1]).astype(np.int32)
    return CSRDocuments(indptr, ids, cnts)


def _kernel(L, m):
    name = L.trlda_model_last_doc_kernel(m._handle)
    return name.decode() if isinstance(name, bytes) else name


@pytest.mark.parametrize("K", [5, 130])
def test_every_entry_point_runs_the_estep_of_estep_host(L, K):
    from trlda_amd import _ffi
    from trlda_amd.models import OnlineLDA
    rng = np.random.RandomState(K)
    lam = np.asfortranarray(rng.gamma(100., 1. / 100., size=(K, V)) * np.exp(rng.uniform(-1, 2, size=(K, 1))))
    g0 = np.asfortranarray(rng.gamma(100., 1. / 100., size=(K, B)))
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    m.lambdas = lam
    batch = m.upload(_docs(LENGTHS, 1))
    held = m.upload(_docs((3, 2, 4, 0, 5, 1, 3), 2))
    nnz, nnz_held, top_n = int(sum(LENGTHS)), 18, 3
    handles = []

    def created(create, destroy, *args):
        h = C.c_void_p()
        _ffi.check(create(m._handle, *args, C.byref(h)))
        handles.append((destroy, h))
        return h

    def f64(*shape):
        return np.empty(shape, dtype=np.float64, order="F")

    def i32(n):
        return np.empty(n, dtype=np.int32)

    try:
        want = g0.copy(order="F")
        sstats = f64(K, V)
        _ffi.check(L.trlda_model_estep_host(m._handle, batch.handle, want, sstats, MAX_ITER, THRESHOLD, None))
        want_kernel = _kernel(L, m)
        assert not np.array_equal(want, g0)
        assert np.array_equal(want[:, 1], np.full(K, .1))            # the empty document: alpha

        index = created(L.trlda_docindex_create, L.trlda_docindex_destroy, 0)
        prevalence = created(L.trlda_prevalence_create, L.trlda_prevalence_destroy, 1)
        diag = created(L.trlda_topicdiag_create, L.trlda_topicdiag_destroy, 1, .5, .02)
        bound = C.c_double(np.nan)
        loglik, tokens, ess = f64(B), f64(B), f64(B)
        topics, tprobs = i32(nnz * top_n), f64(nnz * top_n)
        words, wprobs = i32(B * top_n), f64(B * top_n)
        ranks, scores, cand = i32(nnz_held), f64(nnz_held), i32(B)
        ids, sims = np.empty(B, dtype=np.int64), f64(B)
        p = lambda a: a.ctypes.data
        calls = [
            ("lower_bound", lambda g: L.trlda_model_lower_bound(
                m._handle, batch.handle, g, m.eta, 1.0, MAX_ITER, THRESHOLD, C.byref(bound))),
            ("predictive", lambda g: L.trlda_model_predictive(
                m._handle, batch.handle, held.handle, g, MAX_ITER, THRESHOLD, loglik, tokens)),
            ("document_loglik", lambda g: L.trlda_model_document_loglik(
                m._handle, batch.handle, p(g), 0, 8, MAX_ITER, THRESHOLD, loglik, p(ess))),
            ("word_topics", lambda g: L.trlda_model_word_topics(
                m._handle, batch.handle, p(g), top_n, MAX_ITER, THRESHOLD, p(topics), p(tprobs))),
            ("recommend", lambda g: L.trlda_model_recommend(
                m._handle, batch.handle, p(g), top_n, 1, MAX_ITER, THRESHOLD, p(words), p(wprobs))),
            ("heldout_ranks", lambda g: L.trlda_model_heldout_ranks(
                m._handle, batch.handle, held.handle, p(g), 1, MAX_ITER, THRESHOLD, p(ranks), p(scores), p(cand))),
            ("docindex_add", lambda g: L.trlda_docindex_add(index, batch.handle, p(g), MAX_ITER, THRESHOLD)),
            ("docindex_query", lambda g: L.trlda_docindex_query(
                index, batch.handle, p(g), MAX_ITER, THRESHOLD, 1, p(ids), p(sims))),
            ("prevalence_add", lambda g: L.trlda_prevalence_add(prevalence, batch.handle, p(g), MAX_ITER, THRESHOLD)),
            ("topicdiag_add", lambda g: L.trlda_topicdiag_add(diag, batch.handle, p(g), MAX_ITER, THRESHOLD)),
        ]
        for name, call in calls:
            gamma = g0.copy(order="F")
            _ffi.check(call(gamma))
            assert np.array_equal(gamma, want), name
            assert _kernel(L, m) == want_kernel, (name, _kernel(L, m), want_kernel)
        assert L.trlda_docindex_size(index) == B and np.isfinite(bound.value)
    finally:
        for destroy, h in handles:
            destroy(h)
        held.close()
        batch.close()
        m.close()
