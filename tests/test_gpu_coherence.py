"""LDA.top_words and LDA.topic_coherence on the GPU (csrc/coherence_kernels.h): the top words
against np.lexsort, planted ties included; the counts bitwise against the restatement
(tests/coherence_host.py) across bit-row word and document-block boundaries; coherence within
1e-12; streams of batches; the model's state left alone; every model; the error paths."""
import ctypes

import numpy as np
import pytest

import coherence_host as ch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipdev():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return 0


def _model(K, V, lam=None, seed=1, cls=None):
    from trlda_amd.models import OnlineLDA
    if cls is None:
        m = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    else:
        m = cls(num_words=V, num_topics=K, alpha=.1, eta=.3, device=0)
    if lam is None:
        lam = np.random.RandomState(seed).gamma(2.0, 1.0, size=(K, V)) + 0.05
    m.lambdas = lam
    return m


def _csr(B, V, rng, mean=20, odd=False):
    """B documents; with odd=True also repeated ids, zero and negative counts and empty documents."""
    from trlda_amd.documents import CSRDocuments
    n = rng.poisson(mean, size=B)
    if odd:
        n[rng.rand(B) < 0.1] = 0
    indptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    ids = rng.randint(0, V, size=indptr[-1])
    cnts = rng.randint(1, 4, size=indptr[-1])
    if odd:
        cnts[rng.rand(len(cnts)) < 0.15] = 0
        cnts[rng.rand(len(cnts)) < 0.1] = -1
        rep = rng.rand(len(ids)) < 0.2                  # repeat the entry before (same document or not)
        rep[0] = False
        ids[rep] = ids[np.flatnonzero(rep) - 1]
    return CSRDocuments(indptr, ids, cnts)


def _want(csr, V, words):
    P = ch.presence(csr.indptr, csr.ids, csr.cnts, V)
    return ch.counts(P, words)


def _lists(rng, T, N, V):
    return np.stack([rng.permutation(V)[:N] for _ in range(T)]).astype(np.int32)


# -- top words --------------------------------------------------------------------------------------
CASES = [(K, V, n) for n in (1, 10, 100) for K, V in ((1, n), (7, n), (100, n), (100, 7000), (7, 100000),
                                                       (1, 7000))]
CASES += [(500, 100000, 10), (500, 100000, 100), (500, 7000, 1)]


@pytest.mark.parametrize("K,V,n", CASES)
def test_top_words_match_lexsort(hipdev, K, V, n):
    rng = np.random.RandomState(K * 7 + n)
    lam = rng.gamma(0.3, 1.0, size=(K, V)) + 1e-3
    m = _model(K, V, lam=lam)
    got = m.top_words(n)
    m.close()
    assert got.dtype == np.int32 and got.shape == (K, n)
    assert np.array_equal(got, ch.top_words(lam, n))


@pytest.mark.parametrize("V", [100, 1500, 3000, 9000])
def test_top_words_planted_ties(hipdev, V):
    K = 12
    rng = np.random.RandomState(V)
    lam = rng.randint(0, 4, size=(K, V)).astype(np.float64) + 1.0   # four values: ties everywhere
    lam[1] = 2.5                                                     # a constant row
    lam[2, :] = 1.0
    lam[2, 1000:1050] = 7.0                                          # a tie across the tile boundary
    lam[2, 1020:1030] = 8.0                                          # (tiles of 1024 words)
    lam[6, :] = 1.0
    lam[6, np.arange(V) % 1024 >= 1019] = 5.0                        # tile ends, every tile
    lam[6, np.arange(V) % 1024 <= 3] = 5.0                           # tile starts
    lam[3, ::2] = 0.0
    lam[3, 1::2] = -0.0                                              # -0 ties with +0
    lam[4] = -rng.randint(0, 3, size=V)                              # negative values
    lam[5, -1] = 9.0                                                 # the best in the last word
    m = _model(K, V, lam=lam)
    for n in (1, 10, 37, 100):
        if n > V:
            continue
        assert np.array_equal(m.top_words(n), ch.top_words(lam, n)), n
    m.close()


# -- counts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 64, 65, 200, 12500])
@pytest.mark.parametrize("odd", [False, True])
def test_counts_are_bitwise_those_of_the_restatement(hipdev, B, odd):
    V, T, N = 500, 30, 10
    rng = np.random.RandomState(B + 17 * odd)
    csr = _csr(B, V, rng, odd=odd)
    words = _lists(rng, T, N, V)
    words[1] = words[0][::-1]                        # shared words: fewer slots than T N
    m = _model(20, V)
    for measure in ("umass", "npmi"):
        coh, cnt = m.topic_coherence(csr, measure=measure, words=words, return_counts=True)
        df, co, M = _want(csr, V, words)
        assert cnt["num_documents"] == M == B
        assert cnt["doc_freq"].dtype == np.int64 and cnt["co_doc_freq"].dtype == np.int64
        assert np.array_equal(cnt["words"], words)
        assert np.array_equal(cnt["doc_freq"], df)
        assert np.array_equal(cnt["co_doc_freq"], co)
        want = ch.coherence(measure, df, co, M)
        assert np.array_equal(np.isnan(coh), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.allclose(coh[ok], want[ok], rtol=1e-12, atol=0)
    m.close()


def test_counts_over_several_document_blocks(hipdev):
    """70 000 documents: more than one block of bit rows (65 536 documents at most)."""
    V, T, N = 1000, 40, 20
    rng = np.random.RandomState(8)
    csr = _csr(70000, V, rng, mean=6, odd=True)
    words = _lists(rng, T, N, V)
    m = _model(10, V)
    _, cnt = m.topic_coherence(csr, words=words, return_counts=True)
    m.close()
    df, co, M = _want(csr, V, words)
    assert cnt["num_documents"] == M
    assert np.array_equal(cnt["doc_freq"], df) and np.array_equal(cnt["co_doc_freq"], co)


def test_top_words_coherence_uses_the_models_top_words(hipdev):
    V, K = 400, 15
    rng = np.random.RandomState(2)
    csr = _csr(300, V, rng)
    m = _model(K, V)
    for measure in ("UMass", "NPMI"):
        coh, cnt = m.topic_coherence(csr, top_n=8, measure=measure, return_counts=True)
        words = ch.top_words(np.asarray(m.lambdas), 8)
        assert np.array_equal(cnt["words"], words) and coh.shape == (K,)
        df, co, M = _want(csr, V, words)
        assert np.allclose(coh, ch.coherence(measure.lower(), df, co, M), rtol=1e-12, atol=0)
    m.close()


def test_a_stream_of_batches_counts_like_one_batch(hipdev, tmp_path):
    from trlda_amd.documents import CSRDocuments, as_csr
    from trlda_amd.utils import load_documents
    V, K = 300, 12
    rng = np.random.RandomState(5)
    parts = [_csr(B, V, rng, odd=True) for B in (70, 1, 130, 64)]
    whole = CSRDocuments(np.concatenate([[0]] + [p.indptr[1:] + sum(q.indptr[-1] for q in parts[:i])
                                                 for i, p in enumerate(parts)]),
                         np.concatenate([p.ids for p in parts]), np.concatenate([p.cnts for p in parts]))
    m = _model(K, V)
    one = m.topic_coherence(whole, top_n=10, return_counts=True)
    many = m.topic_coherence(iter(parts), top_n=10, return_counts=True)
    uploaded = [m.upload(p) for p in parts]
    dev = m.topic_coherence(iter(uploaded), top_n=10, return_counts=True)
    for b in uploaded:
        b.close()
    for got in (many, dev):
        assert np.array_equal(got[0], one[0], equal_nan=True)
        for key in ("words", "doc_freq", "co_doc_freq"):
            assert np.array_equal(got[1][key], one[1][key]), key
        assert got[1]["num_documents"] == one[1]["num_documents"] == len(whole)
    # a load_documents generator over a file (positive counts: the text format's)
    pos = _csr(333, V, rng)
    c = as_csr(pos)
    lines = []
    for d in range(len(c)):
        a, b = c.indptr[d], c.indptr[d + 1]
        lines.append("%d %s" % (b - a, " ".join("%d:%d" % (w, k) for w, k in zip(c.ids[a:b], c.cnts[a:b]))))
    path = tmp_path / "corpus.dat"
    path.write_text("\n".join(lines) + "\n")
    streamed = m.topic_coherence(load_documents(str(path), 50), top_n=10, measure="npmi", return_counts=True)
    single = m.topic_coherence(pos, top_n=10, measure="npmi", return_counts=True)
    m.close()
    assert np.array_equal(streamed[0], single[0])
    assert np.array_equal(streamed[1]["co_doc_freq"], single[1]["co_doc_freq"])
    assert streamed[1]["num_documents"] == 333


def test_planted_topics_score_higher_than_random(hipdev):
    import trlda_amd
    K, V = 8, 800
    lam = np.full((K, V), 0.01)
    for k in range(K):
        lam[k, k * 100:(k + 1) * 100] = np.linspace(50.0, 5.0, 100)   # disjoint topics
    trlda_amd.seed(3)
    planted = _model(K, V, lam=lam)
    planted.alpha = 0.05
    docs = planted.sample(2000, 60)
    rand = _model(K, V, seed=4)
    for measure in ("umass", "npmi"):
        good = planted.topic_coherence(docs, top_n=10, measure=measure)
        bad = rand.topic_coherence(docs, top_n=10, measure=measure)
        assert np.nanmean(good) > np.nanmean(bad) + 0.1, (measure, good, bad)
        # the same lists scored through words= give the same values
        assert np.array_equal(rand.topic_coherence(docs, measure=measure, words=planted.top_words(10)), good,
                              equal_nan=True)
    planted.close()
    rand.close()


def test_state_and_stream_are_left_alone(hipdev):
    import trlda_amd
    from trlda_amd import _ffi
    V, K = 500, 20
    rng = np.random.RandomState(6)
    csr = _csr(100, V, rng)
    m = _model(K, V)
    lam, alpha, eta, count = np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count
    key = ctypes.c_uint64()
    trlda_amd.seed(77)
    _ffi.lib().trlda_rng_draw_key(ctypes.byref(key))
    want_key = key.value
    trlda_amd.seed(77)
    m.top_words(10)
    m.topic_coherence(csr, top_n=10, measure="npmi")
    m.topic_coherence(iter([csr, csr]), words=_lists(rng, 3, 5, V))
    _ffi.lib().trlda_rng_draw_key(ctypes.byref(key))
    assert key.value == want_key
    assert np.array_equal(np.asarray(m.lambdas), lam)
    assert np.array_equal(np.asarray(m.alpha), alpha) and m.eta == eta and m.update_count == count
    m.close()


def test_after_updates_with_deferred_statistics_and_lanes(hipdev):
    import torch
    import trlda_amd
    from trlda_amd.stream import EStepStream
    K, V, B = 64, 3000, 120
    rng = np.random.RandomState(12)
    csrs = [_csr(B, V, rng, mean=50) for _ in range(5)]
    trlda_amd.seed(5)
    m = _model(K, V)
    m.update_parameters(csrs[0], max_iter_tr=3, max_iter_inference=20)
    dev = torch.device("cuda", 0)
    batches = [m.upload(c) for c in csrs]
    g0 = [torch.from_numpy(np.random.RandomState(50 + i).gamma(100., 1. / 100., size=(B, K))).to(dev)
          for i in range(5)]
    gam = [torch.empty(B, K, dtype=torch.float64, device=dev) for _ in csrs]
    sst = [torch.empty(V, K, dtype=torch.float64, device=dev) for _ in csrs]
    with EStepStream(m, lanes=2, deferred=True) as s:
        for i, b in enumerate(batches):
            s.step(b, batches[i + 1:i + 3], g0[i], gam[i], sst[i], max_iter=20)
        inside = m.top_words(25)
        coh_in = m.topic_coherence(csrs[1], top_n=25)
    torch.cuda.synchronize()
    lam = np.asarray(m.lambdas).copy()
    alpha, eta, count = np.asarray(m.alpha).copy(), m.eta, m.update_count
    after = m.top_words(25)
    coh_after = m.topic_coherence(csrs[1], top_n=25)
    assert np.array_equal(np.asarray(m.lambdas), lam)
    assert np.array_equal(np.asarray(m.alpha), alpha) and m.eta == eta and m.update_count == count
    for b in batches:
        b.close()
    m.close()
    want = ch.top_words(lam, 25)
    assert np.array_equal(inside, want) and np.array_equal(after, want)
    assert np.array_equal(coh_in, coh_after)


@pytest.mark.parametrize("which", ["OnlineLDA", "BatchLDA", "CumulativeLDA"])
def test_every_model(hipdev, which):
    import trlda.models
    cls = getattr(trlda.models, which)
    V, K = 300, 9
    rng = np.random.RandomState(1)
    csr = _csr(150, V, rng)
    m = _model(K, V, cls=None if which == "OnlineLDA" else cls)
    if which != "OnlineLDA":
        m.update_parameters(csr, max_epochs=2, max_iter_inference=10)
    else:
        m.update_parameters(csr, max_iter_tr=2, max_iter_inference=10)
    lam = np.asarray(m.lambdas)
    words = ch.top_words(lam, 6)
    assert np.array_equal(m.top_words(6), words)
    coh = m.topic_coherence(csr, top_n=6)
    df, co, M = _want(csr, V, words)
    assert np.allclose(coh, ch.umass(df, co), rtol=1e-12, atol=0, equal_nan=True)
    m.close()


def test_errors(hipdev):
    from trlda_amd.models import OnlineLDA
    V, K = 50, 4
    m = _model(K, V)
    csr = _csr(10, V, np.random.RandomState(0))
    for n in (0, -1, 101):
        with pytest.raises(RuntimeError):
            m.top_words(n)
    small = _model(K, 5)
    with pytest.raises(RuntimeError):
        small.top_words(6)
    assert small.top_words(5).shape == (K, 5)
    with pytest.raises(RuntimeError):
        m.topic_coherence(csr, top_n=1)
    for bad in ("cv", "", None, 3):
        with pytest.raises(ValueError):
            m.topic_coherence(csr, measure=bad)
    bad_words = [np.arange(5),                             # one-dimensional
                 np.zeros((2, 0), dtype=np.int32),         # empty
                 np.array([[0, 1, 50]]),                   # out of range
                 np.array([[0, -1, 2]]),
                 np.array([[0, 1, 2], [3, 4, 3]]),         # repeated in a row
                 np.array([[0]]),                          # N < 2
                 np.arange(2 * 101).reshape(2, 101) % V,   # N > 100
                 np.array([[0.5, 1.0]])]                   # not ids
    for w in bad_words:
        with pytest.raises(RuntimeError):
            m.topic_coherence(csr, words=w)
    other = _model(K, V + 1)
    foreign = other.upload(_csr(5, V, np.random.RandomState(1)))
    with pytest.raises(RuntimeError):
        m.topic_coherence(foreign, top_n=3)
    with pytest.raises(RuntimeError):
        m.topic_coherence(iter([csr, foreign]), top_n=3)
    foreign.close()
    other.close()
    small.close()
    # the model is still fine after all that
    assert np.array_equal(m.top_words(3), ch.top_words(np.asarray(m.lambdas), 3))
    m.close()
    assert isinstance(m, OnlineLDA)


def test_c_abi_argument_checks(hipdev):
    from trlda_amd import _ffi
    L = _ffi.lib()
    m = _model(3, 20)
    out = _ffi.vp()
    w = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    assert L.trlda_cooc_create(m._handle, w, 0, 3, ctypes.byref(out)) == _ffi.ERR_ARG
    assert L.trlda_cooc_create(m._handle, w, 2, 1, ctypes.byref(out)) == _ffi.ERR_ARG
    assert L.trlda_cooc_create(m._handle, np.array([[0, 1, 20]], dtype=np.int32), 1, 3,
                               ctypes.byref(out)) == _ffi.ERR_ARG
    assert L.trlda_cooc_create(m._handle, np.array([[0, 1, 0]], dtype=np.int32), 1, 3,
                               ctypes.byref(out)) == _ffi.ERR_ARG
    assert L.trlda_model_top_words(m._handle, 0, np.zeros(3, dtype=np.int32)) == _ffi.ERR_ARG
    assert L.trlda_model_top_words(m._handle, 21, np.zeros(63, dtype=np.int32)) == _ffi.ERR_ARG
    assert L.trlda_cooc_create(m._handle, w, 2, 3, ctypes.byref(out)) == _ffi.OK
    assert L.trlda_cooc_add(out, None) == _ffi.ERR_ARG
    df, co, n = np.empty(6, dtype=np.int64), np.empty(18, dtype=np.int64), ctypes.c_int64(-1)
    assert L.trlda_cooc_read(out, df, co, ctypes.byref(n)) == _ffi.OK
    assert n.value == 0 and not df.any() and not co.any()
    assert L.trlda_cooc_destroy(out) == _ffi.OK
    m.close()
