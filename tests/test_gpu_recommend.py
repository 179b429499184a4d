"""LDA.recommend / recommend_gamma / recall_at on the GPU (csrc/recommend_kernels.h):
the ranked words and their p(w | d) against the longdouble restatement (tests/recommend_host.py) fed
the gamma the call used, exact ties across slabs, the exclusion and the pad, independence of the
partition, the forms, the model's state, the errors and the buffers.

Every array is small: at most 700 words, 130 documents and 2276 topics (never all three at once)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import recommend_host as rh

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GAP_FLOOR = 1e-9                         # relative; four orders above the score bound at K = 2276 (5e-13)
TOPS = (1, 10, 32, 33, 100)              # 32 and 33: the two sides of the 128 / 64 documents switch


def prob_bound(K, V):
    """|p_dev - p_longdouble| / p: the first-order sum of the rounding errors of rs (V - 1 additions),
    of sum(gamma) (K - 1), of the two divisions and of the K-term chain, every term positive --
    (V + 2 K + 8) u."""
    return (V + 2 * K + 8) * U


@pytest.fixture(scope="module")
def hip():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


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


def _lam(K, V, seed=0):
    return np.random.RandomState(7000 + 13 * K + V + seed).gamma(2.0, 1.0, size=(K, V)) + 0.05


def _gammas(K, n, seed):
    """n gamma columns: sparse-ish topic weights of very different totals."""
    rng = np.random.RandomState(seed)
    g = rng.gamma(0.3, 1.0, size=(K, n)) + 0.01
    return np.asfortranarray(g * rng.uniform(0.5, 40.0, size=n))


def _docs(V, n, seed, length=12):
    """n documents of `length` entries: repeated words and counts of 0 among them; document 0 empty."""
    from trlda_amd.documents import CSRDocuments
    rng = np.random.RandomState(seed)
    lengths = np.full(n, length)
    lengths[0] = 0
    indptr = np.concatenate(([0], np.cumsum(lengths)))
    return CSRDocuments(indptr, rng.randint(0, V, size=indptr[-1]), rng.randint(0, 4, size=indptr[-1]))


def _triple(docs, lo=0, hi=None):
    part = docs if hi is None and lo == 0 else docs.slice(lo, hi)
    return part.indptr, part.ids, part.cnts


def _slab(hip, m, words):
    from trlda_amd import _ffi
    _ffi.check(hip.trlda_model_set_recommend_slab_words(m._handle, words))


def _compare(K, V, top_n, words, probs, gamma, lam, docs, s=None):
    """The input condition first, then ids exactly and p within the bound; the worst relative error."""
    want_w, want_p, gap = rh.recommend(gamma, lam, top_n, docs, s=s)
    assert gap.min() > GAP_FLOOR, (K, V, top_n, gap.min())
    assert words.dtype == np.int32 and probs.dtype == np.float64 and words.shape == probs.shape == want_w.shape
    assert np.array_equal(words, want_w), (K, V, top_n)
    pad = want_w < 0
    assert np.all(probs[pad] == 0.0)
    if pad.all():
        return 0.0
    err = float(np.max(np.abs(probs.astype(np.longdouble) - want_p)[~pad] / want_p[~pad]))
    assert err <= prob_bound(K, V), (K, V, top_n, err / U)
    return err


# 1. scores and ids ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 64, 65, 100, 513, 2276])
def test_scores_and_ids(hip, K):
    """V = 300, every B in 1, 17, 33 and top_n in 1, 10, 32, 33, 100, seen words left out.  The inputs
    have no near ties: the restatement's smallest relative gap among the first top_n + 1 stays above
    GAP_FLOOR for every document of every case (checked on the CPU when the seeds were chosen,
    asserted here first), so no case is left out of the id comparison."""
    V, B_max = 300, 33
    lam, gq, docs = _lam(K, V), _gammas(K, B_max, 9000 + K), _docs(V, B_max, K)
    s = rh.scores(gq, lam)
    m = _model(K, V, lam)
    worst = 0.0
    for B in (1, 17, 33):
        part = docs.slice(0, B)
        for top_n in TOPS:
            words, probs = m.recommend_gamma(gq[:, :B], top_n=top_n, docs=part)
            worst = max(worst, _compare(K, V, top_n, words, probs, gq[:, :B], lam, _triple(part), s[:B]))
    words, probs = m.recommend_gamma(gq, top_n=100)                   # every word is ranked
    worst = max(worst, _compare(K, V, 100, words, probs, gq, lam, None, s))
    print("K = %d: max rel err of p %.2f u (bound %d u)" % (K, worst / U, V + 2 * K + 8))
    m.close()


@pytest.mark.parametrize("K", [5, 100])
@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 300])
def test_vocabulary_sizes(hip, K, V):
    """One word, fewer than a tile of 16, one short of / exactly / one past a group of 64; top_n
    clipped to V; B = 17, and B = 130, which crosses the tile of 128 documents."""
    lam = _lam(K, V)
    m = _model(K, V, lam)
    worst = 0.0
    for B in (17, 130):
        gq, docs = _gammas(K, B, 500 + V), _docs(V, B, V, length=min(3, V))
        s = rh.scores(gq, lam)
        for top_n in sorted({min(t, V) for t in TOPS}):
            for part in (docs, None):
                words, probs = m.recommend_gamma(gq, top_n=top_n, docs=part)
                worst = max(worst, _compare(K, V, top_n, words, probs, gq, lam,
                                            None if part is None else _triple(part), s))
    print("K = %d V = %d: max rel err of p %.2f u (bound %d u)" % (K, V, worst / U, V + 2 * K + 8))
    m.close()


def test_through_the_estep(hip):
    """`recommend` (the E-step form) against the restatement fed the gamma it returned; bitwise the
    gamma form on that gamma; a list against an uploaded batch; the E-step is update_variables'."""
    K, V, B = 24, 300, 33
    lam, docs = _lam(K, V), _docs(V, B, 3)
    g0 = np.asfortranarray(np.random.RandomState(4).gamma(1.0, 1.0, size=(K, B)) + 0.1)
    m = _model(K, V, lam)
    want_gamma, _ = m.update_variables(docs, latents=g0, max_iter=20)
    for top_n in (10, 33):
        for exclude in (True, False):
            words, probs, gamma = m.recommend(docs, top_n=top_n, exclude_seen=exclude, latents=g0, max_iter=20,
                                              return_gamma=True)
            assert np.array_equal(gamma, want_gamma) and gamma.shape == (K, B)
            err = _compare(K, V, top_n, words, probs, gamma, lam, _triple(docs) if exclude else None)
            print("E-step form top_n = %d exclude %d: max rel err %.2f u" % (top_n, exclude, err / U))
            w2, p2 = m.recommend_gamma(gamma, top_n=top_n, docs=docs if exclude else None)
            assert np.array_equal(w2, words) and np.array_equal(p2, probs)
    batch = m.upload(docs)
    a = m.recommend(docs.to_list(), top_n=10, latents=g0, max_iter=20)
    b = m.recommend(batch, top_n=10, latents=g0, max_iter=20)
    c = m.recommend_gamma(want_gamma, top_n=10, docs=batch)
    batch.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert np.array_equal(a[0][0], rh.recommend(want_gamma[:, :1], lam, 10)[0][0])     # the empty document
    m.close()


# 2. exact ties, slabs --------------------------------------------------------------------------------
def test_ties_and_slabs(hip):
    """V = 700, slabs of 64 (eleven, the last of 60 words), 128 (six, the last of 60) and the default
    (one); B = 130.  Words 5, 70 and 650 have the same column of lambda: different slabs, equal
    scores, smaller id first.  The results are the same bits whatever the slab."""
    K, V, B = 37, 700, 130
    lam = _lam(K, V)
    lam[:, 70] = lam[:, 5]
    lam[:, 650] = lam[:, 5]
    gq, docs = _gammas(K, B, 77), _docs(V, B, 8)
    m = _model(K, V, lam)
    ref = {}
    for slab in (64, 128, 0):
        _slab(hip, m, slab)
        for top_n in (10, 33, 100):
            for part in (docs, None):
                got = m.recommend_gamma(gq, top_n=top_n, docs=part)
                key = (top_n, part is None)
                if key in ref:
                    assert np.array_equal(got[0], ref[key][0]) and np.array_equal(got[1], ref[key][1]), (slab, key)
                ref[key] = got
    # the tied words: whoever ranks them has them in id order with equal scores
    words, probs = ref[(100, True)]
    seen_tie = 0
    for d in range(B):
        at = [list(words[d]).index(w) if w in words[d] else -1 for w in (5, 70, 650)]
        if at[0] >= 0 and at[2] >= 0:
            assert at[1] == at[0] + 1 and at[2] == at[0] + 2
            assert probs[d, at[0]] == probs[d, at[1]] == probs[d, at[2]]
            seen_tie += 1
    assert seen_tie > 0
    # against the restatement: the input condition holds for every gap but the planted ties', which
    # are exactly 0 and go by id
    s = rh.scores(gq, lam)
    for (top_n, every), (w, p) in ref.items():
        left_out = None if every else rh.seen(*_triple(docs), V)
        for g in rh.ranked_gaps(s, rh.rank(s, left_out), top_n):
            assert np.all((g == 0) | (g > GAP_FLOOR)), (top_n, every, g.min())
        want_w, want_p, _ = rh.recommend(gq, lam, top_n, None if every else _triple(docs), s=s)
        assert np.array_equal(w, want_w), (top_n, every)
        assert float(np.max(np.abs(p.astype(np.longdouble) - want_p) / want_p)) <= prob_bound(K, V)
    # the gap condition on the same inputs without the planted ties
    plain = _lam(K, V)
    m.lambdas = plain
    for top_n in (10, 100):
        words, probs = m.recommend_gamma(gq, top_n=top_n, docs=docs)
        _compare(K, V, top_n, words, probs, gq, plain, _triple(docs))
    m.close()


# 3. exclusion and pad ------------------------------------------------------------------------------
def test_exclusion_and_pad(hip):
    """V = 6: a seen word is left out, a word listed with c = 0 only is not, a word listed twice counts
    once; a document that has seen all but two words gets three pads at top_n = 5, one that has seen
    all six gets five; exclude_seen=False ranks every word."""
    K, V = 3, 6
    lam = _lam(K, V)
    docs = [[(4, 2)], [(4, 0), (1, 1)], [(4, 1), (3, 5), (4, 3)], [(4, 1), (1, 1), (3, 2), (5, 1)], [],
            [(w, 1) for w in range(6)], [(2, 0), (2, 0)]]
    B = len(docs)
    gq = _gammas(K, B, 1)
    indptr = np.cumsum([0] + [len(d) for d in docs])
    flat = [p for d in docs for p in d]
    triple = (indptr, np.array([p[0] for p in flat]), np.array([p[1] for p in flat]))
    m = _model(K, V, lam)
    words, probs = m.recommend_gamma(gq, top_n=5, docs=docs)
    _compare(K, V, 5, words, probs, gq, lam, triple)
    assert 4 not in words[0] and 4 in words[1] and 1 not in words[1] and np.all(words[6] >= 0)
    assert not {3, 4} & set(words[2]) and list(words[2]).count(-1) == 1
    assert list(words[3][2:]) == [-1, -1, -1] and set(words[3][:2]) == {0, 2} and np.all(probs[3, 2:] == 0.0)
    assert np.all(words[5] == -1) and np.all(probs[5] == 0.0) and np.all(words[4] >= 0)
    g0 = np.asfortranarray(gq)
    w_e, p_e, gamma = m.recommend(docs, top_n=5, latents=g0, max_iter=20, return_gamma=True)
    _compare(K, V, 5, w_e, p_e, gamma, lam, triple)
    assert np.array_equal(gamma[:, 4], np.full(K, .1))               # the empty document: alpha
    w_a, p_a = m.recommend(docs, top_n=6, exclude_seen=False, latents=g0, max_iter=20)
    _compare(K, V, 6, w_a, p_a, gamma, lam, None)
    assert np.array_equal(np.sort(w_a, axis=1), np.tile(np.arange(6), (B, 1)))
    assert np.all(np.abs(p_a.sum(axis=1) - 1.0) <= prob_bound(K, V) + 4 * U)    # p(. | d) is a distribution
    # an empty batch
    for got in (m.recommend([], top_n=4), m.recommend_gamma(np.empty((K, 0)), top_n=4)):
        assert got[0].shape == got[1].shape == (0, 4) and got[0].dtype == np.int32
    m.close()


# 4. partition independence ---------------------------------------------------------------------------
def test_partition_independence(hip):
    """Bitwise: two calls; a document alone against the same document inside a batch of 33; top_n = 32
    (workgroups of 128 documents) against the first 32 of top_n = 33 (of 64) -- the library has no
    switch that forces the narrow kernel at top_n <= 32, the prefix compares the two; 130 documents
    against the same in three calls."""
    K, V, B = 65, 300, 33
    lam, gq, docs = _lam(K, V), _gammas(K, B, 21), _docs(V, B, 22)
    m = _model(K, V, lam)
    _slab(hip, m, 64)
    words, probs = m.recommend_gamma(gq, top_n=33, docs=docs)
    again = m.recommend_gamma(gq, top_n=33, docs=docs)
    assert np.array_equal(again[0], words) and np.array_equal(again[1], probs)
    for top_n in (32, 10, 1):
        w, p = m.recommend_gamma(gq, top_n=top_n, docs=docs)
        assert np.array_equal(w, words[:, :top_n]) and np.array_equal(p, probs[:, :top_n]), top_n
    for d in range(B):
        for top_n in (33, 32):
            w1, p1 = m.recommend_gamma(gq[:, d], top_n=top_n, docs=docs.slice(d, d + 1))
            assert np.array_equal(w1[0], words[d, :top_n]) and np.array_equal(p1[0], probs[d, :top_n]), d
    many, mdocs = _gammas(K, 130, 23), _docs(V, 130, 24)
    for top_n in (10, 100):
        w_m, p_m = m.recommend_gamma(many, top_n=top_n, docs=mdocs)
        for lo, hi in ((0, 50), (50, 129), (129, 130)):
            w_c, p_c = m.recommend_gamma(many[:, lo:hi], top_n=top_n, docs=mdocs.slice(lo, hi))
            assert np.array_equal(w_c, w_m[lo:hi]) and np.array_equal(p_c, p_m[lo:hi])
        _compare(K, V, top_n, w_m, p_m, many, lam, _triple(mdocs))
    m.close()


# 5. the model's state --------------------------------------------------------------------------------
def _draw_state():
    from trlda_amd import _ffi
    k = C.c_uint64(0)
    _ffi.check(_ffi.lib().trlda_rng_draw_key(C.byref(k)))
    return k.value


@pytest.mark.parametrize("deferred", [False, True])
def test_state_is_left_alone(hip, deferred):
    """lambda, alpha, eta and update_count around both forms; the gamma form leaves the seeded stream
    and the model's statistics where they were; a VI update_variables after the calls gives the bits
    it gives without them, also with deferred statistics and two stream lanes on."""
    import trlda_amd
    from trlda_amd import _ffi
    K, V, B = 16, 120, 9
    lam, docs, other = _lam(K, V), _docs(V, B, 5), _docs(V, B, 6)
    rng = np.random.RandomState(21)
    g0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)
    g1 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)

    def run(between):
        m = _model(K, V, lam, alpha=.2, eta=.05)
        if deferred:
            _ffi.check(hip.trlda_model_set_deferred_stats(m._handle, 1))
            _ffi.check(hip.trlda_model_set_stream_lanes(m._handle, 2))
        out = [m.update_variables(docs, latents=g0, max_iter=20)]
        if between:
            before = (np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count)
            held = np.empty((K, V), order="F")
            _ffi.check(hip.trlda_model_get_sstats(m._handle, held))
            trlda_amd.seed(9)
            m.recommend_gamma(g1, top_n=5, docs=other)
            m.recommend_gamma(g1, top_n=40)
            trlda_amd.seed(9)
            want = _draw_state()
            trlda_amd.seed(9)
            m.recommend_gamma(g1, top_n=5, docs=other)
            assert _draw_state() == want                              # nothing was drawn
            after = np.empty((K, V), order="F")
            _ffi.check(hip.trlda_model_get_sstats(m._handle, after))
            assert np.array_equal(held, after)                        # no E-step ran
            assert np.array_equal(held, out[0][1])
            after = np.empty((K, V), order="F")
            # the E-step form with latents=None draws the K B values of update_variables
            trlda_amd.seed(9)
            m.recommend(other, top_n=5)
            drawn = _draw_state()
            trlda_amd.seed(9)
            m.update_variables(other)
            assert _draw_state() == drawn
            m.recommend(other, top_n=5, latents=g1, max_iter=20)
            _ffi.check(hip.trlda_model_get_sstats(m._handle, after))
            out.append(after)
            assert np.array_equal(np.asarray(m.lambdas), before[0])
            assert np.array_equal(np.asarray(m.alpha), before[1])
            assert m.eta == before[2] and m.update_count == before[3]
        out.append(m.update_variables(other, latents=g1, max_iter=20))
        m.close()
        return out

    a, b = run(False), run(True)
    for x, y in ((a[0], b[0]), (a[1], b[2])):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    assert np.array_equal(b[1], a[1][1])             # the statistics of that E-step from the same gamma0


# 6. recall -------------------------------------------------------------------------------------------
def test_recall_at(hip):
    """200 documents of 60 tokens sampled from a known K = 10, V = 500 model (each topic 50 words of
    its own), halves as observed and held-out: hits and relevant equal the restatement's, and the
    recall@20 of that model is above the recall@20 of a model whose lambda is constant, which ranks
    the unseen words by id."""
    import trlda_amd
    from trlda_amd.models import OnlineLDA
    K, V = 10, 500
    rng = np.random.RandomState(0)
    truth = np.full((K, V), 0.01)
    for k in range(K):
        truth[k, k * 50:(k + 1) * 50] = rng.gamma(5.0, 1.0, size=50)
    src = OnlineLDA(num_words=V, num_topics=K, num_documents=1, alpha=.1, eta=.01, device=0)
    src.lambdas = truth * 100.
    trlda_amd.seed(1)
    corpus = src.sample(200, 60)
    obs = [d[:len(d) // 2] for d in corpus]
    out = [d[len(d) // 2:] for d in corpus]
    g0 = np.ones((K, 200))
    recall, hits, relevant = src.recall_at(obs, out, top_n=20, latents=g0, return_documents=True)
    batch = src.upload(obs)
    assert recall == src.recall_at(batch, out, top_n=20, latents=g0)
    batch.close()
    assert hits.dtype == relevant.dtype == np.int64 and hits.shape == relevant.shape == (200,)
    words, _ = src.recommend(obs, top_n=20, latents=g0)
    from trlda_amd.documents import as_csr
    o, h = as_csr(obs), as_csr(out)
    r2, h2, n2 = rh.recall(words, (o.indptr, o.ids, o.cnts), (h.indptr, h.ids, h.cnts), V)
    assert np.array_equal(hits, h2) and np.array_equal(relevant, n2) and abs(recall - r2) <= 1e-14
    src.close()
    flat = _model(K, V, np.full((K, V), 1.0))
    base, hits_b, _ = flat.recall_at(obs, out, top_n=20, latents=g0, return_documents=True)
    w_flat, _ = flat.recommend(obs, top_n=20, latents=g0)
    flat.close()
    unseen = ~rh.seen(o.indptr, o.ids, o.cnts, V)
    for d in (0, 7, 199):                                             # constant lambda: the unseen words by id
        assert np.array_equal(w_flat[d], np.flatnonzero(unseen[d])[:20])
    print("recall@20: the sampling model %.4f, a constant lambda %.4f" % (recall, base))
    assert recall > base


# 7. errors -------------------------------------------------------------------------------------------
def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    from trlda_amd import _ffi
    from trlda_amd.documents import DeviceBatch
    K, V, B = 8, 40, 4
    lam, docs = _lam(K, V), _docs(V, B, 7)
    m = _model(K, V, lam)
    gq = _gammas(K, B, 2)
    g = np.array(gq, order="F")
    w = np.full((B, 101), -7, dtype=np.int32)
    p = np.full((B, 101), -7.)
    mine = m.upload(docs)
    longer = m.upload(_docs(V, B + 1, 7))
    other = DeviceBatch(docs, V + 1, 0)
    trlda_amd.seed(3)
    want = _draw_state()
    trlda_amd.seed(3)
    ptr = _ffi.vp()
    _ffi.check(hip.trlda_dev_alloc(0, g.nbytes, C.byref(ptr)))
    try:
        for top_n, batch, code in ((0, mine, _ffi.ERR_ARG), (-1, mine, _ffi.ERR_ARG), (V + 1, mine, _ffi.ERR_ARG),
                                   (101, mine, _ffi.ERR_ARG), (1, other, _ffi.ERR_ARG)):
            assert hip.trlda_model_recommend(m._handle, batch.handle, g.ctypes.data, top_n, 1, 20, 1e-3,
                                             w.ctypes.data, p.ctypes.data) == code
            assert hip.trlda_model_recommend_dev(m._handle, batch.handle, ptr, B, top_n, ptr, ptr) == code
        assert hip.trlda_model_recommend(m._handle, None, g.ctypes.data, 1, 1, 20, 1e-3, w.ctypes.data,
                                         p.ctypes.data) == _ffi.ERR_ARG
        assert hip.trlda_model_recommend_dev(m._handle, longer.handle, ptr, B, 1, ptr, ptr) == _ffi.ERR_SHAPE
        assert hip.trlda_model_recommend_dev(m._handle, None, None, B, 1, ptr, ptr) == _ffi.ERR_ARG
        assert hip.trlda_model_recommend_dev(m._handle, None, ptr, -1, 1, ptr, ptr) == _ffi.ERR_ARG
    finally:
        hip.trlda_dev_free(0, ptr)
    for words in (-16, 8, 17):
        assert hip.trlda_model_set_recommend_slab_words(m._handle, words) == _ffi.ERR_ARG
    with pytest.raises(RuntimeError, match="different model"):
        m.recommend(other)
    with pytest.raises(RuntimeError, match="different model"):
        m.recommend_gamma(gq, docs=other)
    with pytest.raises(RuntimeError, match="Initial gamma has wrong dimensionality."):
        m.recommend(docs, latents=np.ones((K, B + 1)))
    with pytest.raises(RuntimeError, match="same number of documents"):
        m.recommend_gamma(gq, docs=longer)
    with pytest.raises(RuntimeError, match="top_n"):
        m.recommend(docs, top_n=V + 1)
    # nothing was drawn or written
    assert _draw_state() == want
    assert np.array_equal(g, gq) and np.all(w == -7) and np.all(p == -7.)
    # the model still works after the refusals
    got, probs = m.recommend(mine, top_n=V, exclude_seen=False)
    assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(V), (B, 1))) and np.all(np.diff(probs, axis=1) <= 0)
    for b in (mine, longer, other):
        b.close()
    m.close()


def test_above_the_vi_bound(hip):
    """The E-step form refuses K above TRLDA_VI_MAX_TOPICS before it draws; the gamma form takes it."""
    import trlda_amd
    from trlda_amd import _ffi
    K, V = _ffi.vi_max_topics() + 1, 20
    lam = _lam(K, V)
    m = _model(K, V, lam)
    try:
        trlda_amd.seed(3)
        want = _draw_state()
        trlda_amd.seed(3)
        with pytest.raises(_ffi.TrldaError, match="TRLDA_VI_MAX_TOPICS"):
            m.recommend([[(0, 1)]], top_n=1)
        with pytest.raises(_ffi.TrldaError, match="TRLDA_VI_MAX_TOPICS"):
            m.recall_at([[(0, 1)]], [[(1, 1)]], top_n=1)
        batch = m.upload([[(0, 1)]])
        g, w, p = np.ones((K, 1), order="F"), np.zeros(1, dtype=np.int32), np.zeros(1)
        assert hip.trlda_model_recommend(m._handle, batch.handle, g.ctypes.data, 1, 1, 10, 1e-3, w.ctypes.data,
                                         p.ctypes.data) == _ffi.ERR_ARG
        batch.close()
        assert _draw_state() == want
        gq, docs = _gammas(K, 5, 3), _docs(V, 5, 4, length=3)
        words, probs = m.recommend_gamma(gq, top_n=7, docs=docs)
        _compare(K, V, 7, words, probs, gq, lam, _triple(docs))
    finally:
        m.close()


# 8. buffers ------------------------------------------------------------------------------------------
def test_no_buffer_is_left_after_close(hip):
    """A fresh process (the count is the process's): both forms, with and without seen words, two slab
    widths, recall_at; after close() the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "recommend_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout
