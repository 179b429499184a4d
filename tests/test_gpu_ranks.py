"""LDA.heldout_ranks / heldout_ranks_gamma / ranking_metrics on the GPU (csrc/ranks_kernels.h, DESIGN.md
3.30): the ranks are integers, so they are compared exactly -- completely against ``recommend`` where
its list can hold the whole vocabulary, against the longdouble restatement (tests/ranks_host.py)
beyond --, the scores bitwise against ``recommend``'s; exact ties across slabs, the threshold chunk,
independence of the partition, the forms, the metrics, the model's state, the errors and the buffers.

Every array is small: at most 700 words, 130 documents and 2276 topics (never all three at once)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ranks_host as kh
import recommend_host as rh

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GAP_FLOOR = 1e-9                         # relative: the floor of tests/test_gpu_recommend.py


def prob_bound(K, V):
    """|s_dev - s_longdouble| / s: the bound of DESIGN.md 3.22, (V + 2 K + 8) u."""
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


def _chunk(hip, m, pairs):
    from trlda_amd import _ffi
    _ffi.check(hip.trlda_model_set_ranks_chunk(m._handle, pairs))


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def _c_form(hip, m, gamma, heldout, observed=None):
    """trlda_model_heldout_ranks_dev itself: (ranks, scores, candidates) aligned with heldout's entries."""
    from trlda_amd import _ffi
    g = np.asfortranarray(gamma, dtype=np.float64)
    B = g.shape[1]
    held = m.upload(heldout)
    obs = m.upload(observed) if observed is not None else None
    nnz = len(held.csr.ids)
    ranks, scores, cand = np.full(nnz, -7, dtype=np.int32), np.full(nnz, -7.), np.full(B, -7, dtype=np.int32)
    ptrs = []
    try:
        for nbytes in (g.nbytes, ranks.nbytes, scores.nbytes, cand.nbytes):
            ptr = _ffi.vp()
            _ffi.check(hip.trlda_dev_alloc(0, max(nbytes, 8), C.byref(ptr)))
            ptrs.append(ptr)
        _ffi.check(hip.trlda_dev_upload(0, ptrs[0], g.ctypes.data, g.nbytes))
        _ffi.check(hip.trlda_model_heldout_ranks_dev(m._handle, None if obs is None else obs.handle, held.handle,
                                                     ptrs[0], B, ptrs[1], ptrs[2], ptrs[3]))
        _ffi.check(hip.trlda_model_synchronize(m._handle))
        for a, ptr in ((ranks, ptrs[1]), (scores, ptrs[2]), (cand, ptrs[3])):
            if a.nbytes:
                _ffi.check(hip.trlda_dev_download(0, a.ctypes.data, ptr, a.nbytes))
    finally:
        for ptr in ptrs:
            hip.trlda_dev_free(0, ptr)
        held.close()
        if obs is not None:
            obs.close()
    return ranks, scores, cand


def _relevant(observed, heldout, V):
    """Per document the relevant words in ascending id, by the definition."""
    held = rh.seen(*heldout, V)
    obs = rh.seen(*observed, V) if observed is not None else np.zeros_like(held)
    return [np.flatnonzero(held[d] & ~obs[d]) for d in range(held.shape[0])]


# 1. complete and exact against recommend -------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 100])
@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 100])
def test_complete_against_recommend(hip, K, V):
    """V <= 100: recommend_gamma(top_n=V) is the whole ranking.  Every relevant word's rank is its
    position + 1 there, its score that entry's bits, candidates the row's non-pad entries.  No
    tolerance and no tie caveat.  B = 17, and 130, which crosses the tile of 128 documents."""
    lam = _lam(K, V)
    m = _model(K, V, lam)
    checked = 0
    for B in (17, 130):
        gq = _gammas(K, B, 500 + V)
        observed, heldout = _docs(V, B, V, length=min(3, V)), _docs(V, B, V + 1000, length=min(5, 2 * V))
        for obs in (observed, None):
            full, probs = m.recommend_gamma(gq, top_n=V, docs=obs)
            indptr, words, ranks, cand, scores = m.heldout_ranks_gamma(gq, heldout, docs=obs, return_scores=True)
            assert indptr.dtype == np.int64 and words.dtype == ranks.dtype == cand.dtype == np.int32
            assert scores.dtype == np.float64 and indptr.shape == (B + 1,) and cand.shape == (B,)
            assert np.array_equal(cand, (full >= 0).sum(axis=1))
            want = _relevant(None if obs is None else _triple(obs), _triple(heldout), V)
            for d in range(B):
                mine = slice(indptr[d], indptr[d + 1])
                assert np.array_equal(words[mine], want[d]), (B, d)
                assert np.all(ranks[mine] >= 1) and np.all(ranks[mine] <= cand[d])
                assert np.array_equal(full[d, ranks[mine] - 1], words[mine]), (B, d)
                assert np.array_equal(probs[d, ranks[mine] - 1], scores[mine]), (B, d)
                checked += len(want[d])
    assert checked > 0
    m.close()


# 2. V = 300, where the list stops at 100 -------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 64, 65, 100, 513, 2276])
def test_beyond_the_list(hip, K):
    """V = 300, B in 1, 17, 33.  Every relevant word of rank <= 100 sits at that position of
    recommend_gamma(top_n=100) with the same bits, and every relevant word that list holds has that
    rank.  All ranks equal the restatement's: its inputs have no near tie -- the smallest relative
    gap between a relevant word's score and any other candidate's stays above GAP_FLOOR for every
    case (checked on the CPU when the seeds were chosen, asserted here first).  Scores within
    (V + 2 K + 8) u of the longdouble value."""
    V, B_max = 300, 33
    lam, gq = _lam(K, V), _gammas(K, B_max, 9000 + K)
    # (without the generator's empty first document: B = 1 ranks something)
    observed = _docs(V, B_max + 1, K).slice(1, B_max + 1)
    heldout = _docs(V, B_max + 1, K + 5000, length=10).slice(1, B_max + 1)
    s = rh.scores(gq, lam)
    m = _model(K, V, lam)
    worst, in_list = 0.0, 0
    for B in (1, 17, 33):
        obs, held = observed.slice(0, B), heldout.slice(0, B)
        want = kh.ranks(gq[:, :B], lam, _triple(obs), _triple(held), s=s[:B])
        assert len(want[5]) == 0 or want[5].min() > GAP_FLOOR, (K, B, want[5].min())
        indptr, words, ranks, cand, scores = m.heldout_ranks_gamma(gq[:, :B], held, docs=obs, return_scores=True)
        assert np.array_equal(indptr, want[0]) and np.array_equal(words, want[1])
        assert np.array_equal(ranks, want[2]), (K, B)
        assert np.array_equal(cand, want[3])
        if len(scores):
            err = float(np.max(np.abs(scores.astype(np.longdouble) - want[4]) / want[4]))
            assert err <= prob_bound(K, V), (K, B, err / U)
            worst = max(worst, err)
        top, probs = m.recommend_gamma(gq[:, :B], top_n=100, docs=obs)
        relevant = _relevant(_triple(obs), _triple(held), V)
        for d in range(B):
            mine = slice(indptr[d], indptr[d + 1])
            near = ranks[mine] <= 100
            assert np.array_equal(top[d, ranks[mine][near] - 1], words[mine][near]), (K, B, d)
            assert np.array_equal(probs[d, ranks[mine][near] - 1], scores[mine][near]), (K, B, d)
            listed = np.flatnonzero(np.isin(top[d], relevant[d]))         # and conversely
            assert np.array_equal(np.sort(ranks[mine][near]), listed + 1), (K, B, d)
            in_list += len(listed)
    assert in_list > 0
    print("K = %d: max rel err of s %.2f u (bound %d u)" % (K, worst / U, V + 2 * K + 8))
    m.close()


# 3. exact ties ---------------------------------------------------------------------------------------
def test_exact_ties_across_slabs(hip):
    """V = 300 in slabs of 64: words 5, 70 and 250 (slabs 0, 1 and 3) have the same column of lambda,
    hence equal scores.  Held out together with nothing seen they rank r, r + 1, r + 2, by id.  With one
    of them seen, one held out and one neither, the seen one is not counted and the other counts
    only where its id is smaller."""
    K, V, B = 37, 300, 17
    tied = (5, 70, 250)
    lam = _lam(K, V)
    lam[:, 70] = lam[:, 5]
    lam[:, 250] = lam[:, 5]
    gq = _gammas(K, B, 77)
    m = _model(K, V, lam)
    _slab(hip, m, 64)
    held_all = [[(w, 1) for w in tied]] * B
    indptr, words, base, cand, scores = m.heldout_ranks_gamma(gq, held_all, return_scores=True)
    assert np.all(cand == V) and np.array_equal(words, np.tile(tied, B))
    base = base.reshape(B, 3)
    scores = scores.reshape(B, 3)
    assert np.array_equal(base[:, 1], base[:, 0] + 1) and np.array_equal(base[:, 2], base[:, 0] + 2)
    assert np.array_equal(scores[:, 0], scores[:, 1]) and np.array_equal(scores[:, 0], scores[:, 2])
    assert len(set(base[:, 0])) > 1                        # (the documents differ)
    r = base[:, 0]
    for held, seen, shift in ((70, 5, 0), (5, 70, 0), (250, 5, 1), (250, 70, 1), (5, 250, 0), (70, 250, 1)):
        got = m.heldout_ranks_gamma(gq, [[(held, 2)]] * B, docs=[[(seen, 1)]] * B, return_scores=True)
        assert np.array_equal(got[1], np.full(B, held)) and np.all(got[3] == V - 1)
        assert np.array_equal(got[2], r + shift), (held, seen)
        assert np.array_equal(got[4], scores[:, 0])
    # the seen one held out as well: it is never ranked
    got = m.heldout_ranks_gamma(gq, [[(5, 1), (70, 1)]] * B, docs=[[(5, 1)]] * B)
    assert np.array_equal(got[1], np.full(B, 70)) and np.array_equal(got[2], r)
    # against the restatement, whose tied scores are equal too and go by id
    want = kh.ranks(gq, lam, None, (np.arange(B + 1) * 3, np.tile(tied, B), np.ones(3 * B, dtype=int)))
    assert np.all((want[5] == 0) | (want[5] > GAP_FLOOR))
    assert np.array_equal(want[2].reshape(B, 3), base)
    m.close()


# 4. the threshold chunk ------------------------------------------------------------------------------
def _chunk_case(V, B):
    """B documents whose held-out parts have 0, 1, 4, 5, 9 and 33 candidate entries (in turn; document
    B - 1 has 33) -- from 4 on one of them a repeated word --, plus per document an entry with c = 0,
    one with c = -1 and a word that is also in the observed part, the entries shuffled; word V - 1 is
    held out by document B - 1 and seen by document 2.  Returns the two parts and per document the
    numbers of candidate entries and of distinct candidate words."""
    from trlda_amd.documents import CSRDocuments
    rng = np.random.RandomState(41)
    sizes = [(0, 1, 4, 5, 9, 33)[d % 6] for d in range(B)]
    sizes[B - 1] = 33
    distinct = [n - (n >= 4) for n in sizes]
    obs_docs, held_docs = [], []
    for d in range(B):
        words = rng.permutation(V - 1)[:distinct[d] + 8]
        seen, cand, spare = words[:4], list(words[4:4 + distinct[d]]), words[4 + distinct[d]:]
        if d == B - 1:
            cand[0] = V - 1
        if d == 2:
            seen = np.append(seen, V - 1)
        entries = [(int(w), int(rng.randint(1, 4))) for w in cand]
        if sizes[d] >= 4:
            entries.append((int(cand[0]), 2))                        # a repeated word
        entries += [(int(spare[0]), 0), (int(spare[1]), -1), (int(seen[0]), 3)]
        order = rng.permutation(len(entries))
        held_docs.append([entries[i] for i in order])
        obs_docs.append([(int(w), 1) for w in seen] + [(int(spare[2]), 0)])
    def csr(docs):
        indptr = np.cumsum([0] + [len(x) for x in docs])
        flat = [p for x in docs for p in x]
        return CSRDocuments(indptr, np.array([p[0] for p in flat]), np.array([p[1] for p in flat]))
    return csr(obs_docs), csr(held_docs), sizes, distinct


def test_threshold_chunk_and_slabs(hip):
    """V = 700, B = 65: the C form at the default chunk and slab against chunk 4 (the longest document, 36 entries
    of which 33 are candidates, takes nine sweeps), slabs of 64 and 128, and both at once: bitwise the same.
    Entries with c <= 0 and words also in `observed` give 0 in the C form and are absent from the
    Python form; a repeated word has its rank twice in the C form and once in the Python form."""
    K, V, B = 37, 700, 65
    lam, gq = _lam(K, V), _gammas(K, B, 78)
    observed, heldout, sizes, distinct = _chunk_case(V, B)
    m = _model(K, V, lam)
    ref = _c_form(hip, m, gq, heldout, observed)
    py_ref = m.heldout_ranks_gamma(gq, heldout, docs=observed, return_scores=True)
    for chunk, slab in ((4, 0), (0, 64), (0, 128), (4, 64), (1, 128)):
        _chunk(hip, m, chunk)
        _slab(hip, m, slab)
        assert _same(_c_form(hip, m, gq, heldout, observed), ref), (chunk, slab)
        assert _same(m.heldout_ranks_gamma(gq, heldout, docs=observed, return_scores=True), py_ref), (chunk, slab)
    _chunk(hip, m, 0)
    _slab(hip, m, 0)
    ranks, scores, cand = ref
    seen = rh.seen(*_triple(observed), V)
    indptr, words, py_ranks, py_cand, py_scores = py_ref
    assert np.array_equal(cand, V - seen.sum(axis=1)) and np.array_equal(py_cand, cand)
    assert np.array_equal(np.diff(indptr), distinct)
    for d in range(B):
        lo, hi = heldout.indptr[d], heldout.indptr[d + 1]
        ids, cnts = heldout.ids[lo:hi], heldout.cnts[lo:hi]
        no = (cnts <= 0) | seen[d][ids]
        assert np.all(ranks[lo:hi][no] == 0) and np.all(scores[lo:hi][no] == 0.0)
        assert np.all(ranks[lo:hi][~no] >= 1) and np.count_nonzero(~no) == sizes[d]
        by_word = {}
        for w, r, s in zip(ids[~no], ranks[lo:hi][~no], scores[lo:hi][~no]):
            assert by_word.setdefault(w, (r, s)) == (r, s)              # listed twice: the rank twice
        mine = slice(indptr[d], indptr[d + 1])
        assert list(words[mine]) == sorted(by_word)
        assert [by_word[w] for w in words[mine]] == list(zip(py_ranks[mine], py_scores[mine]))
    assert words[-1] == V - 1 and indptr[B] - indptr[B - 1] == 32
    # and the ranks are the restatement's
    want = kh.ranks(gq, lam, _triple(observed), _triple(heldout))
    assert want[5].min() > GAP_FLOOR
    assert np.array_equal(want[1], words) and np.array_equal(want[2], py_ranks) and np.array_equal(want[3], cand)
    with pytest.raises(Exception):
        _chunk(hip, m, 33)
    with pytest.raises(Exception):
        _chunk(hip, m, -1)
    m.close()


# 5. independence -------------------------------------------------------------------------------------
def test_independence_and_forms(hip):
    """Bitwise: two calls; a document alone against the same document inside a batch of 33; 130
    documents against the same in three calls; heldout_ranks against heldout_ranks_gamma on the gamma
    it returned; a list against an uploaded batch; docs=None gives candidates == V."""
    K, V, B = 65, 300, 33
    lam, gq = _lam(K, V), _gammas(K, B, 21)
    observed, heldout = _docs(V, B, 22), _docs(V, B, 23, length=9)
    m = _model(K, V, lam)
    _slab(hip, m, 64)
    ref = m.heldout_ranks_gamma(gq, heldout, docs=observed, return_scores=True)
    assert _same(m.heldout_ranks_gamma(gq, heldout, docs=observed, return_scores=True), ref)
    assert _same(m.heldout_ranks_gamma(gq, heldout, docs=observed), ref[:4])
    indptr = ref[0]
    for d in range(B):
        one = m.heldout_ranks_gamma(gq[:, d], heldout.slice(d, d + 1), docs=observed.slice(d, d + 1),
                                    return_scores=True)
        mine = slice(indptr[d], indptr[d + 1])
        assert np.array_equal(one[0], [0, indptr[d + 1] - indptr[d]])
        assert all(np.array_equal(one[i], ref[i][mine]) for i in (1, 2, 4)) and one[3][0] == ref[3][d], d
    every = m.heldout_ranks_gamma(gq, heldout)
    assert np.all(every[3] == V) and np.array_equal(every[0][-1:], [sum(len(w) for w in _relevant(None, _triple(heldout), V))])
    many, mobs, mheld = _gammas(K, 130, 24), _docs(V, 130, 25), _docs(V, 130, 26, length=9)
    whole = m.heldout_ranks_gamma(many, mheld, docs=mobs, return_scores=True)
    for lo, hi in ((0, 50), (50, 129), (129, 130)):
        part = m.heldout_ranks_gamma(many[:, lo:hi], mheld.slice(lo, hi), docs=mobs.slice(lo, hi), return_scores=True)
        mine = slice(whole[0][lo], whole[0][hi])
        assert np.array_equal(part[0], whole[0][lo:hi + 1] - whole[0][lo])
        assert all(np.array_equal(part[i], whole[i][mine]) for i in (1, 2, 4))
        assert np.array_equal(part[3], whole[3][lo:hi])
    # the E-step form
    g0 = np.asfortranarray(np.random.RandomState(4).gamma(1.0, 1.0, size=(K, B)) + 0.1)
    want_gamma, _ = m.update_variables(observed, latents=g0, max_iter=20)
    out = m.heldout_ranks(observed, heldout, latents=g0, max_iter=20, return_scores=True, return_gamma=True)
    assert len(out) == 6 and np.array_equal(out[5], want_gamma)
    assert _same(m.heldout_ranks_gamma(out[5], heldout, docs=observed, return_scores=True), out[:5])
    assert _same(m.heldout_ranks(observed, heldout, latents=g0, max_iter=20), out[:4])
    o_batch, h_batch = m.upload(observed), m.upload(heldout)
    a = m.heldout_ranks(observed.to_list(), heldout.to_list(), latents=g0, max_iter=20, return_scores=True)
    b = m.heldout_ranks(o_batch, h_batch, latents=g0, max_iter=20, return_scores=True)
    c = m.heldout_ranks_gamma(want_gamma, h_batch, docs=o_batch, return_scores=True)
    o_batch.close()
    h_batch.close()
    assert _same(a, out[:5]) and _same(b, out[:5]) and _same(c, out[:5])
    # the scores are recommend's bits
    top, probs = m.recommend(observed, top_n=100, latents=g0, max_iter=20)
    for d in range(B):
        mine = slice(out[0][d], out[0][d + 1])
        near = out[2][mine] <= 100
        assert np.array_equal(top[d, out[2][mine][near] - 1], out[1][mine][near])
        assert np.array_equal(probs[d, out[2][mine][near] - 1], out[4][mine][near])
    # empty batches
    for got in (m.heldout_ranks([], []), m.heldout_ranks_gamma(np.empty((K, 0)), [])):
        assert [len(x) for x in got] == [1, 0, 0, 0]
    none = m.heldout_ranks_gamma(gq[:, :2], [[], []], docs=[[(0, 1)], []])
    assert list(none[0]) == [0, 0, 0] and list(none[3]) == [V - 1, V]
    m.close()


# 6. metrics end to end -------------------------------------------------------------------------------
def test_recall_of_the_metrics_is_recall_at(hip):
    """ranking_metrics(...)["recall"][N] == recall_at(..., top_n=N) exactly for N = 1, 20, 100 on the
    same gamma0.  Every document has 1, 2 or 4 relevant words, so every ratio is a multiple of 1/4 and
    the two means (recall_at adds in document order, the metrics through math.fsum) are both exact;
    per document hits / relevant are compared on documents of any size."""
    K, V, B = 10, 300, 40
    rng = np.random.RandomState(5)
    lam = _lam(K, V)
    m = _model(K, V, lam)
    g0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)
    observed, heldout, mixed = [], [], []
    for d in range(B):
        words = rng.permutation(V)
        observed.append([(int(w), int(rng.randint(1, 3))) for w in words[:10]])
        heldout.append([(int(w), 1) for w in words[10:10 + (1, 2, 4)[d % 3]]] + [(int(words[0]), 1)])
        mixed.append([(int(w), 1) for w in words[10:10 + d % 7]])
    got = m.ranking_metrics(observed, heldout, top_n=(1, 20, 100), latents=g0, max_iter=20)
    for n in (1, 20, 100):
        assert got["recall"][n] == m.recall_at(observed, heldout, top_n=n, latents=g0, max_iter=20), n
    assert 0.0 <= got["recall"][1] <= got["recall"][20] <= got["recall"][100] <= 1.0
    assert 0.0 < got["mean_percentile_rank"] < 1.0 and 0.0 < got["auc"] < 1.0
    got = m.ranking_metrics(observed, mixed, top_n=(1, 20, 100), latents=g0, max_iter=20, return_documents=True)
    for n in (1, 20, 100):
        recall, hits, relevant = m.recall_at(observed, mixed, top_n=n, latents=g0, max_iter=20, return_documents=True)
        keep = relevant > 0
        assert np.array_equal(got["documents"]["relevant"], relevant)
        assert np.array_equal(got["documents"]["recall"][n][keep], hits[keep] / relevant[keep])
        assert np.all(np.isnan(got["documents"]["recall"][n][~keep])) and abs(got["recall"][n] - recall) <= 4 * U
    with pytest.raises(RuntimeError, match="held-out"):
        m.ranking_metrics(observed, observed, latents=g0, max_iter=20)
    m.close()


def test_direction_of_the_percentile_rank(hip):
    """120 documents of 60 tokens sampled from a known K = 10, V = 500 model (each topic 50 words of
    its own) and split by split_documents: their mean percentile rank under the generating model is
    below that under a constant lambda.  Under a constant lambda every score ties and the ranks go by
    id, so that figure follows from the ids alone: it is computed by hand and asserted."""
    import math
    import trlda_amd
    from trlda_amd.documents import as_csr
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils import split_documents
    K, V, B = 10, 500, 120
    rng = np.random.RandomState(0)
    truth = np.full((K, V), 0.01)
    for k in range(K):
        truth[k, k * 50:(k + 1) * 50] = rng.gamma(5.0, 1.0, size=50)
    src = OnlineLDA(num_words=V, num_topics=K, num_documents=1, alpha=.1, eta=.01, device=0)
    src.lambdas = truth * 100.
    trlda_amd.seed(1)
    corpus = src.sample(B, 60)
    obs, out = split_documents(corpus, heldout=0.3)
    g0 = np.ones((K, B))
    good = src.ranking_metrics(obs, out, top_n=(20, 500), latents=g0)
    src.close()
    flat = _model(K, V, np.full((K, V), 1.0))
    base = flat.ranking_metrics(obs, out, top_n=(20, 500), latents=g0)
    indptr, words, ranks, cand = flat.heldout_ranks(obs, out, latents=g0)
    flat.close()
    o = as_csr(obs)
    unseen = ~rh.seen(o.indptr, o.ids, o.cnts, V)
    terms = []
    for d in range(B):
        before = np.cumsum(unseen[d]) - unseen[d]                        # unseen words of smaller id
        mine = slice(indptr[d], indptr[d + 1])
        assert np.array_equal(ranks[mine], before[words[mine]] + 1) and cand[d] == unseen[d].sum()
        terms.extend((before[w] / (cand[d] - 1.0)) for w in words[mine])
    assert abs(base["mean_percentile_rank"] - math.fsum(terms) / len(terms)) <= 1e-15
    print("mean percentile rank: the sampling model %.4f, a constant lambda %.4f; AUC %.4f / %.4f" %
          (good["mean_percentile_rank"], base["mean_percentile_rank"], good["auc"], base["auc"]))
    assert good["mean_percentile_rank"] < base["mean_percentile_rank"]
    assert good["auc"] > base["auc"] and good["recall"][500] == base["recall"][500] == 1.0


# 7. the model's state --------------------------------------------------------------------------------
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
    lam, docs, other, held = _lam(K, V), _docs(V, B, 5), _docs(V, B, 6), _docs(V, B, 8, length=7)
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
            kept = np.empty((K, V), order="F")
            _ffi.check(hip.trlda_model_get_sstats(m._handle, kept))
            trlda_amd.seed(9)
            want = _draw_state()
            trlda_amd.seed(9)
            m.heldout_ranks_gamma(g1, held, docs=other)
            m.heldout_ranks_gamma(g1, held, return_scores=True)
            assert _draw_state() == want                              # nothing was drawn
            after = np.empty((K, V), order="F")
            _ffi.check(hip.trlda_model_get_sstats(m._handle, after))
            assert np.array_equal(kept, after)                        # no E-step ran
            assert np.array_equal(kept, out[0][1])
            after = np.empty((K, V), order="F")
            # the E-step form with latents=None draws the K B values of update_variables
            trlda_amd.seed(9)
            m.heldout_ranks(other, held)
            drawn = _draw_state()
            trlda_amd.seed(9)
            m.update_variables(other)
            assert _draw_state() == drawn
            m.ranking_metrics(other, held, latents=g1, max_iter=20)
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


def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    from trlda_amd import _ffi
    from trlda_amd.documents import DeviceBatch
    K, V, B = 8, 40, 4
    lam, docs, held_docs = _lam(K, V), _docs(V, B, 7), _docs(V, B, 9, length=5)
    m = _model(K, V, lam)
    gq = _gammas(K, B, 2)
    g = np.array(gq, order="F")
    nnz = len(held_docs.ids)
    r = np.full(nnz, -7, dtype=np.int32)
    s = np.full(nnz, -7.)
    c = np.full(B, -7, dtype=np.int32)
    mine, held = m.upload(docs), m.upload(held_docs)
    longer = m.upload(_docs(V, B + 1, 7))
    other = DeviceBatch(docs, V + 1, 0)
    live = C.c_longlong(-1)
    total = C.c_longlong(-1)
    _ffi.check(hip.trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    trlda_amd.seed(3)
    want = _draw_state()
    trlda_amd.seed(3)
    ptr = _ffi.vp()
    _ffi.check(hip.trlda_dev_alloc(0, g.nbytes, C.byref(ptr)))
    try:
        def host(o, h, gamma=g.ctypes.data, ranks=r.ctypes.data, cand=c.ctypes.data):
            return hip.trlda_model_heldout_ranks(m._handle, o, h, gamma, 1, 20, 1e-3, ranks, s.ctypes.data, cand)
        def dev(o, h, n=B, gamma=ptr, cand=ptr):
            return hip.trlda_model_heldout_ranks_dev(m._handle, o, h, gamma, n, ptr, ptr, cand)
        assert host(other.handle, held.handle) == _ffi.ERR_ARG
        assert host(mine.handle, other.handle) == _ffi.ERR_ARG
        assert host(None, held.handle) == _ffi.ERR_ARG and host(mine.handle, None) == _ffi.ERR_ARG
        assert host(mine.handle, longer.handle) == _ffi.ERR_SHAPE
        assert host(longer.handle, held.handle) == _ffi.ERR_SHAPE
        assert host(mine.handle, held.handle, gamma=None) == _ffi.ERR_ARG
        assert host(mine.handle, held.handle, ranks=None) == _ffi.ERR_ARG
        assert host(mine.handle, held.handle, cand=None) == _ffi.ERR_ARG
        assert dev(other.handle, held.handle) == _ffi.ERR_ARG and dev(mine.handle, other.handle) == _ffi.ERR_ARG
        assert dev(None, None) == _ffi.ERR_ARG
        assert dev(mine.handle, longer.handle) == _ffi.ERR_SHAPE and dev(longer.handle, held.handle) == _ffi.ERR_SHAPE
        assert dev(None, held.handle, n=B + 1) == _ffi.ERR_SHAPE and dev(None, held.handle, n=-1) == _ffi.ERR_ARG
        assert dev(None, held.handle, gamma=None) == _ffi.ERR_ARG and dev(None, held.handle, cand=None) == _ffi.ERR_ARG
    finally:
        hip.trlda_dev_free(0, ptr)
    for pairs in (-1, 33):
        assert hip.trlda_model_set_ranks_chunk(m._handle, pairs) == _ffi.ERR_ARG
    with pytest.raises(RuntimeError, match="different model"):
        m.heldout_ranks(other, held)
    with pytest.raises(RuntimeError, match="different model"):
        m.heldout_ranks_gamma(gq, other)
    with pytest.raises(RuntimeError, match="Initial gamma has wrong dimensionality."):
        m.heldout_ranks(docs, held_docs, latents=np.ones((K, B + 1)))
    with pytest.raises(RuntimeError, match="equal in number"):
        m.heldout_ranks(mine, longer)
    with pytest.raises(RuntimeError, match="same number of documents"):
        m.heldout_ranks_gamma(gq, longer)
    # nothing was drawn, written or allocated
    assert _draw_state() == want
    assert np.array_equal(g, gq) and np.all(r == -7) and np.all(s == -7.) and np.all(c == -7)
    now = C.c_longlong(-1)
    _ffi.check(hip.trlda_debug_device_buffers(C.byref(now), C.byref(total)))
    assert now.value == live.value
    # the model still works after the refusals
    got = m.heldout_ranks(mine, held)
    assert len(got[1]) > 0 and np.all(got[2] >= 1) and np.all(got[3] <= V)
    for b in (mine, held, longer, other):
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
            m.heldout_ranks([[(0, 1)]], [[(1, 1)]])
        with pytest.raises(_ffi.TrldaError, match="TRLDA_VI_MAX_TOPICS"):
            m.ranking_metrics([[(0, 1)]], [[(1, 1)]])
        o, h = m.upload([[(0, 1)]]), m.upload([[(1, 1)]])
        g, r, c = np.ones((K, 1), order="F"), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        assert hip.trlda_model_heldout_ranks(m._handle, o.handle, h.handle, g.ctypes.data, 1, 10, 1e-3, r.ctypes.data,
                                             None, c.ctypes.data) == _ffi.ERR_ARG
        o.close()
        h.close()
        assert _draw_state() == want
        gq, docs, held = _gammas(K, 5, 3), _docs(V, 5, 4, length=3), _docs(V, 5, 6, length=4)
        got = m.heldout_ranks_gamma(gq, held, docs=docs, return_scores=True)
        full, probs = m.recommend_gamma(gq, top_n=V, docs=docs)
        assert len(got[1]) > 0 and np.array_equal(got[3], (full >= 0).sum(axis=1))
        for d in range(5):
            mine = slice(got[0][d], got[0][d + 1])
            assert np.array_equal(full[d, got[2][mine] - 1], got[1][mine])
            assert np.array_equal(probs[d, got[2][mine] - 1], got[4][mine])
    finally:
        m.close()


# 8. buffers ------------------------------------------------------------------------------------------
def test_no_buffer_is_left_after_close(hip):
    """A fresh process (the count is the process's): both forms, with and without seen words, two slab
    widths, two chunks, ranking_metrics; after close() the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ranks_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout
