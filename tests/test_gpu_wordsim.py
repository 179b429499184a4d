"""LDA.similar_words / words_near / word_topic_proportions on the GPU (csrc/wordsim_kernels.h,
DESIGN.md 3.28) against the longdouble restatement (tests/wordsim_host.py): ids exactly and s within
the first-order bound under the gap condition; chunk, tile, slab and batch edges; symmetry and
independence, bitwise; exact ties; the weights; the model's state, the errors and the buffers.

Every array is small: at most 2100 words, 129 queries and 2276 topics (never all at once)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import wordsim_host as wh

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GAP_FLOOR = 1e-9                         # the project's floor: the smallest gap among the first top_n + 1
MEASURES = ("hellinger", "cosine")
LD = np.longdouble


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


def _lam(K, V, seed=None):
    return np.random.RandomState(1000 + K if seed is None else seed).gamma(0.3, 1.0, size=(K, V)) + 0.01


def _given(K):
    return np.random.RandomState(2000 + K).gamma(2.0, 1.0, K) + 0.1


def _queries(K, V, B):
    """B query words: word V - 1 (the clamp of the last group must not enter it twice), a repeated
    id, the rest drawn.  The seed base 5000 was chosen on the CPU so that the input condition holds
    in every case of this file (3000 gave a gap of 5.3e-10 at K = 2276, hellinger, given weights,
    top_n = 100; 4000 one of 1.3e-10 at K = 513, cosine); smallest gap with it 4.6e-9."""
    q = np.random.RandomState(5000 + K + V).randint(0, V, size=B)
    q[0] = V - 1
    if B > 2:
        q[2] = q[1]
    return q


def _slab(hip, m, words):
    from trlda_amd import _ffi
    _ffi.check(hip.trlda_model_set_wordsim_slab_words(m._handle, words))


class Ref(object):
    """The restatement of one (lambda, weights, measure, queries): the similarities once."""

    def __init__(self, lam, given, measure, queries):
        self.K, self.V = lam.shape
        self.measure, self.given, self.queries = measure, given, np.asarray(queries)
        self.rows = wh.rows(lam, measure, given)
        self.s = wh.similarities(self.rows[self.queries], self.rows)
        self.bound = wh.sim_bound(self.K, measure, V=self.V, given=given is not None)

    def search(self, top_n, exclude_self=True):
        return wh.search_s(self.s, top_n, self.queries if exclude_self else None)


def _check(m, ref, top_n, exclude_self=True):
    """The input condition, then ids exactly and s within the bound (relative); the distances are the
    conversion of the similarities.  Returns the worst error as a fraction of the bound."""
    want_ids, want_s, gap = ref.search(top_n, exclude_self)
    assert gap > GAP_FLOOR, (ref.K, ref.V, ref.measure, top_n, gap)
    kw = dict(measure=ref.measure, topic_weights=ref.given, exclude_self=exclude_self)
    ids, s = m.similar_words(ref.queries, top_n, return_similarity=True, **kw)
    assert ids.dtype == np.int32 and s.dtype == np.float64 and ids.shape == s.shape == (len(ref.queries), top_n)
    assert np.array_equal(ids, want_ids), (ref.K, ref.V, ref.measure, top_n)
    err = np.abs(s.astype(LD) - want_s) / want_s
    frac = float(err.max()) / ref.bound
    print("K = %d V = %d %s %s top_n = %d: rel err %.1f u, %.3f of the bound (%.0f u)"
          % (ref.K, ref.V, ref.measure, "given" if ref.given is not None else "default", top_n,
             float(err.max()) / U, frac, ref.bound / U))
    assert frac <= 1.0, (ref.K, ref.V, ref.measure, top_n, float(err.max()) / U)
    if exclude_self:
        assert not np.any(ids == ref.queries[:, None])
    ids2, dist = m.similar_words(ref.queries, top_n, **kw)
    assert np.array_equal(ids2, ids) and np.array_equal(dist, wh.distance(s, ref.measure))
    return frac, ids, s


# 1. ids and similarities -----------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("K", [3, 5, 31, 32, 33, 65, 100, 513, 2276])
def test_ids_and_similarities(hip, K, given):
    """V = 300, 40 queries, top_n in 1, 32, 33 (the width switch), 100, both measures.  K = 3, 5 (a
    tail of 4), 31 / 32 / 33 and 65 (chunk edges), 100 (more than one element per lane in the column
    pass), 513 and 2276 (many chunks).  lambda = Gamma(0.3) + 0.01, given weights Gamma(2) + 0.1: no
    near ties (the condition is asserted first on the restatement)."""
    V, B = 300, 40
    lam = _lam(K, V)
    pi = _given(K) if given else None
    queries = _queries(K, V, B)
    m = _model(K, V, lam)
    try:
        for measure in MEASURES:
            ref = Ref(lam, pi, measure, queries)
            assert ref.bound <= 1e-3 * GAP_FLOOR             # three orders between the error and what the ids need
            for top_n in (1, 32, 33, 100):
                _, ids, s = _check(m, ref, top_n)
                assert np.array_equal(ids[1], ids[2]) and np.array_equal(s[1], s[2])     # the repeated id
            # the word itself comes first when it may, at s = 1 within the bound
            ids, s = m.similar_words(queries, 1, measure=measure, topic_weights=pi, exclude_self=False,
                                     return_similarity=True)
            assert np.array_equal(ids[:, 0], queries)
            assert float(np.max(np.abs(s - 1.0))) <= ref.bound
    finally:
        m.close()


def test_one_topic(hip):
    """K = 1: every word is the same point, every s is 1 up to rounding -- one exact tie in the
    restatement, so the ids are compared with what the device computed: distinct, in range, never
    the query, ranked (s descending, id ascending), every s within the bound of 1."""
    K, V, B = 1, 300, 5
    lam = _lam(K, V)
    queries = _queries(K, V, B)
    m = _model(K, V, lam)
    try:
        for measure in MEASURES:
            for top_n in (1, 33, 100):
                ids, s = m.similar_words(queries, top_n, measure=measure, return_similarity=True)
                assert float(np.max(np.abs(s - 1.0))) <= wh.sim_bound(K, measure, V=V, given=False)
                for b in range(B):
                    assert len(set(ids[b])) == top_n and queries[b] not in ids[b]
                    assert np.all((ids[b] >= 0) & (ids[b] < V))
                    assert np.all(np.diff(s[b]) <= 0)
                    assert np.all(np.diff(ids[b])[np.diff(s[b]) == 0] > 0)
            p = m.word_topic_proportions(queries)
            assert np.array_equal(p, np.ones((1, B)))
    finally:
        m.close()


# 2. vocabulary and batch edges -----------------------------------------------------------------------
@pytest.mark.parametrize("V", [17, 63, 64, 65])
def test_vocabulary_edges(hip, V):
    """Below / at / past a group of 64 words and V = 17 with top_n = V - 1 = 16; every word is a query
    (B = V: 17, 63, 64, 65 -- tile edges of the 64-query width), K = 33, given weights."""
    K = 33
    lam = _lam(K, V, seed=1000 + K + V)
    queries = np.arange(V)
    m = _model(K, V, lam)
    try:
        for measure in MEASURES:
            ref = Ref(lam, _given(K), measure, queries)
            for top_n in sorted({1, min(V - 1, 33), min(V - 1, 100)}):
                _check(m, ref, top_n)
            _check(m, ref, min(V, 100), exclude_self=False)
    finally:
        m.close()


@pytest.mark.parametrize("B", [1, 63, 65, 129])
def test_batch_edges_and_independence(hip, B):
    """Tile edges of both widths (64 and 128 queries).  A query's row is bitwise the same alone, in
    the batch and under another slab width."""
    K, V = 33, 300
    lam = _lam(K, V)
    queries = _queries(K, V, B)
    m = _model(K, V, lam)
    try:
        for measure in MEASURES:
            ref = Ref(lam, None, measure, queries)
            for top_n in (10, 33):
                _, ids, s = _check(m, ref, top_n)
                for b in sorted({0, B // 2, B - 1}):
                    for slab in (0, 64):
                        _slab(hip, m, slab)
                        i1, s1 = m.similar_words(int(queries[b]), top_n, measure=measure, return_similarity=True)
                        assert i1.shape == (1, top_n)
                        assert np.array_equal(i1[0], ids[b]) and np.array_equal(s1[0], s[b])
                    _slab(hip, m, 0)
    finally:
        m.close()


def test_slabs(hip):
    """V = 2100 with the slab forced to 16 (132 slabs), 48 (a ragged last slab: 2100 = 43 x 48 + 36)
    and 2048 (two slabs, the last of 52 words): bitwise equal outputs, and the restatement's."""
    K, V, B = 100, 2100, 129
    lam = _lam(K, V)
    queries = _queries(K, V, B)
    m = _model(K, V, lam)
    try:
        for measure, pi in (("hellinger", None), ("cosine", _given(K))):
            ref = Ref(lam, pi, measure, queries)
            for top_n in (10, 33):
                out = []
                for slab in (16, 48, 2048):
                    _slab(hip, m, slab)
                    out.append(m.similar_words(queries, top_n, measure=measure, topic_weights=pi,
                                               return_similarity=True))
                _slab(hip, m, 0)
                for ids, s in out[1:]:
                    assert np.array_equal(ids, out[0][0]) and np.array_equal(s, out[0][1])
                _, ids, s = _check(m, ref, top_n)
                assert np.array_equal(ids, out[0][0]) and np.array_equal(s, out[0][1])
    finally:
        m.close()


# 3. symmetry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [32, 65])
def test_symmetry(hip, V):
    """All pairs of a small vocabulary, exclude_self=False and top_n = V (32: the wide tile, 65: the
    narrow one): s(q, w) from querying q equals s(w, q) from querying w, bitwise."""
    K = 37
    lam = _lam(K, V, seed=77 + V)
    m = _model(K, V, lam)
    try:
        for measure in MEASURES:
            for pi in (None, _given(K)):
                ids, s = m.similar_words(np.arange(V), V, measure=measure, topic_weights=pi, exclude_self=False,
                                         return_similarity=True)
                S = np.full((V, V), np.nan)
                for q in range(V):
                    assert sorted(ids[q]) == list(range(V))
                    S[q, ids[q]] = s[q]
                assert np.array_equal(S, S.T)
                assert float(np.max(np.abs(np.diag(S) - 1.0))) <= wh.sim_bound(K, measure, V=V, given=pi is not None)
    finally:
        m.close()


# 4. exact ties ---------------------------------------------------------------------------------------
def test_exact_ties(hip):
    """A planted copy of a column ties with its original bitwise against every query and ranks by id,
    also across a slab boundary (slab 48: words 40 and 1000 lie in slabs 0 and 20).  A column
    multiplied by 4 gives the same p(k | w) and the same bits of s against every query under both
    measures, because every step scales exactly by a power of two: a = c lambda (x 4), sqrt(a) (x 2),
    the sums of a (x 4) and of a^2 (x 16), their roots (x 2, x 4) and reciprocals, every product of
    the chain (x 2 or x 4) -- and the two factors cancel exactly in d (z_q z_w)."""
    K, V = 33, 2100
    lam = _lam(K, V)
    src, dup, quad = 40, 1000, 1500
    lam[:, dup] = lam[:, src]
    lam[:, quad] = 4.0 * lam[:, src]
    m = _model(K, V, lam)
    try:
        for measure in MEASURES:
            for pi in (None, _given(K)):
                bound = wh.sim_bound(K, measure, V=V, given=pi is not None)
                rows = wh.rows(lam, measure, pi)
                near = wh.search(rows[[src]], rows, 8, self_ids=[src])[0][0]
                queries = np.array([src, dup, quad] + [int(w) for w in near if w not in (dup, quad)][:4])
                for slab, top_n in ((48, 20), (48, 100), (0, 100)):    # (both widths of the query kernel)
                    _slab(hip, m, slab)
                    ids, s = m.similar_words(queries, top_n, measure=measure, topic_weights=pi,
                                             return_similarity=True)
                    # the three equal points see each other first, at s = 1 within the bound, in id order
                    assert list(ids[0][:2]) == [dup, quad] and list(ids[1][:2]) == [src, quad]
                    assert list(ids[2][:2]) == [src, dup]
                    assert float(np.max(np.abs(s[:3, :2] - 1.0))) <= bound
                    assert np.array_equal(s[0, 2:], s[1, 2:]) and np.array_equal(ids[0, 2:], ids[1, 2:])
                    assert np.array_equal(s[0, 2:], s[2, 2:]) and np.array_equal(ids[0, 2:], ids[2, 2:])
                    # in the other queries' lists the three tie bitwise and stand together in id order
                    found = 0
                    for b in range(3, len(queries)):
                        row = list(ids[b])
                        if src in row[:top_n - 2]:
                            i = row.index(src)
                            assert row[i:i + 3] == [src, dup, quad] and s[b, i] == s[b, i + 1] == s[b, i + 2]
                            found += 1
                        else:
                            assert dup not in row[:top_n - 2] and quad not in row[:top_n - 2]
                    assert found >= 1 or top_n < 100
                _slab(hip, m, 0)
                p = m.word_topic_proportions([src, dup, quad], topic_weights=pi)
                assert np.array_equal(p[:, 0], p[:, 1]) and np.array_equal(p[:, 0], p[:, 2])
    finally:
        m.close()


# 5. the weights --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,V", [(3, 300), (100, 300), (513, 65)])
def test_default_weights_give_the_normalised_column(hip, K, V):
    """topic_weights=None: c_k is 1 / sum(lambda) for every k (up to 2 u), so p(k | w) is the
    normalised column of lambda; each column sums to 1.  With given weights p follows the
    restatement."""
    lam = _lam(K, V)
    words = _queries(K, V, 20)
    m = _model(K, V, lam)
    try:
        p = m.word_topic_proportions(words)
        assert p.dtype == np.float64 and p.shape == (K, 20) and p.flags.f_contiguous
        col = lam[:, words].astype(LD)
        want = col / col.sum(axis=0)
        bound = wh.prop_bound(K, given=False)
        err = float(np.max(np.abs(p.astype(LD) - want) / want))
        print("K = %d default: p rel err %.1f u (bound %.0f u)" % (K, err / U, bound / U))
        assert err <= bound
        assert float(np.max(np.abs(p.astype(LD).sum(axis=0) - 1))) <= bound + K * 2.0 ** -64
        pi = _given(K)
        p = m.word_topic_proportions(words, topic_weights=pi)
        want = wh.proportions(lam, pi, words)
        err = float(np.max(np.abs(p.astype(LD) - want) / want))
        assert err <= wh.prop_bound(K, V=V)
        assert np.array_equal(m.word_topic_proportions(int(words[3]), topic_weights=pi)[:, 0], p[:, 3])
    finally:
        m.close()


def test_given_weights_change_the_answer(hip):
    """Two topics; word 0 lies mostly in topic 0, candidate 1 is topic 0's alone, candidate 2 is even.
    Weights on topic 0 make 1 the nearer, weights on topic 1 pull word 0 to the even side and make 2
    the nearer (tests/test_wordsim_host.py has the same case on the restatement)."""
    lam = np.array([[8.0, 9.0, 1.0], [1.0, 0.01, 1.0]])
    m = _model(2, 3, lam)
    try:
        for measure in MEASURES:
            first = {}
            for name, w in (("zero", [100.0, 1.0]), ("one", [1.0, 100.0])):
                ref = Ref(lam, np.array(w), measure, np.array([0]))
                _, ids, _ = _check(m, ref, 2)
                first[name] = int(ids[0, 0])
            assert first == {"zero": 1, "one": 2}
    finally:
        m.close()


@pytest.mark.parametrize("K", [5, 100, 513])
def test_words_near_is_consistent_with_similar_words(hip, K):
    """words_near(p) with p = word_topic_proportions([q]) ranks as similar_words([q],
    exclude_self=False) does; the two paths round differently (p is rounded, normalised again and
    rooted), so s agrees within 2 sim_bound and the ids under the gap condition."""
    V, B, top_n = 300, 9, 20
    lam = _lam(K, V)
    queries = _queries(K, V, B)
    m = _model(K, V, lam)
    try:
        for measure in MEASURES:
            for pi in (None, _given(K)):
                ref = Ref(lam, pi, measure, queries)
                want_ids, want_s, gap = ref.search(top_n, exclude_self=False)
                assert gap > GAP_FLOOR
                p = m.word_topic_proportions(queries, topic_weights=pi)
                ids, s = m.words_near(p, top_n, measure=measure, topic_weights=pi, return_similarity=True)
                ids2, s2 = m.similar_words(queries, top_n, measure=measure, topic_weights=pi, exclude_self=False,
                                           return_similarity=True)
                assert np.array_equal(ids, ids2) and np.array_equal(ids, want_ids)
                assert float(np.max(np.abs(s - s2) / s2)) <= 2 * ref.bound
                one, d1 = m.words_near(p[:, 4], top_n, measure=measure, topic_weights=pi)
                assert one.shape == (1, top_n) and np.array_equal(one[0], ids[4])
                assert np.array_equal(d1[0], wh.distance(s[4], measure))
        # any positive scale of the proportions gives the same point
        a = m.words_near(3.0 * p, 5, return_similarity=True)
        b = m.words_near(p, 5, return_similarity=True)
        assert np.array_equal(a[0], b[0]) and float(np.max(np.abs(a[1] - b[1]))) <= 2 * wh.sim_bound(K, "hellinger", V=V)
    finally:
        m.close()


# 6. state --------------------------------------------------------------------------------------------
def _draw_state():
    from trlda_amd import _ffi
    k = C.c_uint64(0)
    _ffi.check(_ffi.lib().trlda_rng_draw_key(C.byref(k)))
    return k.value


def _docs(V, n, seed):
    rng = np.random.RandomState(seed)
    return [[(int(rng.randint(V)), int(rng.randint(1, 5))) for _ in range(rng.randint(1, 14))] for _ in range(n)]


@pytest.mark.parametrize("deferred", [False, True])
def test_state_is_left_alone(hip, deferred):
    """Two calls agree bitwise; lambda, alpha, eta, update_count, the model's statistics and the seeded
    stream stay where they were; VI E-steps before and after the calls give the bits they give
    without them, also with deferred statistics and two stream lanes on (which the calls settle)."""
    import trlda_amd
    from trlda_amd import _ffi
    K, V, B = 16, 120, 9
    lam = _lam(K, V)
    docs, other = _docs(V, B, 5), _docs(V, B, 6)
    rng = np.random.RandomState(21)
    g0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)
    g1 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)
    given = _given(K)

    def calls(m):
        return (m.similar_words([3, 7, 119], 10, return_similarity=True),
                m.similar_words([5], 7, measure="cosine", topic_weights=given),
                m.words_near(g1, 5, measure="cosine"), m.words_near(g1[:, 0], 100, topic_weights=given),
                (m.word_topic_proportions([0, 1, 2], topic_weights=given),))

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
            want = _draw_state()
            trlda_amd.seed(9)
            a = calls(m)
            assert _draw_state() == want                              # nothing was drawn
            b = calls(m)
            for x, y in zip(a, b):
                for u, v in zip(x, y):
                    assert np.array_equal(u, v)
            after = np.empty((K, V), order="F")
            _ffi.check(hip.trlda_model_get_sstats(m._handle, after))
            assert np.array_equal(held, after) and np.array_equal(held, out[0][1])   # no E-step ran
            assert np.array_equal(np.asarray(m.lambdas), before[0])
            assert np.array_equal(np.asarray(m.alpha), before[1])
            assert m.eta == before[2] and m.update_count == before[3]
        out.append(m.update_variables(other, latents=g1, max_iter=20))
        m.close()
        return out

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


# 7. errors -------------------------------------------------------------------------------------------
def _made():
    from trlda_amd import _ffi
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return total.value


def test_errors_come_before_anything_is_allocated(hip):
    from trlda_amd import _ffi
    K, V, B = 8, 40, 4
    m = _model(K, V, _lam(K, V))
    ids = np.array([0, 5, 39, 7], dtype=np.int32)
    props = np.asfortranarray(np.ones((K, B)))
    w = np.full((B, 101), -7, dtype=np.int32)
    s = np.full((max(B, K), 101), -7.)
    h = m._handle

    def similar(handle=h, ids=ids, B=B, top_n=5, measure=0, pi=None, exclude=1, wo=w, so=s):
        return hip.trlda_model_similar_words(handle, None if ids is None else ids.ctypes.data, B, top_n, measure,
                                             None if pi is None else pi.ctypes.data, exclude,
                                             None if wo is None else wo.ctypes.data,
                                             None if so is None else so.ctypes.data)

    def near(handle=h, props=props, B=B, top_n=5, measure=0, pi=None, wo=w, so=s):
        return hip.trlda_model_similar_words_rows(handle, None if props is None else props.ctypes.data, B, top_n,
                                                  measure, None if pi is None else pi.ctypes.data,
                                                  None if wo is None else wo.ctypes.data,
                                                  None if so is None else so.ctypes.data)

    def topics(handle=h, ids=ids, B=B, pi=None, out=s):
        return hip.trlda_model_word_topic_proportions(handle, None if ids is None else ids.ctypes.data, B,
                                                      None if pi is None else pi.ctypes.data,
                                                      None if out is None else out.ctypes.data)

    bad_pi = [np.r_[np.ones(K - 1), 0.0], np.r_[np.ones(K - 1), -1.0], np.r_[np.ones(K - 1), np.nan],
              np.r_[np.ones(K - 1), np.inf]]
    try:
        made = _made()
        # TRLDA_ERR_ARG
        assert similar(handle=None) == near(handle=None) == topics(handle=None) == _ffi.ERR_ARG
        assert similar(wo=None) == similar(so=None) == near(wo=None) == near(so=None) == _ffi.ERR_ARG
        assert topics(out=None) == _ffi.ERR_ARG
        assert similar(B=-1) == near(B=-1) == topics(B=-1) == _ffi.ERR_ARG
        for top_n in (0, -1, 101, V + 1):
            assert similar(top_n=top_n) == near(top_n=top_n) == similar(top_n=top_n, exclude=0) == _ffi.ERR_ARG
        assert similar(top_n=V) == _ffi.ERR_ARG                       # V - 1 candidates without the word itself
        for measure in (-1, 2):
            assert similar(measure=measure) == near(measure=measure) == _ffi.ERR_ARG
        for pi in bad_pi:
            assert similar(pi=pi) == near(pi=pi) == topics(pi=pi) == _ffi.ERR_ARG
            for call in (lambda: m.similar_words(ids, topic_weights=pi), lambda: m.words_near(props, topic_weights=pi),
                         lambda: m.word_topic_proportions(ids, topic_weights=pi)):
                with pytest.raises(RuntimeError, match="topic_weights"):
                    call()
        # the order: a bad top_n or weight is named before a bad id, a bad id before bad proportions
        wrong = np.array([0, V, 3, 1], dtype=np.int32)
        assert similar(ids=wrong, top_n=0) == _ffi.ERR_ARG and similar(ids=wrong, pi=bad_pi[0]) == _ffi.ERR_ARG
        # the word ids
        for bad in (V, -1, 2 ** 31 - 1):
            wrong = np.array([0, 1, bad, 3], dtype=np.int32)
            assert similar(ids=wrong) == topics(ids=wrong) == _ffi.ERR_WORD_ID
            with pytest.raises(RuntimeError, match="[Ww]ord id"):
                m.similar_words(wrong)
        # the proportions
        for bad in (0.0, -1.0, np.nan, np.inf):
            spoiled = props.copy(order="F")
            spoiled[K - 1, B - 1] = bad
            assert near(props=spoiled) == _ffi.ERR_VALUE
            with pytest.raises(RuntimeError, match="finite and positive"):
                m.words_near(spoiled)
        with pytest.raises(RuntimeError, match="top_n"):
            m.similar_words(ids, V)
        assert hip.trlda_model_set_wordsim_slab_words(h, 24) == _ffi.ERR_ARG
        assert hip.trlda_model_set_wordsim_slab_words(h, -16) == _ffi.ERR_ARG
        assert _made() == made                                        # no buffer was made for any of them
        assert np.all(w == -7) and np.all(s == -7.)
        # B = 0 writes nothing and succeeds
        assert similar(B=0) == near(B=0) == topics(B=0) == _ffi.OK
        assert np.all(w == -7) and np.all(s == -7.) and _made() == made
        # the model still works after the refusals: top_n = V without the exclusion lists every word
        words, _ = m.similar_words(ids, V, exclude_self=False)
        assert np.array_equal(np.sort(words, axis=1), np.tile(np.arange(V), (B, 1)))
        words, _ = m.similar_words(ids, V - 1)
        for b in range(B):
            assert sorted(words[b]) == [x for x in range(V) if x != ids[b]]
    finally:
        m.close()


@pytest.mark.parametrize("planted", [0.0, float("nan"), -1.0, float("inf")])
def test_a_bad_lambda_is_refused(hip, planted):
    from trlda_amd import _ffi
    K, V = 70, 1100
    lam = _lam(K, V)
    lam[66, 1050] = planted
    m = _model(K, V, lam)
    ids = np.array([3, 4], dtype=np.int32)
    props = np.asfortranarray(np.ones((K, 2)))
    w = np.full((2, 10), -7, dtype=np.int32)
    s = np.full((K, 10), -7.)
    try:
        for call in (lambda: m.similar_words([3, 4]), lambda: m.similar_words([3], measure="cosine"),
                     lambda: m.words_near(props), lambda: m.word_topic_proportions([3, 4]),
                     lambda: m.similar_words([3], topic_weights=_given(K))):
            with pytest.raises(RuntimeError, match="positive, finite lambda"):
                call()
        for measure in (0, 1):
            assert hip.trlda_model_similar_words(m._handle, ids.ctypes.data, 2, 10, measure, None, 1, w.ctypes.data,
                                                 s.ctypes.data) == _ffi.ERR_VALUE
            assert hip.trlda_model_similar_words_rows(m._handle, props.ctypes.data, 2, 10, measure, None,
                                                      w.ctypes.data, s.ctypes.data) == _ffi.ERR_VALUE
        assert hip.trlda_model_word_topic_proportions(m._handle, ids.ctypes.data, 2, None,
                                                      s.ctypes.data) == _ffi.ERR_VALUE
        assert np.all(w == -7) and np.all(s == -7.)                   # nothing was written
        m.lambdas = _lam(K, V)                                        # a good lambda again: the flag is per call
        assert m.similar_words([3, 4])[0].shape == (2, 10)
    finally:
        m.close()


# 8. buffers ------------------------------------------------------------------------------------------
def test_no_buffer_is_left_after_close(hip):
    """A fresh process (the count is the process's): every workspace of the three calls; after close()
    the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wordsim_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout
