"""LDA.relevant_words / word_statistics / salient_words / topic_prevalence on the GPU
(csrc/relevance_kernels.h) against the longdouble restatement
(tests/relevance_host.py): ids exactly, values within first-order bounds, vocabulary edges, exact
ties across tiles, weight = 1 against top_words, the prevalence and its independence of the
batching, the model's state, the errors and the buffers.

Every array is small: at most 2100 words, 33 documents and 2276 topics (never all at once)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import relevance_host as vh

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GAP_FLOOR = 1e-9                         # absolute for r (a log scale), relative for S
TOPS = (1, 10, 33, 100)
WEIGHTS = (1.0, 0.6, 0.3, 0.0)
LD = np.longdouble


def p_bound(K, V):
    """|p_dev - p| / p, first order.  Default weights: c_k = fl(fl(R_k / S) / R_k) is 1 / S with the
    error of S (V - 1 additions per row sum, K - 1 over the rows) and two divisions, R_k's own error
    cancelling; given weights: c_k = pi_k / R_k carries pi's rounding, R_k's V - 1 additions and a
    division.  Then K products and K - 1 additions, every term positive: at most (V + 2 K) u either
    way; (V + 2 K + 8) u."""
    return (V + 2 * K + 8) * U


def r_bound(K, V, L):
    """|r_dev - r|, absolute, first order; L bounds |log lambda|, |log R|, |log p| and |r|.  log R_k:
    (V - 1) u from the row sum and an ulp (2 u L) of the device log; log lambda: an ulp; (1 - l) log p:
    p_bound and an ulp of log p, the rounding of 1 - l and of the product (2 u L); two subtractions
    (u L each): (V - 1) + (V + 2 K + 8) + 10 L, rounded up to (2 V + 2 K + 7 + 12 L) u."""
    return (2 * V + 2 * K + 7 + 12 * L) * U


def d_bound(K, V, scale, Lpi):
    """|D_dev - D|, absolute, first order, per word; scale = sum_k |q (log q - log pi)| from the
    restatement, Lpi = max |log pi|.  With q~ = q (1 + d_k) and log pi~ = log pi + e_k the error of
    sum_k q~ (log q~ - log pi~) is sum_k q d_k (log q - log pi) + sum_k q (d_k - e_k) + the device
    logs' ulps (2 u sum_k q (|log q| + |log pi|) <= 2 u (log K + Lpi), q being a distribution) + the
    subtraction, the product and the K - 1 additions ((K + 1) u scale).  Default weights: the common
    factor 1 / S cancels in q, |d_k| <= (K + 6) u, and |e_k| <= (2 V + K - 2) u (R_k, S, a division);
    given weights: |d_k| <= (2 V + K + 4) u (c_k: V + 1; p: V + K + 1; a product and a division) and
    pi's rounding is the same in q~ and pi~, |d_k - e_k| <= (2 V + K + 3) u.  The second sum does not
    scale with D: it stays when the word is not distinctive.  Both cases lie within
    ((2 V + 2 K + 7) scale + (2 V + 2 K + 4) + 2 (log K + Lpi)) u."""
    return ((2 * V + 2 * K + 7) * scale + (2 * V + 2 * K + 4) + 2 * (np.log(max(K, 2)) + Lpi)) * U


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


def _given(K):
    """The given topic weights.  The seed 100002 + K was chosen on the CPU so that the input condition
    holds for every K, weight and top_n of this file (RandomState(K) gave a relevance gap of 6e-11 at
    K = 2276, weight 0); smallest relevance gap with it 2.5e-8 (K = 2276, weight 0.6)."""
    return np.random.RandomState(100002 + K).gamma(0.5, 1.0, K) + 0.01


class Ref(object):
    """The restatement of one (lambda, weights), computed once and shared."""

    def __init__(self, lam, given=None):
        self.lam, self.given = lam, given
        self.K, self.V = lam.shape
        self.pi, self.R = vh.weights(lam, given)
        self.p, self.D, self.S, self.scale = vh.word_statistics(lam, given)
        self.r = {}
        logs = [np.log(lam.astype(LD)), np.log(self.R), np.log(self.p), self.relevance(0.0)]
        self.L = float(max(np.abs(x).max() for x in logs))
        self.Lpi = float(np.abs(np.log(self.pi)).max())

    def relevance(self, weight):
        if weight not in self.r:
            self.r[weight] = vh.relevance(self.lam, weight, self.given)
        return self.r[weight]

    def rows(self, weight, top_n):
        r = self.relevance(weight)
        out = [vh.rank(r[k], top_n, relative=False) for k in range(self.K)]
        return np.stack([x[0] for x in out]), np.stack([x[1] for x in out]), min(x[2] for x in out)


def _check_relevance(m, ref, weight, top_n, tied=False):
    """ids exactly, scores within r_bound; the input condition first.  Returns the worst error."""
    K, V = ref.K, ref.V
    want_w, want_r, gap = ref.rows(weight, top_n)
    if not tied:
        assert gap > GAP_FLOOR, (K, V, weight, top_n, gap)
    pi = None if ref.given is None else ref.given
    words, scores = m.relevant_words(top_n, weight, topic_weights=pi, return_scores=True)
    assert words.dtype == np.int32 and scores.dtype == np.float64 and words.shape == scores.shape == (K, top_n)
    assert np.array_equal(words, m.relevant_words(top_n, weight, topic_weights=pi))
    assert np.array_equal(words, want_w), (K, V, weight, top_n)
    err = float(np.max(np.abs(scores.astype(LD) - want_r)))
    assert err <= r_bound(K, V, ref.L), (K, V, weight, top_n, err / U)
    return err


def _check_statistics(m, ref):
    """p, D, S within their bounds; returns the worst errors in u (p relative, D absolute)."""
    K, V = ref.K, ref.V
    p, D, S = m.word_statistics(topic_weights=ref.given)
    for x in (p, D, S):
        assert x.dtype == np.float64 and x.shape == (V,)
    ep = float(np.max(np.abs(p.astype(LD) - ref.p) / ref.p))
    assert ep <= p_bound(K, V), (K, V, ep / U)
    db = d_bound(K, V, ref.scale, ref.Lpi)
    ed = np.abs(D.astype(LD) - ref.D)
    assert np.all(ed <= db), (K, V, float(np.max(ed / db)))
    es = np.abs(S.astype(LD) - ref.S)
    assert np.all(es <= ref.p * db + ref.S * (p_bound(K, V) + U)), (K, V)
    return ep, float(ed.max()), float(np.max(ed / db))


def _check_salient(m, ref, top_n, tied=False):
    K, V = ref.K, ref.V
    want_w, want_s, gap = vh.rank(ref.S, top_n, relative=True)
    if not tied:
        assert gap > GAP_FLOOR, (K, V, top_n, gap)
    words, sal = m.salient_words(top_n, topic_weights=ref.given)
    assert words.dtype == np.int32 and sal.dtype == np.float64 and words.shape == sal.shape == (top_n,)
    assert np.array_equal(words, want_w), (K, V, top_n)
    db = d_bound(K, V, ref.scale, ref.Lpi)
    bound = (ref.p * db + ref.S * (p_bound(K, V) + U))[want_w]
    assert np.all(np.abs(sal.astype(LD) - want_s) <= bound), (K, V, top_n)
    return words, sal


# 1. ids and scores -----------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("K", [1, 3, 64, 65, 100, 513, 2276])
def test_ids_and_scores(hip, K, given):
    """V = 300, top_n in 1, 10, 33, 100, weight in 1, 0.6, 0.3, 0, default and given weights.  The
    inputs have no near ties: the restatement's smallest gap among the first top_n + 1 of every row
    stays above GAP_FLOOR (absolute for r, relative for S) in every case -- checked on the CPU when
    the given weights' seeds were chosen (smallest relevance gap 6.8e-9, default weights, K = 2276,
    weight 0; smallest relative saliency gap 6e-7), asserted here first, so no case is left out of
    the id comparison.  K = 1 has lift 1 for every word, r = weight log beta: at weight 0 its r is one
    exact tie (every r is 0), where the scores must be finite and equal within the bound and the ids
    in the order of what the device computed; at weights 0.6 and 0.3 its gaps (8.9e-6, 4.5e-6) pass
    the condition like any other case and the ids are compared.  Its saliency is exactly 0."""
    V = 300
    lam = _lam(K, V)
    ref = Ref(lam, _given(K) if given else None)
    # three orders between what the device may be off by and what the ids need
    assert r_bound(K, V, ref.L) <= 1e-3 * GAP_FLOOR and p_bound(K, V) <= 1e-3 * GAP_FLOOR
    assert float(np.max(d_bound(K, V, ref.scale, ref.Lpi))) <= 1e-3 * GAP_FLOOR
    m = _model(K, V, lam)
    try:
        worst = 0.0
        for weight in WEIGHTS:
            for top_n in TOPS:
                if K == 1 and weight == 0.0:
                    words, scores = m.relevant_words(top_n, weight, topic_weights=ref.given, return_scores=True)
                    assert words.shape == (1, top_n) and len(set(words[0])) == top_n
                    assert np.all((words >= 0) & (words < V)) and np.all(np.isfinite(scores))
                    want = ref.relevance(weight)[0][words[0]]
                    err = float(np.max(np.abs(scores[0].astype(LD) - want)))
                    assert err <= r_bound(K, V, ref.L)
                    assert np.ptp(scores) <= 2 * r_bound(K, V, ref.L)
                    # (ranked by what the device computed: larger first, equal values by smaller id)
                    assert np.all(np.diff(scores[0]) <= 0)
                    same = np.diff(scores[0]) == 0
                    assert np.all(np.diff(words[0])[same] > 0)
                else:
                    err = _check_relevance(m, ref, weight, top_n)
                worst = max(worst, err)
        ep, ed, frac = _check_statistics(m, ref)
        for top_n in TOPS:
            words, sal = _check_salient(m, ref, top_n, tied=K == 1)
            if K == 1:
                assert np.array_equal(words, np.arange(top_n)) and np.all(sal == 0.0)
        print("K = %d %s: r err %.1f u (bound %.0f u); p rel err %.1f u (bound %d u); D err %.1f u, "
              "%.3f of its bound (largest bound %.0f u)"
              % (K, "given" if given else "default", worst / U, r_bound(K, V, ref.L) / U, ep / U, V + 2 * K + 8,
                 ed / U, frac, float(np.max(d_bound(K, V, ref.scale, ref.Lpi))) / U))
    finally:
        m.close()


# 2. vocabulary edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 100])
@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 1023, 1024, 1025])
def test_vocabulary_edges(hip, K, V):
    """A single word, below / at / past a group of 64, below / at / past one tile of 1024; top_n
    clipped to V.  (V = 1: p = 1 and every r and S is 0 up to rounding -- one row of one word.)"""
    lam = _lam(K, V)
    ref = Ref(lam)
    m = _model(K, V, lam)
    try:
        for top_n in sorted({min(t, V) for t in TOPS}):
            for weight in (1.0, 0.6, 0.0):
                _check_relevance(m, ref, weight, top_n)
            _check_salient(m, ref, top_n, tied=V == 1)
        _check_statistics(m, ref)
    finally:
        m.close()


# 3. exact ties ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 70])
def test_exact_ties_across_tiles(hip, K):
    """V = 2100 (three tiles).  The columns of the best words of topic 0 and of the most salient words
    are copied to other ids, some in other tiles: equal r in every topic and equal S, bitwise; the
    tied ids come out in id order; everything matches the restatement, which ties them exactly too
    (identical columns give identical longdouble values).  The gap condition is asserted on the same
    lambda without the planted ties."""
    V, top_n = 2100, 33
    base = _lam(K, V)
    clean = Ref(base)
    for weight in (0.6, 0.0):
        assert clean.rows(weight, top_n)[2] > GAP_FLOOR
    assert vh.rank(clean.S, top_n, relative=True)[2] > GAP_FLOOR
    src = [int(w) for w in clean.rows(0.6, 4)[0][0]]
    src += [int(w) for w in vh.rank(clean.S, 7, relative=True)[0] if int(w) not in src][:3]
    dst = [1030, 7, 2099, 1023, 1024, 2048, 64]          # (other tiles, tile borders, a group border)
    lam = base.copy()
    taken = set(int(s) for s in src)
    pairs = []
    for s, d in zip(src, dst):
        assert d not in taken
        lam[:, d] = lam[:, int(s)]
        pairs.append((int(s), d))
    ref = Ref(lam)
    m = _model(K, V, lam)
    try:
        for weight in (0.6, 0.0):
            _check_relevance(m, ref, weight, top_n, tied=True)
            words, scores = m.relevant_words(top_n, weight, return_scores=True)
            row = list(words[0])
            for s, d in pairs[:4]:
                if weight == 0.6:                                     # (the list's own best words)
                    assert s in row and d in row
                if max(s, d) in row:
                    i, j = row.index(min(s, d)), row.index(max(s, d))
                    assert j == i + 1 and scores[0, i] == scores[0, j]
        words, sal = _check_salient(m, ref, top_n, tied=True)
        row = list(words)
        for s, d in pairs[4:]:
            i, j = row.index(min(s, d)), row.index(max(s, d))
            assert j == i + 1 and sal[i] == sal[j]
        p, D, S = m.word_statistics()
        for s, d in pairs:
            assert p[s] == p[d] and D[s] == D[d] and S[s] == S[d]
    finally:
        m.close()


# 4. weight = 1 against top_words ---------------------------------------------------------------------
@pytest.mark.parametrize("K,V", [(3, 300), (100, 300), (513, 300), (5, 1025)])
def test_weight_one_is_top_words(hip, K, V):
    lam = _lam(K, V)
    m = _model(K, V, lam)
    try:
        for top_n in (1, 10, 100):
            assert np.array_equal(m.relevant_words(top_n, 1.0), m.top_words(top_n))
            assert np.array_equal(m.relevant_words(top_n, 1.0, topic_weights=_given(K)), m.top_words(top_n))
    finally:
        m.close()


# 5. prevalence ---------------------------------------------------------------------------------------
def _docs(V, n, seed, negative=False):
    """n documents as lists: document 1 empty, document 2 with counts <= 0 only (a negative one only
    where no E-step sees it), repeated ids and counts of 0 among the others."""
    rng = np.random.RandomState(seed)
    docs = [[(int(rng.randint(V)), int(rng.randint(0, 5))) for _ in range(rng.randint(1, 14))] for _ in range(n)]
    docs[0] = [(3 % V, 2), (3 % V, 1), (1 % V, 4)]
    if n > 2:
        docs[1] = []
        docs[2] = [(2 % V, 0), (5 % V, -3 if negative else 0)]
    return docs


def _gammas(K, n, seed):
    rng = np.random.RandomState(seed)
    g = rng.gamma(0.3, 1.0, size=(K, n)) + 0.01
    return np.asfortranarray(g * rng.uniform(0.5, 40.0, size=n))


@pytest.mark.parametrize("K", [3, 100, 513])
def test_prevalence_gamma(hip, K):
    """B = 33 against the restatement to (B + K + 8) u relative -- K - 1 additions and a division per
    document, two products, B - 1 additions per topic, the normalisation in long double --; bitwise the
    same for one batch of 33, for 17 + 16 and for 33 batches of one, with both weight_by_length."""
    from trlda_amd import _ffi
    V, B = 120, 33
    docs, g = _docs(V, B, 40 + K, negative=True), _gammas(K, B, 50 + K)
    counted = sum(1 for d in docs if sum(c for _, c in d if c > 0) > 0)
    assert counted <= B - 2
    m = _model(K, V, _lam(K, V))
    try:
        for by_length in (True, False):
            pi = m.topic_prevalence_gamma(g, docs, weight_by_length=by_length)
            want = vh.prevalence(g, docs, by_length)
            assert pi.dtype == np.float64 and pi.shape == (K,)
            err = float(np.max(np.abs(pi.astype(LD) - want) / want))
            print("K = %d by_length = %s: rel err %.2f u (bound %d u)" % (K, by_length, err / U, B + K + 8))
            assert err <= (B + K + 8) * U
            for cuts in ((0, 17, 33), tuple(range(B + 1))):
                acc = _ffi.vp()
                _ffi.check(hip.trlda_prevalence_create(m._handle, int(by_length), C.byref(acc)))
                try:
                    for lo, hi in zip(cuts[:-1], cuts[1:]):
                        batch = m.upload(docs[lo:hi])
                        part = np.asfortranarray(g[:, lo:hi])
                        ptr = _ffi.vp()
                        _ffi.check(hip.trlda_dev_alloc(0, part.nbytes, C.byref(ptr)))
                        try:
                            _ffi.check(hip.trlda_dev_upload(0, ptr, part.ctypes.data, part.nbytes))
                            _ffi.check(hip.trlda_prevalence_add_dev(acc, batch.handle, ptr))
                            _ffi.check(hip.trlda_model_synchronize(m._handle))
                        finally:
                            hip.trlda_dev_free(0, ptr)
                            batch.close()
                    got = np.empty(K)
                    n = C.c_int64(0)
                    _ffi.check(hip.trlda_prevalence_read(acc, got.ctypes.data, C.byref(n)))
                finally:
                    hip.trlda_prevalence_destroy(acc)
                assert n.value == counted and np.array_equal(got, pi), (K, by_length, len(cuts))
    finally:
        m.close()


def test_prevalence_through_the_estep(hip):
    """topic_prevalence(docs, latents=g0, max_iter=20) is bitwise the gamma form on update_variables'
    gamma; a list, an uploaded batch and an iterator of one batch agree; fed into relevant_words the
    weights give the restatement's lists for the same weights."""
    K, V, B = 20, 300, 33
    lam = _lam(K, V)
    docs = _docs(V, B, 77)
    g0 = np.asfortranarray(np.random.RandomState(3).gamma(1.0, 1.0, size=(K, B)) + 0.1)
    m = _model(K, V, lam)
    try:
        gamma, _ = m.update_variables(docs, latents=g0, max_iter=20)
        for by_length in (True, False):
            want = m.topic_prevalence_gamma(gamma, docs, weight_by_length=by_length)
            pi = m.topic_prevalence(docs, latents=g0, max_iter=20, weight_by_length=by_length)
            assert np.array_equal(pi, want)
            batch = m.upload(docs)
            assert np.array_equal(m.topic_prevalence(batch, latents=g0, max_iter=20, weight_by_length=by_length), want)
            assert np.array_equal(m.topic_prevalence(iter([batch]), latents=g0, max_iter=20,
                                                     weight_by_length=by_length), want)
            batch.close()
            assert abs(pi.sum() - 1.0) <= 4 * U and np.all(pi > 0)
        # an iterator of several batches: each document's gamma does not depend on its batch
        parts = iter([docs[:17], docs[17:]])
        cut = m.topic_prevalence(parts, latents=g0, max_iter=20)
        pi = m.topic_prevalence(docs, latents=g0, max_iter=20)
        assert np.max(np.abs(cut - pi) / pi) <= 1e-12                 # (the E-step's launch may differ by batch)
        ref = Ref(lam, pi)
        for weight in (0.6, 0.0):
            _check_relevance(m, ref, weight, 10)
        _check_statistics(m, ref)
    finally:
        m.close()


# 6. state and forms ----------------------------------------------------------------------------------
def _draw_state():
    from trlda_amd import _ffi
    k = C.c_uint64(0)
    _ffi.check(_ffi.lib().trlda_rng_draw_key(C.byref(k)))
    return k.value


@pytest.mark.parametrize("deferred", [False, True])
def test_state_is_left_alone(hip, deferred):
    """Two calls agree bitwise; lambda, alpha, eta, update_count, the model's statistics and the seeded
    stream stay where they were; VI E-steps before and after the calls give the bits they give
    without them, also with deferred statistics and two stream lanes on."""
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
        return (m.relevant_words(10, 0.6, return_scores=True), m.relevant_words(7, 0.3, topic_weights=given),
                m.word_statistics(), m.salient_words(30, topic_weights=given),
                m.topic_prevalence_gamma(g1, other))

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
                for u, v in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)):
                    assert np.array_equal(u, v)
            after = np.empty((K, V), order="F")
            _ffi.check(hip.trlda_model_get_sstats(m._handle, after))
            assert np.array_equal(held, after) and np.array_equal(held, out[0][1])   # no E-step ran
            trlda_amd.seed(9)
            m.topic_prevalence(other, latents=g1, max_iter=20)        # an E-step from given latents: no draw
            assert _draw_state() == want
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
def _live():
    from trlda_amd import _ffi
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return total.value


def test_errors_come_before_anything_is_allocated(hip):
    from trlda_amd import _ffi
    from trlda_amd.documents import DeviceBatch
    K, V, B = 8, 40, 4
    lam = _lam(K, V)
    m = _model(K, V, lam)
    other = DeviceBatch(_docs(V, B, 7), V + 1, 0)
    w = np.full((K, 101), -7, dtype=np.int32)
    s = np.full((K, 101), -7.)
    bad_pi = [np.ones(K + 1), np.ones(K - 1), np.r_[np.ones(K - 1), 0.0], np.r_[np.ones(K - 1), -1.0],
              np.r_[np.ones(K - 1), np.nan], np.r_[np.ones(K - 1), np.inf]]
    try:
        made = _live()
        for top_n in (0, -1, V + 1, 101):
            with pytest.raises(RuntimeError, match="top_n"):
                m.relevant_words(top_n)
            with pytest.raises(RuntimeError, match="top_n"):
                m.salient_words(top_n)
            assert hip.trlda_model_relevant_words(m._handle, top_n, 0.6, None, w.ctypes.data, s.ctypes.data) \
                == _ffi.ERR_ARG
            assert hip.trlda_model_salient_words(m._handle, top_n, None, w.ctypes.data, s.ctypes.data) == _ffi.ERR_ARG
        for weight in (-0.01, 1.01, float("nan"), float("inf")):
            with pytest.raises(RuntimeError, match="weight"):
                m.relevant_words(5, weight)
            assert hip.trlda_model_relevant_words(m._handle, 5, weight, None, w.ctypes.data, s.ctypes.data) \
                == _ffi.ERR_ARG
        for pi in bad_pi:
            for call in (lambda: m.relevant_words(5, topic_weights=pi), lambda: m.word_statistics(topic_weights=pi),
                         lambda: m.salient_words(5, topic_weights=pi)):
                with pytest.raises(RuntimeError, match="topic_weights"):
                    call()
            if pi.size == K:
                assert hip.trlda_model_relevant_words(m._handle, 5, 0.6, pi.ctypes.data, w.ctypes.data,
                                                      s.ctypes.data) == _ffi.ERR_ARG
                assert hip.trlda_model_word_stats(m._handle, pi.ctypes.data, s.ctypes.data, s.ctypes.data,
                                                  s.ctypes.data) == _ffi.ERR_ARG
                assert hip.trlda_model_salient_words(m._handle, 5, pi.ctypes.data, w.ctypes.data,
                                                     s.ctypes.data) == _ffi.ERR_ARG
        assert hip.trlda_model_relevant_words(m._handle, 5, 0.6, None, None, None) == _ffi.ERR_ARG
        assert hip.trlda_model_word_stats(m._handle, None, None, s.ctypes.data, s.ctypes.data) == _ffi.ERR_ARG
        with pytest.raises(RuntimeError, match="different model"):
            m.topic_prevalence(other)
        with pytest.raises(RuntimeError, match="different model"):
            m.topic_prevalence_gamma(np.ones((K, B)), other)
        with pytest.raises(RuntimeError, match="same number of documents"):
            m.topic_prevalence_gamma(np.ones((K, B + 1)), _docs(V, B, 7))
        with pytest.raises(RuntimeError, match="finite and positive"):
            m.topic_prevalence_gamma(np.zeros((K, B)), _docs(V, B, 7))
        with pytest.raises(RuntimeError, match="wrong dimensionality"):
            m.topic_prevalence(_docs(V, B, 7), latents=np.ones((K, B + 1)))
        assert _live() == made                                        # no buffer was made for any of them
        with pytest.raises(RuntimeError, match="no document"):
            m.topic_prevalence([[], [(1, 0)]], latents=np.ones((K, 2)))
        assert np.all(w == -7) and np.all(s == -7.)
        # the model still works after the refusals
        words = m.relevant_words(V, 0.6)
        assert np.array_equal(np.sort(words, axis=1), np.tile(np.arange(V), (K, 1)))
    finally:
        other.close()
        m.close()


@pytest.mark.parametrize("planted", [0.0, float("nan"), -1.0, float("inf")])
def test_a_bad_lambda_is_refused(hip, planted):
    from trlda_amd import _ffi
    K, V = 70, 1100
    lam = _lam(K, V)
    lam[66, 1050] = planted
    m = _model(K, V, lam)
    w = np.full((K, 10), -7, dtype=np.int32)
    s = np.full((3, V), -7.)
    try:
        for call in (lambda: m.relevant_words(10), lambda: m.word_statistics(), lambda: m.salient_words(10),
                     lambda: m.relevant_words(10, 1.0, topic_weights=_given(K))):
            with pytest.raises(RuntimeError, match="positive, finite lambda"):
                call()
        assert hip.trlda_model_relevant_words(m._handle, 10, 0.6, None, w.ctypes.data, s.ctypes.data) == _ffi.ERR_VALUE
        assert hip.trlda_model_salient_words(m._handle, 10, None, w.ctypes.data, s.ctypes.data) == _ffi.ERR_VALUE
        assert hip.trlda_model_word_stats(m._handle, None, s[0].ctypes.data, s[1].ctypes.data,
                                          s[2].ctypes.data) == _ffi.ERR_VALUE
        assert np.all(w == -7) and np.all(s == -7.)                   # nothing was written
        m.lambdas = _lam(K, V)                                        # a good lambda again: the flag is per call
        assert m.relevant_words(10).shape == (K, 10)
    finally:
        m.close()


# 8. buffers ------------------------------------------------------------------------------------------
def test_no_buffer_is_left_after_close(hip):
    """A fresh process (the count is the process's): every new workspace and the accumulator; after
    close() the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "relevance_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout
