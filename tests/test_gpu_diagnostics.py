"""LDA.topic_word_diagnostics / topic_document_diagnostics / topic_diagnostics on the GPU
(csrc/diagnostics_kernels.h) against the longdouble restatement
(tests/diagnostics_host.py): every value within a first-order bound, the counts exactly, the token sums
bitwise against topic_prevalence and against the device's order restated on the host, independence of
the batching, the model's state, the errors and the buffers.

Every array is small: at most 1025 words, 33 documents and 513 topics."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import diagnostics_host as dh

pytestmark = pytest.mark.gpu

U = dh.U
LD = np.longdouble


def p_bound(K, V):
    """|p_dev - p| / p (tests/test_gpu_relevance.py, p_bound)."""
    return (V + 2 * K + 8) * U


def beta_bound(V):
    """|beta_dev - beta| / beta: R_k's V - 1 additions, the division 1 / R_k, the product."""
    return (V + 1) * U


def logbeta_bound(V, L):
    """|log beta_dev - log beta|, absolute; L bounds |log lambda|, |log R|, |log beta| and |log p|.
    log lambda: the device log at one ulp (2 u L); log R_k: (V - 1) u from the row sum and an ulp;
    the subtraction (u L)."""
    return (V - 1 + 5 * L) * U


def eff_bound(V):
    """Relative.  Q = sum beta^2: each term twice beta_bound and a product, V - 1 additions of
    positive terms; then the division 1 / Q."""
    return (2 * (V + 1) + 1 + (V - 1) + 1) * U


def entropy_bound(V, L, H):
    """|H_dev - H|, absolute.  Each term beta log beta: beta_bound |term| + beta logbeta_bound + the
    product (u |term|); V - 1 additions (u sum |term| each, the terms share a sign: sum |term| = H);
    sum beta = 1."""
    return ((V + 1 + 1 + V - 1) * H + (V - 1 + 5 * L)) * U


def corpus_bound(K, V, L, scale):
    """|C_dev - C|, absolute; scale = sum_w |beta (log beta - log p)|.  The factor log beta - log p:
    logbeta_bound, p_bound and an ulp of the device log for log p (2 u L), the subtraction (2 u L);
    then as entropy_bound."""
    factor = (V - 1 + 5 * L) + (V + 2 * K + 8) + 4 * L
    return ((V + 1 + 1 + V - 1) * scale + factor) * U


def exclusivity_bound(K, V, n):
    """Relative.  A ratio beta_kw / u_w: beta_bound for the numerator, beta_bound and K - 1
    additions for u_w, the division; the mean: n - 1 additions and a division."""
    return (2 * (V + 1) + (K - 1) + 1 + n) * U


def doc_entropy_bound(K, B, scales, A_over_T):
    """|entropy_dev - entropy|, absolute.  a_dk: K - 1 additions, a division and two products,
    (K + 2) u relative; T_k: B additions of positive terms, (B + K + 2) u relative, so log T_k has
    that error absolutely (the closing arithmetic is long double).  A_k = sum a log a: a's error moves
    a term by (K + 2) u a (|log a| + 1), the device log by an ulp and the product (3 u |a log a|), B
    additions (B u sum |a log a|).  A_k / T_k: A's error over T and |A / T| times T's."""
    s1, s2 = scales
    rel_T = (B + K + 2) * U
    err_A = ((K + 2) * s1 + (3 + B) * s2) * U
    return rel_T + err_A + np.abs(A_over_T) * rel_T + 4 * U


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


WORD_KEYS = ("eff_num_words", "word_entropy", "uniform_dist", "corpus_dist", "exclusivity")


def _check_word_side(got, ref, K, V, n):
    """Every value within its bound; returns each key's worst error over its bound."""
    L = ref["L"]
    H = ref["word_entropy"]
    bounds = {"eff_num_words": eff_bound(V) * ref["eff_num_words"],
              "word_entropy": entropy_bound(V, L, H),
              "uniform_dist": entropy_bound(V, L, H) + U * np.abs(ref["uniform_dist"]),
              "corpus_dist": corpus_bound(K, V, L, ref["scale_corpus"]),
              "exclusivity": exclusivity_bound(K, V, n) * ref["exclusivity"]}
    worst = {}
    for key in WORD_KEYS:
        assert got[key].dtype == np.float64 and got[key].shape == (K,)
        err = np.abs(got[key].astype(LD) - ref[key])
        worst[key] = float(np.max(err / bounds[key]))
        print("K = %d V = %d n = %d %s: worst err %.2f u, %.3f of its bound"
              % (K, V, n, key, float(err.max()) / U, worst[key]))
        assert np.all(err <= bounds[key]), (K, V, n, key, worst[key])
    assert np.all(got["uniform_dist"] >= -bounds["uniform_dist"])
    assert np.all(got["corpus_dist"] >= -bounds["corpus_dist"])
    return worst


# 1. the word side ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", dh.WORD_TOPICS)
def test_word_side(hip, K):
    """V over the chunk of 256 (below, at, past, five chunks) and the small vocabularies, top_n in 1,
    10, min(V, 100), default and given weights, lambda = Gamma(0.3) + 0.01.  The lists are
    top_words(top_n)'s, the restatement averages the exclusivity over the same lists; with words= from
    relevant_words it is averaged over those; two calls agree bitwise; K = 1 has exclusivity 1.0."""
    for V in dh.WORD_VOCABS:
        lam = dh.lam(K, V)
        m = _model(K, V, lam)
        try:
            for given in (None, dh.given(K)):
                base = dh.word_side(lam, 1, given)                    # (all but the exclusivity: once)

                def reference(words):
                    ref = dict(base)
                    ref["exclusivity"] = dh.exclusivity(lam, words)
                    return ref

                for n in sorted({1, min(V, 10), min(V, 100)}):
                    got = m.topic_word_diagnostics(n, topic_weights=given)
                    again = m.topic_word_diagnostics(n, topic_weights=given)
                    assert sorted(got) == sorted(WORD_KEYS + ("top_words",))
                    for key in got:
                        assert np.array_equal(got[key], again[key]), key
                    assert got["top_words"].dtype == np.int32
                    assert np.array_equal(got["top_words"], m.top_words(n))
                    _check_word_side(got, reference(got["top_words"]), K, V, n)
                    if K == 1:
                        assert got["exclusivity"][0] == 1.0
                # the lists of relevant_words
                n = min(V, 10)
                mine = m.relevant_words(n, 0.3, topic_weights=given)
                got = m.topic_word_diagnostics(topic_weights=given, words=mine)
                assert np.array_equal(got["top_words"], mine)
                _check_word_side(got, reference(mine), K, V, n)
                merged = m.topic_diagnostics(topic_weights=given, words=mine)
                for key in got:
                    assert np.array_equal(got[key], merged[key]), key
        finally:
            m.close()


@pytest.mark.parametrize("planted", [0.0, float("nan"), -1.0, float("inf")])
def test_a_bad_lambda_is_refused(hip, planted):
    from trlda_amd import _ffi
    K, V, n = 70, 600, 10
    lam = dh.lam(K, V)
    lam[66, 550] = planted
    m = _model(K, V, lam)
    words = np.tile(np.arange(n, dtype=np.int32), (K, 1))
    out = np.full((5, K), -7.)
    try:
        with pytest.raises(RuntimeError, match="positive, finite lambda"):
            m.topic_word_diagnostics(words=words)
        with pytest.raises(RuntimeError, match="positive, finite lambda"):
            m.topic_word_diagnostics(n, topic_weights=dh.given(K), words=words)
        assert hip.trlda_model_word_diagnostics(m._handle, n, None, words.ctypes.data,
                                                *[out[i].ctypes.data for i in range(5)]) == _ffi.ERR_VALUE
        assert np.all(out == -7.)                                     # nothing was written
        m.lambdas = dh.lam(K, V)                                      # a good lambda again: the flag is per call
        assert m.topic_word_diagnostics(n)["exclusivity"].shape == (K,)
    finally:
        m.close()


# 2. the document side --------------------------------------------------------------------------------
INT_KEYS = ("rank_1_docs", "docs_high", "docs_low")


def _same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=key == "allocation_ratio"), key


@pytest.mark.parametrize("K", dh.DOC_TOPICS)
def test_document_side_gamma(hip, K):
    """33 documents (an empty one, one token, counts <= 0 only, 300 entries) and the peaked gamma of
    diagnostics_host.gammas; tests/test_diagnostics_host.py asserts that nothing lies near a threshold
    or a rank tie, so every count is compared.  tokens: bitwise the device's order restated on the
    host, and normalised as the library's prevalence read-out normalises (the sum in long double in
    topic order, one rounding per quotient; a plain float64 `tokens / tokens.sum()` rounds
    differently and is compared to (K + 1) u) bitwise topic_prevalence_gamma.  One batch of 33, 1 + 32 and
    16 + 17 agree bitwise."""
    V, B = dh.DOC_V, dh.DOC_B
    docs, g = dh.documents(), dh.gammas(K)
    m = _model(K, V, dh.lam(K, V))
    try:
        for by_length in (True, False):
            ref = dh.document_side(g, docs, weight_by_length=by_length)
            assert not ref["near"]
            got = m.topic_document_diagnostics_gamma(g, docs, weight_by_length=by_length)
            assert got["num_docs"] == ref["num_docs"] == B - 2
            for key in INT_KEYS:
                assert got[key].dtype == np.int64 and got[key].shape == (K,)
                assert np.array_equal(got[key], ref[key]), key
            assert got["rank_1_docs"].sum() == got["num_docs"]
            assert np.array_equal(got["allocation_ratio"], ref["allocation_ratio"], equal_nan=True)
            pi = m.topic_prevalence_gamma(g, docs, weight_by_length=by_length)
            assert np.array_equal(dh.normalise(got["tokens"]), pi)
            # (K - 1 float64 additions in whatever order, a division, and pi's own rounding)
            assert np.max(np.abs(got["tokens"] / got["tokens"].sum() - pi) / pi) <= (K + 1) * U
            assert np.array_equal(got["tokens"], dh.tokens_device_order(g, docs, by_length))
            err_t = float(np.max(np.abs(got["tokens"].astype(LD) - ref["tokens"]) / ref["tokens"]))
            assert err_t <= (B + K + 2) * U
            A_over_T = np.log(ref["tokens"]) - ref["document_entropy"]
            bound = doc_entropy_bound(K, B, ref["scales"], A_over_T)
            err = np.abs(got["document_entropy"].astype(LD) - ref["document_entropy"])
            print("K = %d by_length = %s: tokens rel err %.2f u (bound %d u); entropy err %.2f u, %.3f of its "
                  "bound" % (K, by_length, err_t / U, B + K + 2, float(err.max()) / U, float(np.max(err / bound))))
            assert np.all(err <= bound), float(np.max(err / bound))
            for cuts in ((0, 1, 33), (0, 16, 33)):
                parts = iter([docs[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])])
                _same(m.topic_document_diagnostics_gamma(g, parts, weight_by_length=by_length), got)
        # other thresholds
        ref = dh.document_side(g, docs, high=0.3, low=0.1)
        assert not ref["near"]
        got = m.topic_document_diagnostics_gamma(g, docs, high=0.3, low=0.1)
        for key in INT_KEYS:
            assert np.array_equal(got[key], ref[key]), key
    finally:
        m.close()


def test_document_side_through_the_estep(hip):
    """topic_document_diagnostics(docs, latents=g0, max_iter=20) is bitwise the gamma form on
    update_variables' gamma; a list, an uploaded batch and an iterator of one batch agree;
    topic_diagnostics merges the two sides."""
    K, V, B = 20, dh.DOC_V, dh.DOC_B
    lam = dh.lam(K, V)
    docs = dh.documents(negative=False)
    g0 = np.asfortranarray(np.random.RandomState(3).gamma(1.0, 1.0, size=(K, B)) + 0.1)
    m = _model(K, V, lam)
    try:
        gamma, _ = m.update_variables(docs, latents=g0, max_iter=20)
        for by_length in (True, False):
            want = m.topic_document_diagnostics_gamma(gamma, docs, weight_by_length=by_length)
            _same(m.topic_document_diagnostics(docs, latents=g0, max_iter=20, weight_by_length=by_length), want)
            batch = m.upload(docs)
            _same(m.topic_document_diagnostics(batch, latents=g0, max_iter=20, weight_by_length=by_length), want)
            _same(m.topic_document_diagnostics(iter([batch]), latents=g0, max_iter=20,
                                               weight_by_length=by_length), want)
            batch.close()
            pi = m.topic_prevalence(docs, latents=g0, max_iter=20, weight_by_length=by_length)
            assert np.array_equal(dh.normalise(want["tokens"]), pi)
        both = m.topic_diagnostics(docs, latents=g0, max_iter=20, top_n=5)
        _same({k: both[k] for k in want}, m.topic_document_diagnostics_gamma(gamma, docs))
        _same({k: both[k] for k in both if k not in want}, m.topic_word_diagnostics(5))
        with pytest.raises(TypeError):
            m.topic_diagnostics(max_iter=20)
    finally:
        m.close()


# 3. state --------------------------------------------------------------------------------------------
def _draw_state():
    from trlda_amd import _ffi
    k = C.c_uint64(0)
    _ffi.check(_ffi.lib().trlda_rng_draw_key(C.byref(k)))
    return k.value


def test_state_is_left_alone(hip):
    """With deferred statistics and two stream lanes on: lambda, alpha, eta, update_count and the seeded
    stream stay where they were, the word side and the gamma form leave the model's statistics alone,
    and VI E-steps before and after the calls give the bits they give without them."""
    import trlda_amd
    from trlda_amd import _ffi
    K, V, B = 16, dh.DOC_V, dh.DOC_B
    lam = dh.lam(K, V)
    docs, other = dh.documents(negative=False), dh.documents(negative=False, seed=1)
    rng = np.random.RandomState(21)
    g0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)
    g1 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, B)) + 0.1)

    def run(between):
        m = _model(K, V, lam, alpha=.2, eta=.05)
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
            m.topic_word_diagnostics(10, topic_weights=dh.given(K))
            m.topic_document_diagnostics_gamma(g1, other)
            assert _draw_state() == want                              # nothing was drawn
            after = np.empty((K, V), order="F")
            _ffi.check(hip.trlda_model_get_sstats(m._handle, after))
            assert np.array_equal(held, after) and np.array_equal(held, out[0][1])   # no E-step ran
            trlda_amd.seed(9)                                         # (reading the state draws)
            m.topic_document_diagnostics(other, latents=g1, max_iter=20)   # an E-step from given latents: no draw
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


# 4. errors -------------------------------------------------------------------------------------------
def _live():
    from trlda_amd import _ffi
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return total.value


def test_errors_come_before_anything_is_allocated(hip):
    from trlda_amd import _ffi
    from trlda_amd.documents import DeviceBatch
    K, V, B = 8, 40, 4
    m = _model(K, V, dh.lam(K, V))
    docs = [[(1, 2)], [(2, 1), (3, 1)], [(0, 4)], [(5, 1)]]
    other = DeviceBatch(docs, V + 1, 0)
    ok = np.tile(np.arange(5, dtype=np.int32), (K, 1))
    out = np.full((5, K), -7.)
    ptrs = [out[i].ctypes.data for i in range(5)]
    try:
        made = _live()
        for high, low in ((0.5, 0.5), (0.02, 0.5), (1.0, 0.02), (0.5, -0.01), (float("nan"), 0.02), (0.5, float("nan"))):
            with pytest.raises(RuntimeError, match="low < high"):
                m.topic_document_diagnostics(docs, high=high, low=low)
            with pytest.raises(RuntimeError, match="low < high"):
                m.topic_document_diagnostics_gamma(np.ones((K, B)), docs, high=high, low=low)
            acc = _ffi.vp()
            assert hip.trlda_topicdiag_create(m._handle, 1, high, low, C.byref(acc)) == _ffi.ERR_ARG and not acc
        for top_n in (0, -1, V + 1, 101):
            with pytest.raises(RuntimeError, match="top_n"):
                m.topic_word_diagnostics(top_n)
            assert hip.trlda_model_word_diagnostics(m._handle, top_n, None, ok.ctypes.data, *ptrs) == _ffi.ERR_ARG
        for pi in (np.ones(K + 1), np.r_[np.ones(K - 1), 0.0], np.r_[np.ones(K - 1), np.nan]):
            with pytest.raises(RuntimeError, match="topic_weights"):
                m.topic_word_diagnostics(5, topic_weights=pi)
        for bad in (ok[:-1], ok.astype(np.float64), np.where(ok == 2, V, ok), np.where(ok == 2, -1, ok),
                    np.where(ok == 2, 3, ok), np.tile(np.arange(101), (K, 1))):
            with pytest.raises(RuntimeError):
                m.topic_word_diagnostics(words=bad)
        for bad, code in ((np.where(ok == 2, V, ok), _ffi.ERR_WORD_ID), (np.where(ok == 2, 3, ok), _ffi.ERR_ARG)):
            bad = np.ascontiguousarray(bad, dtype=np.int32)
            assert hip.trlda_model_word_diagnostics(m._handle, 5, None, bad.ctypes.data, *ptrs) == code
        assert hip.trlda_model_word_diagnostics(m._handle, 5, None, None, *ptrs) == _ffi.ERR_ARG
        with pytest.raises(RuntimeError, match="different model"):
            m.topic_document_diagnostics(other)
        with pytest.raises(RuntimeError, match="different model"):
            m.topic_document_diagnostics_gamma(np.ones((K, B)), other)
        with pytest.raises(RuntimeError, match="same number of documents"):
            m.topic_document_diagnostics_gamma(np.ones((K, B + 1)), docs)
        with pytest.raises(RuntimeError, match="finite and positive"):
            m.topic_document_diagnostics_gamma(np.zeros((K, B)), docs)
        with pytest.raises(RuntimeError, match="wrong dimensionality"):
            m.topic_document_diagnostics(docs, latents=np.ones((K, B + 1)))
        assert _live() == made                                        # no buffer was made for any of them
        with pytest.raises(RuntimeError, match="no document"):
            m.topic_document_diagnostics([[], [(1, 0)]], latents=np.ones((K, 2)))
        assert np.all(out == -7.)
        # the model still works after the refusals
        assert m.topic_diagnostics(docs, latents=np.ones((K, B)))["num_docs"] == B
    finally:
        other.close()
        m.close()


# 5. buffers ------------------------------------------------------------------------------------------
def test_no_buffer_is_left_after_close(hip):
    """A fresh process (the count is the process's): every new workspace and the accumulator; after
    close() the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diagnostics_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout
