"""CPU checks of the word recommendation: the restatement (tests/recommend_host.py) on hand cases --
its ranking, tie order, exclusion and pad --, the pure recall function of ``LDA.recall_at`` on
hand-made arrays, and what the library and ``LDA.recommend*`` answer before any GPU work."""
import numpy as np
import pytest

import recommend_host as rh


def _csr(docs):
    indptr = np.cumsum([0] + [len(d) for d in docs])
    flat = [p for d in docs for p in d]
    ids = np.array([p[0] for p in flat], dtype=np.int32)
    cnts = np.array([p[1] for p in flat], dtype=np.int32)
    return indptr.astype(np.int32), ids, cnts


# -- the restatement ------------------------------------------------------------------------------
def test_scores_by_hand():
    """K = 2, V = 3: theta = (1/4, 3/4); beta_0 = (1/2, 1/4, 1/4), beta_1 = (1/8, 1/8, 3/4)."""
    lam = np.array([[2.0, 1.0, 1.0], [1.0, 1.0, 6.0]])
    s = rh.scores(np.array([[1.0], [3.0]]), lam)
    want = [0.25 * 0.5 + 0.75 * 0.125, 0.25 * 0.25 + 0.75 * 0.125, 0.25 * 0.25 + 0.75 * 0.75]
    assert s.shape == (1, 3) and np.allclose(s[0].astype(np.float64), want, rtol=0, atol=1e-16)
    assert abs(float(s.sum()) - 1.0) <= 1e-16                  # p(. | d) is a distribution
    words, probs, gap = rh.recommend(np.array([[1.0], [3.0]]), lam, 3)
    assert words.dtype == np.int32 and np.array_equal(words, [[2, 0, 1]])
    assert np.allclose(probs[0].astype(np.float64), [want[2], want[0], want[1]], rtol=0, atol=1e-16)
    assert abs(gap[0] - (want[0] - want[1]) / want[0]) <= 1e-15


def test_one_topic_ranks_by_lambda():
    lam = np.array([[0.5, 4.0, 0.25, 3.0, 8.0, 1.0]])
    for g in (0.1, 7.0):
        words, probs, gap = rh.recommend(np.array([[g]]), lam, 6)
        assert np.array_equal(words[0], np.lexsort((np.arange(6), -lam[0]))) and list(words[0]) == [4, 1, 3, 5, 0, 2]
        assert np.allclose(probs[0].astype(np.float64), lam[0, words[0]] / lam.sum(), rtol=0, atol=1e-16)
        assert gap[0] > 0


def test_equal_columns_go_by_smaller_id():
    rng = np.random.RandomState(3)
    lam = rng.gamma(2.0, 1.0, size=(3, 7))
    lam[:, 5] = lam[:, 1]
    gamma = rng.gamma(1.0, 1.0, size=(3, 4)) + 0.1
    words, probs, gap = rh.recommend(gamma, lam, 7)
    for d in range(4):
        at1, at5 = list(words[d]).index(1), list(words[d]).index(5)
        assert at5 == at1 + 1 and probs[d, at1] == probs[d, at5]
    assert np.all(gap == 0)


def test_seen_words_are_left_out():
    lam = np.array([[0.5, 4.0, 0.25, 3.0, 8.0, 1.0]])
    gamma = np.ones((1, 3))
    # document 0 has seen the best word; document 1 lists it with c = 0 and c = -1, which do not
    # count; document 2 lists it twice
    docs = _csr([[(4, 2)], [(4, 0), (4, -1), (1, 1)], [(4, 1), (3, 5), (4, 3)]])
    words, probs, _ = rh.recommend(gamma, lam, 3, docs)
    assert np.array_equal(words, [[1, 3, 5], [4, 3, 5], [1, 5, 0]])
    assert np.array_equal(rh.seen(*docs, 6).sum(axis=1), [1, 1, 2])
    every, _, _ = rh.recommend(gamma, lam, 3)
    assert np.array_equal(every, [[4, 1, 3]] * 3)


def test_pad():
    """Seen all but 2 of V = 6 words, top_n = 5: three pads of (-1, 0.0)."""
    lam = np.array([[0.5, 4.0, 0.25, 3.0, 8.0, 1.0]])
    docs = _csr([[(4, 1), (1, 1), (3, 2), (5, 1)], []])
    words, probs, gap = rh.recommend(np.ones((1, 2)), lam, 5, docs)
    assert np.array_equal(words, [[0, 2, -1, -1, -1], [4, 1, 3, 5, 0]])
    assert np.all(probs[0, 2:] == 0) and np.all(probs[0, :2] > 0) and np.all(probs[1] > 0)
    assert gap[0] == (0.5 - 0.25) / 0.5 and np.isfinite(gap[1])
    # a single candidate, none
    one = _csr([[(w, 1) for w in (0, 1, 2, 3, 4)], [(w, 1) for w in range(6)]])
    words, probs, gap = rh.recommend(np.ones((1, 2)), lam, 2, one)
    assert np.array_equal(words, [[5, -1], [-1, -1]]) and np.all(np.isinf(gap))


# -- recall ---------------------------------------------------------------------------------------
def _recall(words, observed, heldout, V):
    from trlda_amd.models import _recall_at
    return _recall_at(np.asarray(words), _csr(observed), _csr(heldout), V)


def test_recall_by_hand():
    V = 10
    observed = [[(0, 1), (1, 2)],          # has seen 0 and 1
                [(2, 1)],
                [(5, 0)],                  # c = 0: has not seen 5
                []]
    heldout = [[(1, 1), (2, 1), (3, 1), (3, 2)],      # 1 is in both parts: not relevant; 3 twice: once
               [(2, 4)],                              # nothing relevant
               [(5, 1), (6, 0)],                      # 6 has no positive count
               [(7, 1), (8, 1), (9, 1)]]
    words = [[1, 2, 9],                    # 1 is no hit although recommended; 2 is
             [2, 3, 4],
             [5, -1, -1],
             [0, 1, 2]]
    recall, hits, relevant = _recall(words, observed, heldout, V)
    assert hits.dtype == relevant.dtype == np.int64
    assert np.array_equal(relevant, [2, 0, 1, 3]) and np.array_equal(hits, [1, 0, 1, 0])
    assert recall == (0.5 + 1.0 + 0.0) / 3                    # document 1 is left out of the mean
    r2, h2, n2 = rh.recall(np.asarray(words), _csr(observed), _csr(heldout), V)
    assert abs(r2 - recall) <= 1e-16 and np.array_equal(h2, hits) and np.array_equal(n2, relevant)


def test_recall_needs_a_relevant_word():
    with pytest.raises(RuntimeError, match="held-out"):
        _recall([[1, 2], [0, 3]], [[(0, 1)], [(1, 1)]], [[(0, 2)], [(1, 1), (2, 0)]], 4)
    with pytest.raises(RuntimeError, match="equal in number"):
        _recall([[1, 2], [0, 3]], [[(0, 1)], [(1, 1)]], [[(0, 2)]], 4)
    assert rh.recall(np.array([[1, 2]]), _csr([[(0, 1)]]), _csr([[(0, 2)]]), 4)[0] is None


def test_recall_against_the_restatement():
    rng = np.random.RandomState(5)
    V, B, top_n = 30, 40, 6
    def part():
        return [[(int(w), int(c)) for w, c in zip(rng.randint(0, V, size=n), rng.randint(-1, 3, size=n))]
                for n in rng.randint(0, 9, size=B)]
    observed, heldout = part(), part()
    words = np.array([rng.permutation(V)[:top_n] for _ in range(B)])
    words[rng.uniform(size=words.shape) < 0.1] = -1
    recall, hits, relevant = _recall(words, observed, heldout, V)
    r2, h2, n2 = rh.recall(words, _csr(observed), _csr(heldout), V)
    assert np.array_equal(hits, h2) and np.array_equal(relevant, n2) and abs(recall - r2) <= 1e-15
    assert 0 < recall < 1 and (relevant == 0).any()


# -- the library ----------------------------------------------------------------------------------
def _bare(K, V):
    """An LDA that has no device side: whatever it raises, it raises before any GPU work."""
    from trlda_amd.models import LDA
    m = LDA.__new__(LDA)
    m._handle, m._K, m._V, m._device = None, K, V, 0
    return m


def test_argument_errors_come_before_any_gpu_work():
    import trlda.models
    from trlda_amd.models import LDA
    assert trlda.models.LDA is LDA
    for name in ("recommend", "recommend_gamma", "recall_at"):
        assert callable(getattr(LDA, name)) and "DESIGN.md 3.22" in getattr(LDA, name).__doc__
    m = _bare(3, 200)
    docs = [[(0, 1)], [(1, 1)]]
    g = np.ones((3, 2))
    for top_n in (0, -1, 101):
        with pytest.raises(RuntimeError, match="top_n"):
            m.recommend(docs, top_n=top_n)
        with pytest.raises(RuntimeError, match="top_n"):
            m.recommend_gamma(g, top_n=top_n)
        with pytest.raises(RuntimeError, match="top_n"):
            m.recall_at(docs, docs, top_n=top_n)
    small = _bare(3, 7)
    for call in (lambda: small.recommend(docs, top_n=8), lambda: small.recommend_gamma(g, top_n=8),
                 lambda: small.recall_at(docs, docs, top_n=8)):
        with pytest.raises(RuntimeError, match="top_n"):
            call()
    with pytest.raises(TypeError):
        m.recommend_gamma(g, top_n=2.5)
    # gamma: shape, type, finite and positive
    for bad in (np.ones((4, 2)), np.ones((2, 3, 1)), np.ones(4)):
        with pytest.raises(RuntimeError, match="Gamma has wrong dimensionality."):
            m.recommend_gamma(bad)
    with pytest.raises(TypeError):
        m.recommend_gamma("gamma")
    for bad in (0.0, -1.0, np.inf, -np.inf, np.nan):
        spoiled = g.copy()
        spoiled[2, 1] = bad
        with pytest.raises(RuntimeError, match="finite and positive"):
            m.recommend_gamma(spoiled)
    with pytest.raises(RuntimeError, match="same number of documents"):
        m.recommend_gamma(g, docs=docs + docs)
    # parts of unequal number
    with pytest.raises(RuntimeError, match="equal in number"):
        m.recall_at(docs, docs[:1])
    # an empty gamma needs no device either
    words, probs = m.recommend_gamma(np.empty((3, 0)), top_n=4)
    assert words.shape == probs.shape == (0, 4) and words.dtype == np.int32 and probs.dtype == np.float64


def test_recommend_entry_points_are_exported(hip_lib):
    from trlda_amd import _ffi
    for name in ("trlda_model_recommend", "trlda_model_recommend_dev", "trlda_model_set_recommend_slab_words"):
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    # (no model: the argument check answers before any device is touched)
    assert hip_lib.trlda_model_recommend(None, None, None, 1, 1, 10, 1e-3, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_model_recommend_dev(None, None, None, 1, 1, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_model_set_recommend_slab_words(None, 16) == _ffi.ERR_ARG


def test_recommend_kernels_do_not_spill(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    mine = {k: v for k, v in res.items() if "recommend_" in k}
    assert len(mine) == 5, sorted(mine)                  # rows, seen, query<1>, query<2>, merge
    for name, f in mine.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_spill_count"] == 0, (name, f)
        if "query_kernelILi1E" in name:
            assert f["vgpr_count"] <= 256, (name, f)     # two waves per SIMD
        elif "query" in name:
            assert f["vgpr_count"] <= 512, (name, f)     # one: its LDS leaves room for one workgroup from top_n = 12 on
