"""CPU checks of the held-out ranks and the full-ranking metrics: the restatement (tests/ranks_host.py)
on hand cases, the pure ``_ranking_metrics`` of ``LDA.ranking_metrics`` on figures written out by hand
and against a brute-force restatement, and what the library and ``LDA.heldout_ranks*`` answer before any
GPU work."""
import numpy as np
import pytest

import ranks_host as kh
import recommend_host as rh


def _csr(docs):
    indptr = np.cumsum([0] + [len(d) for d in docs])
    flat = [p for d in docs for p in d]
    ids = np.array([p[0] for p in flat], dtype=np.int32)
    cnts = np.array([p[1] for p in flat], dtype=np.int32)
    return indptr.astype(np.int32), ids, cnts


LAM1 = np.array([[0.5, 4.0, 0.25, 3.0, 8.0, 1.0]])            # K = 1: the ranking is 4, 1, 3, 5, 0, 2


# -- the restatement ------------------------------------------------------------------------------
def test_one_topic_ranks_follow_lambda():
    for g in (0.1, 7.0):
        indptr, words, ranks, cand, scores, gap = kh.ranks(np.array([[g]]), LAM1, None, _csr([[(3, 1), (2, 5), (4, 1)]]))
        assert indptr.dtype == np.int64 and words.dtype == ranks.dtype == cand.dtype == np.int32
        assert list(indptr) == [0, 3] and list(words) == [2, 3, 4] and list(ranks) == [6, 3, 1] and list(cand) == [6]
        assert np.allclose(scores.astype(np.float64), LAM1[0, [2, 3, 4]] / LAM1.sum(), rtol=0, atol=1e-16)
        # the nearest other score: 0.5 to 0.25, 4 to 3, 4 to 8
        assert np.allclose(gap, [0.25 / 0.25, 1.0 / 3.0, 4.0 / 8.0], rtol=1e-15)


def test_equal_columns_go_by_smaller_id():
    rng = np.random.RandomState(3)
    lam = rng.gamma(2.0, 1.0, size=(3, 7))
    lam[:, 5] = lam[:, 1]
    gamma = rng.gamma(1.0, 1.0, size=(3, 4)) + 0.1
    held = _csr([[(1, 1), (5, 1)]] * 4)
    indptr, words, ranks, cand, scores, gap = kh.ranks(gamma, lam, None, held)
    for d in range(4):
        assert list(words[2 * d:2 * d + 2]) == [1, 5] and ranks[2 * d + 1] == ranks[2 * d] + 1
        assert scores[2 * d] == scores[2 * d + 1]
    assert np.all(gap == 0)
    # the tied word seen: it is not counted
    indptr, words, ranks2, cand, _, _ = kh.ranks(gamma, lam, _csr([[(1, 2)]] * 4), _csr([[(5, 1)]] * 4))
    assert np.array_equal(ranks2, ranks[1::2] - 1) and list(cand) == [6] * 4


def test_relevance_and_candidates_by_hand():
    gamma = np.ones((1, 7))
    observed = _csr([[(4, 2), (1, 1)],                    # has seen 4 and 1: the ranking is 3, 5, 0, 2
                     [(4, 0), (4, -1)],                   # c = 0 and c = -1: has seen nothing
                     [(4, 1), (4, 3)],                    # listed twice: seen once
                     [(w, 1) for w in (0, 1, 2, 3, 4)],   # all but word 5: n = 1
                     [(w, 1) for w in range(6)],          # everything: n = 0
                     [],
                     [(0, 1)]])
    heldout = _csr([[(1, 1), (5, 1), (2, 3)],             # 1 is in both parts: not relevant
                    [(4, 1), (0, 0), (2, -1)],            # 0 and 2 have no positive count
                    [(3, 1), (3, 2), (4, 1)],             # 3 listed twice: once; 4 seen
                    [(5, 1), (0, 1)],
                    [(5, 1)],                             # no candidate at all
                    [],
                    [(2, 0)]])                            # no relevant word
    indptr, words, ranks, cand, scores, gap = kh.ranks(gamma, LAM1, observed, heldout)
    assert list(cand) == [4, 6, 5, 1, 0, 6, 5]
    assert list(indptr) == [0, 2, 3, 4, 5, 5, 5, 5]
    assert list(words) == [2, 5, 4, 3, 5] and list(ranks) == [4, 2, 1, 2, 1]
    assert np.isinf(gap[4]) and np.all(np.isfinite(gap[:4]))
    # docs=None: every word is a candidate, every distinct positive-count held-out word relevant
    indptr, words, ranks, cand, _, _ = kh.ranks(gamma, LAM1, None, heldout)
    assert list(cand) == [6] * 7 and list(indptr) == [0, 3, 4, 6, 8, 9, 9, 9]
    assert list(words) == [1, 2, 5, 4, 3, 4, 0, 5, 5] and list(ranks) == [2, 6, 4, 1, 3, 1, 5, 4, 4]


def test_ranks_are_positions_of_the_recommendation():
    """Against rh.recommend with top_n = V: the restatement of the list the ranks are positions in."""
    rng = np.random.RandomState(11)
    K, V, B = 4, 30, 12
    lam = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    gamma = rng.gamma(0.5, 1.0, size=(K, B)) + 0.01
    def part():
        return [[(int(w), int(c)) for w, c in zip(rng.randint(0, V, size=n), rng.randint(-1, 3, size=n))]
                for n in rng.randint(0, 9, size=B)]
    observed, heldout = _csr(part()), _csr(part())
    indptr, words, ranks, cand, scores, gap = kh.ranks(gamma, lam, observed, heldout)
    full, probs, _ = rh.recommend(gamma, lam, V, observed)
    assert np.array_equal(cand, (full >= 0).sum(axis=1)) and len(words) > 10
    for d in range(B):
        for p in range(indptr[d], indptr[d + 1]):
            assert full[d, ranks[p] - 1] == words[p] and probs[d, ranks[p] - 1] == scores[p]
    _, _, relevant = rh.recall(full, observed, heldout, V)
    assert np.array_equal(np.diff(indptr), relevant)


# -- the metrics ----------------------------------------------------------------------------------
def _metrics(*args, **kwargs):
    from trlda_amd.models import _ranking_metrics
    return _ranking_metrics(*args, **kwargs)


def test_metrics_by_hand():
    """Four documents: n = 10 with ranks (4, 1) -- given unsorted --, n = 5 with rank 2, one without
    a relevant word, and n = 2 with ranks (1, 2), which has n = R and is left out of the AUC."""
    indptr, ranks, cand = [0, 2, 3, 3, 5], [4, 1, 2, 1, 2], [10, 5, 7, 2]
    got = _metrics(indptr, ranks, cand, (1, 4, 1000), return_documents=True)
    l2 = np.log2
    doc = got["documents"]
    # document 0: AUC = 1 - (0 + 2) / (2 * 8), AP = (1/1 + 2/4) / 2, percentiles 0 and 3/9
    assert doc["auc"][0] == 0.875 and doc["map"][0] == 0.75 and doc["mrr"][0] == 1.0
    assert doc["percentile_rank"][0] == (0.0 + 3.0 / 9.0) / 2
    assert abs(doc["ndcg"][0] - (1 / l2(2) + 1 / l2(5)) / (1 / l2(2) + 1 / l2(3))) <= 1e-15
    # document 1: AUC = 1 - (2 - 1) / (1 * 4), AP = 1/2, percentile 1/4
    assert doc["auc"][1] == 0.75 and doc["map"][1] == 0.5 and doc["mrr"][1] == 0.5
    assert doc["percentile_rank"][1] == 0.25 and abs(doc["ndcg"][1] - 1 / l2(3)) <= 1e-15
    assert all(np.isnan(doc[k][2]) for k in ("auc", "map", "mrr", "ndcg", "percentile_rank"))
    assert np.isnan(doc["auc"][3]) and doc["map"][3] == 1.0 and doc["mrr"][3] == 1.0 and doc["ndcg"][3] == 1.0
    assert doc["percentile_rank"][3] == 0.5
    assert np.array_equal(doc["relevant"], [2, 1, 0, 2]) and doc["relevant"].dtype == np.int64
    assert np.array_equal(doc["recall"][1], [0.5, 0.0, np.nan, 0.5], equal_nan=True)
    assert np.array_equal(doc["recall"][4], [1.0, 1.0, np.nan, 1.0], equal_nan=True)
    # the six figures
    assert abs(got["mean_percentile_rank"] - (0.0 + 1.0 / 3.0 + 0.25 + 0.0 + 1.0) / 5) <= 1e-16
    assert got["auc"] == (0.875 + 0.75) / 2
    assert got["mrr"] == (1.0 + 0.5 + 1.0) / 3
    assert got["map"] == (0.75 + 0.5 + 1.0) / 3
    assert abs(got["ndcg"] - ((1 + 1 / l2(5)) / (1 + 1 / l2(3)) + 1 / l2(3) + 1.0) / 3) <= 1e-15
    assert got["recall"] == {1: (0.5 + 0.0 + 0.5) / 3, 4: 1.0, 1000: 1.0}
    assert "documents" not in _metrics(indptr, ranks, cand, 4) and _metrics(indptr, ranks, cand, 4)["recall"] == {4: 1.0}
    # a document whose only candidate is its relevant word: percentile 0, no AUC at all
    one = _metrics([0, 1], [1], [1], (1,))
    assert one["mean_percentile_rank"] == 0.0 and np.isnan(one["auc"]) and one["mrr"] == 1.0


def _random_case(rng, B, V, sizes=None):
    """B documents: a seen set, a ranking of the unseen words (a permutation) and relevant words among them."""
    indptr, ranks, cand, lists, observed, heldout = [0], [], [], [], [], []
    for d in range(B):
        seen = rng.permutation(V)[:rng.randint(0, V - 8)]
        order = np.array([w for w in rng.permutation(V) if w not in set(seen)])
        R = rng.randint(0, 7) if sizes is None else sizes[d % len(sizes)]
        want = np.sort(rng.permutation(order)[:R])
        position = {w: i for i, w in enumerate(order)}
        ranks.extend(position[w] + 1 for w in want)
        indptr.append(len(ranks))
        cand.append(len(order))
        lists.append(list(order) + [-1] * (V - len(order)))
        observed.append([(int(w), 1) for w in seen])
        heldout.append([(int(w), 2) for w in want] + [(int(w), 1) for w in seen[:2]])
    return indptr, ranks, cand, np.array(lists), observed, heldout


def test_metrics_against_brute_force():
    rng = np.random.RandomState(17)
    B, V, tops = 40, 30, (1, 6, 30)
    indptr, ranks, cand, _, _, _ = _random_case(rng, B, V)
    got = _metrics(indptr, ranks, cand, tops)
    want = kh.metrics(indptr, ranks, cand, tops)
    assert (np.diff(indptr) == 0).any() and 0 < got["mean_percentile_rank"] < 1
    for key in ("mean_percentile_rank", "auc", "mrr", "map", "ndcg"):
        assert abs(got[key] - want[key]) <= 1e-12, key
    for n in tops:
        assert abs(got["recall"][n] - want["recall"][n]) <= 1e-12, n
    assert got["recall"][30] == 1.0


def test_recall_is_recall_at_of_the_full_list():
    """recall[N] equals _recall_at on the first N of the full list, N = 1, 6, 30.  Every document has 0,
    1, 2 or 4 relevant words, so each ratio is a multiple of 1/4 and both ways of adding are exact."""
    from trlda_amd.models import _recall_at
    rng = np.random.RandomState(23)
    B, V = 40, 30
    indptr, ranks, cand, lists, observed, heldout = _random_case(rng, B, V, sizes=(1, 4, 0, 2, 4))
    got = _metrics(indptr, ranks, cand, (1, 6, 30), return_documents=True)
    for n in (1, 6, 30):
        recall, hits, relevant = _recall_at(lists[:, :n], _csr(observed), _csr(heldout), V)
        assert got["recall"][n] == recall, n
        assert np.array_equal(got["documents"]["relevant"], relevant)
        keep = relevant > 0
        assert np.array_equal(got["documents"]["recall"][n][keep], hits[keep] / relevant[keep])


def test_metrics_need_a_relevant_word():
    with pytest.raises(RuntimeError, match="held-out"):
        _metrics([0, 0, 0], [], [5, 6], (10,))
    for bad in (0, -3, (10, 0)):
        with pytest.raises(RuntimeError, match="top_n"):
            _metrics([0, 1], [1], [5], bad)
    with pytest.raises(TypeError):
        _metrics([0, 1], [1], [5], 2.5)
    assert kh.metrics([0, 0, 0], [], [5, 6], (10,)) is None


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
    for name in ("heldout_ranks", "heldout_ranks_gamma", "ranking_metrics"):
        assert callable(getattr(LDA, name)) and "DESIGN.md 3.30" in getattr(LDA, name).__doc__
    m = _bare(3, 200)
    docs = [[(0, 1)], [(1, 1)]]
    g = np.ones((3, 2))
    with pytest.raises(RuntimeError, match="equal in number"):
        m.heldout_ranks(docs, docs[:1])
    with pytest.raises(RuntimeError, match="equal in number"):
        m.ranking_metrics(docs, docs[:1])
    for bad in (0, (10, -1)):
        with pytest.raises(RuntimeError, match="top_n"):
            m.ranking_metrics(docs, docs, top_n=bad)
    with pytest.raises(TypeError):
        m.ranking_metrics(docs, docs, top_n=2.5)
    # gamma: shape, type, finite and positive -- the checks and messages of recommend_gamma
    for bad in (np.ones((4, 2)), np.ones((2, 3, 1)), np.ones(4)):
        with pytest.raises(RuntimeError, match="Gamma has wrong dimensionality."):
            m.heldout_ranks_gamma(bad, docs)
    with pytest.raises(TypeError):
        m.heldout_ranks_gamma("gamma", docs)
    for bad in (0.0, -1.0, np.inf, -np.inf, np.nan):
        spoiled = g.copy()
        spoiled[2, 1] = bad
        with pytest.raises(RuntimeError, match="finite and positive"):
            m.heldout_ranks_gamma(spoiled, docs)
    with pytest.raises(RuntimeError, match="same number of documents"):
        m.heldout_ranks_gamma(g, docs + docs)
    with pytest.raises(RuntimeError, match="same number of documents"):
        m.heldout_ranks_gamma(g, docs, docs=docs + docs)
    # an empty gamma needs no device either
    out = m.heldout_ranks_gamma(np.empty((3, 0)), [], return_scores=True)
    assert [len(a) for a in out] == [1, 0, 0, 0, 0] and out[0].dtype == np.int64
    assert out[1].dtype == out[2].dtype == out[3].dtype == np.int32 and out[4].dtype == np.float64


def test_entries_to_lists():
    """What Python makes of the library's per-entry results: rank 0 dropped, a word once, ascending id."""
    from trlda_amd.models import _ranks_entries
    indptr = [0, 4, 4, 7]
    ids = [5, 2, 5, 9, 1, 0, 1]
    ranks = [3, 0, 3, 1, 7, 2, 7]
    scores = [.3, 0., .3, .9, .1, .5, .1]
    got = _ranks_entries(indptr, ids, np.array(ranks, dtype=np.int32), np.array(scores), 10)
    assert got[0].dtype == np.int64 and got[1].dtype == got[2].dtype == np.int32 and got[3].dtype == np.float64
    assert list(got[0]) == [0, 2, 2, 4] and list(got[1]) == [5, 9, 0, 1] and list(got[2]) == [3, 1, 2, 7]
    assert list(got[3]) == [.3, .9, .5, .1]


def test_ranks_entry_points_are_exported(hip_lib):
    from trlda_amd import _ffi
    for name in ("trlda_model_heldout_ranks", "trlda_model_heldout_ranks_dev", "trlda_model_set_ranks_chunk"):
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    # (no model: the argument check answers before any device is touched)
    assert hip_lib.trlda_model_heldout_ranks(None, None, None, None, 1, 10, 1e-3, None, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_model_heldout_ranks_dev(None, None, None, None, 1, None, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_model_set_ranks_chunk(None, 4) == _ffi.ERR_ARG


def test_ranks_kernels_do_not_spill(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    mine = {k: v for k, v in res.items() if "ranks_" in k}
    assert len(mine) == 3, sorted(mine)                  # thresholds, order, count<2>
    for name, f in mine.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_spill_count"] == 0, (name, f)
        if "count_kernel" in name:
            assert f["vgpr_count"] <= 512, (name, f)     # one workgroup per CU: its LDS leaves room for no more
