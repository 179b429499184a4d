"""CPU checks of the topic-diagnostics restatement (tests/diagnostics_host.py): the
closed forms by hand, the device-order token sums against the plain ones, and the input condition of
tests/test_gpu_diagnostics.py -- the restatement's near list is empty for every input used there, so
no document is left out of a comparison on the GPU."""
import numpy as np
import pytest

import diagnostics_host as dh
import relevance_host as vh

LD = np.longdouble
TINY = 1e-17                             # longdouble arithmetic on a handful of terms


def test_constant_lambda():
    """Every topic uniform: eff_num_words = V, both divergences 0, exclusivity 1 / K."""
    K, V = 4, 37
    w = dh.word_side(np.full((K, V), 2.5), top_n=5)
    assert np.max(np.abs(w["eff_num_words"] - V)) <= V * TINY
    assert np.max(np.abs(w["word_entropy"] - np.log(LD(V)))) <= 10 * TINY
    assert np.max(np.abs(w["uniform_dist"])) <= 10 * TINY and np.max(np.abs(w["corpus_dist"])) <= 10 * TINY
    assert np.max(np.abs(w["exclusivity"] - LD(1) / K)) <= TINY
    assert np.array_equal(w["top_words"], np.tile(np.arange(5), (K, 1)))   # (ties by smaller id)


def test_disjoint_blocks():
    """Topic k owns words k W .. k W + W - 1 (value 1) over a floor eps: as eps -> 0 exclusivity -> 1,
    corpus_dist -> log K under equal weights and eff_num_words -> W.  At eps = 1e-12 each is within
    1e-9 of its limit (the floor moves them by O(K W eps log(1 / eps)))."""
    K, W = 5, 8
    lam = np.full((K, K * W), 1e-12)
    for k in range(K):
        lam[k, k * W:(k + 1) * W] = 1.0
    w = dh.word_side(lam, top_n=W, topic_weights=np.ones(K))
    assert np.max(np.abs(w["exclusivity"] - 1)) <= 1e-9
    assert np.max(np.abs(w["corpus_dist"] - np.log(LD(K)))) <= 1e-9
    assert np.max(np.abs(w["eff_num_words"] - W)) <= 1e-9
    for k in range(K):
        assert sorted(w["top_words"][k]) == list(range(k * W, (k + 1) * W))
    # K = 1: every ratio is beta / beta
    one = dh.word_side(lam[:1], top_n=3)
    assert one["exclusivity"][0] == 1 and abs(one["corpus_dist"][0]) <= TINY


def test_words_argument_and_weights():
    lam = dh.lam(3, 20)
    mine = np.array([[4, 2, 9], [0, 1, 2], [19, 3, 7]])
    a, b = dh.word_side(lam, words=mine), dh.word_side(lam, top_n=3)
    assert np.array_equal(a["top_words"], mine) and not np.array_equal(a["exclusivity"], b["exclusivity"])
    for key in ("eff_num_words", "word_entropy", "uniform_dist", "corpus_dist"):
        assert np.array_equal(a[key], b[key])
    beta = lam.astype(LD) / lam.astype(LD).sum(axis=1)[:, None]
    want = np.mean([beta[1, w] / beta[:, w].sum() for w in (0, 1, 2)])
    assert abs(a["exclusivity"][1] - want) <= TINY
    # corpus_dist is the KL divergence from the p of the same weights
    pi = dh.given(3)
    p = vh.word_statistics(lam, pi)[0]
    kl = (beta * np.log(beta / p[None, :])).sum(axis=1)
    assert np.max(np.abs(dh.word_side(lam, topic_weights=pi)["corpus_dist"] - kl)) <= 100 * TINY
    assert np.all(kl > 0)


def test_identical_documents():
    """D identical documents: p(d | k) = 1 / D for every topic, entropy log D."""
    D, K = 7, 4
    gamma = np.tile(np.array([[0.5], [3.0], [1.0], [0.25]]), (1, D))
    docs = [[(1, 2), (4, 3)]] * D
    for by_length in (True, False):
        r = dh.document_side(gamma, docs, weight_by_length=by_length)
        assert np.max(np.abs(r["document_entropy"] - np.log(LD(D)))) <= 10 * TINY
        assert r["num_docs"] == D and list(r["rank_1_docs"]) == [0, D, 0, 0]
        # theta = (2, 12, 4, 1) / 19: only topic 1 is above 0.5, all are above 0.02
        assert list(r["docs_high"]) == [0, D, 0, 0] and list(r["docs_low"]) == [D] * K
        assert np.array_equal(r["allocation_ratio"], [0.0, 1.0, 0.0, 0.0])
        assert not r["near"]


def test_one_document_dominates():
    """Topic 1 lives in document 0 alone up to 1e-12: its entropy -> 0; a topic no document holds
    above `low` has allocation ratio NaN; skipped documents do not count."""
    gamma = np.array([[1.0] * 5, [1.0] + [1e-12] * 4, [1e-3] * 5])
    docs = [[(0, 5)], [(1, 5)], [], [(2, 5)], [(3, 0), (4, -1)]]
    r = dh.document_side(gamma, docs)
    assert r["num_docs"] == 3 and r["rank_1_docs"].sum() == 3
    assert 0 <= r["document_entropy"][1] <= 1e-9             # (2 x 1e-12 log(1e12) = 5.5e-11)
    assert 1.0 < r["document_entropy"][0] < np.log(LD(3))    # (p(d | 0) = 0.2, 0.4, 0.4)
    assert list(r["docs_low"]) == [3, 1, 0] and np.isnan(r["allocation_ratio"][2])
    assert dh.document_side(gamma[:, 2:3], docs[2:3]) is None


def test_ties_rank_the_smaller_topic():
    gamma = np.array([[2.0, 1.0], [5.0, 4.0], [5.0, 4.0], [1.0, 4.0]])
    r = dh.document_side(gamma, [[(0, 1)], [(0, 1)]])
    assert list(r["rank_1_docs"]) == [0, 2, 0, 0] and not r["near"]
    # a pair that differs by less than the bound is reported, an exact tie is not
    gamma[2, 0] = 5.0 * (1 - 2.0 ** -52)
    assert dh.document_side(gamma, [[(0, 1)], [(0, 1)]])["near"] == [(0, 1, "rank")]
    # theta exactly at a threshold is reported
    r = dh.document_side(np.array([[1.0], [1.0]]), [[(0, 1)]], high=0.5, low=0.25)
    assert r["near"] == [(0, 0, "high"), (0, 1, "high")] and list(r["docs_high"]) == [0, 0]


@pytest.mark.parametrize("K", dh.DOC_TOPICS)
def test_gpu_inputs_have_an_empty_near_list(K):
    """The documents and gammas of tests/test_gpu_diagnostics.py: nothing near a threshold or a
    rank tie, rank_1_docs sums to num_docs, sum_k tokens is the corpus' token count to 1e-12, and
    the device-order fp64 token sums agree with the longdouble ones to (B + K + 4) u."""
    docs, g = dh.documents(), dh.gammas(K)
    counted = [sum(c for _, c in d if c > 0) for d in docs]
    for by_length in (True, False):
        r = dh.document_side(g, docs, weight_by_length=by_length)
        assert not r["near"], r["near"]
        assert r["num_docs"] == sum(1 for n in counted if n > 0) == dh.DOC_B - 2
        assert r["rank_1_docs"].sum() == r["num_docs"]
        total = sum(counted) if by_length else r["num_docs"]
        assert abs(r["tokens"].sum() - total) <= 1e-12 * total
        assert np.all(r["docs_high"] <= r["docs_low"]) and r["docs_high"].sum() > 0
        dev = dh.tokens_device_order(g, docs, by_length)
        assert np.max(np.abs(dev.astype(LD) - r["tokens"]) / r["tokens"]) <= (dh.DOC_B + K + 4) * dh.U
        want = vh.prevalence(g, docs, by_length)
        assert np.max(np.abs(dh.normalise(dev).astype(LD) - want) / want) <= (dh.DOC_B + K + 8) * dh.U
    # the planted tie of document 5 ranks the smaller topic
    tied = np.nonzero(g[:, 5] == g[:, 5].max())[0]
    assert len(tied) == 2
    alone = dh.document_side(g[:, 5:6], docs[5:6])
    assert alone["rank_1_docs"][tied[0]] == 1
    # the E-step's own documents (no negative count) have the same shape
    assert [len(d) for d in dh.documents(negative=False)] == [len(d) for d in docs]


def test_entry_points_are_exported(hip_lib):
    from trlda_amd import _ffi
    for name in ("trlda_model_word_diagnostics", "trlda_topicdiag_create", "trlda_topicdiag_add",
                 "trlda_topicdiag_add_dev", "trlda_topicdiag_read", "trlda_topicdiag_destroy"):
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    from trlda_amd.models import LDA
    for name in ("topic_word_diagnostics", "topic_document_diagnostics", "topic_document_diagnostics_gamma",
                 "topic_diagnostics"):
        assert callable(getattr(LDA, name))
