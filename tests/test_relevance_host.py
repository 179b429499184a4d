"""CPU checks of the relevance / saliency / prevalence restatement (tests/relevance_host.py): the
identities of the contract and hand cases."""
import numpy as np

import relevance_host as vh

LD = np.longdouble


def _lam(K, V, seed=0):
    return np.random.RandomState(7000 + 13 * K + V + seed).gamma(2.0, 1.0, size=(K, V)) + 0.05


def test_weight_one_ranks_by_lambda():
    for K, V in ((1, 7), (3, 50), (20, 300)):
        lam = _lam(K, V)
        for pi in (None, np.random.RandomState(K).gamma(0.5, 1.0, K) + 0.01):
            ids, scores, gap = vh.relevant_words(lam, min(V, 10), 1.0, pi)
            for k in range(K):
                assert np.array_equal(ids[k], np.lexsort((np.arange(V), -lam[k]))[:min(V, 10)])
            assert ids.dtype == np.int32 and gap > 0
            beta = lam.astype(LD) / lam.astype(LD).sum(axis=1)[:, None]
            want = np.log(np.take_along_axis(beta, ids.astype(np.int64), axis=1))
            assert np.max(np.abs(scores - want)) <= 1e-17


def test_statistics_identities():
    for K, V in ((2, 9), (7, 120), (64, 300)):
        lam = _lam(K, V)
        for given in (None, np.random.RandomState(K + 1).gamma(0.5, 1.0, K) + 0.01):
            pi, R = vh.weights(lam, given)
            p, D, S, scale = vh.word_statistics(lam, given)
            assert abs(float(p.sum()) - 1.0) <= 1e-15
            assert np.all(D >= 0) and np.all(scale >= D)
            # the mutual information of topic and word from the joint P(k, w) = pi_k beta_kw
            joint = pi[:, None] * lam.astype(LD) / R[:, None]
            mi = (joint * (np.log(joint) - np.log(pi)[:, None] - np.log(p)[None, :])).sum()
            assert abs(float(S.sum() - mi)) <= 1e-15
            assert float(S.sum()) <= np.log(K)


def test_a_word_every_topic_holds_alike_is_not_distinctive():
    """Word 4 has beta = 1/9 in every topic (dyadic lambda, equal row sums): D = 0 under uniform
    weights, as for words 5 .. 8; the first four words are distinctive."""
    K, V = 4, 8
    lam = np.array([[8, 2, 1, 1, 1, 1, 1, 1],
                    [1, 8, 2, 1, 1, 1, 1, 1],
                    [1, 1, 8, 2, 1, 1, 1, 1],
                    [2, 1, 1, 8, 1, 1, 1, 1]], dtype=np.float64) / 16.0
    lam = np.concatenate([lam[:, :4], np.full((K, 1), 0.0), lam[:, 4:]], axis=1)
    lam[:, 4] = 1.0 / 8.0                                # the planted word; the rows now sum to 9/8 alike
    p, D, S, scale = vh.word_statistics(lam, np.full(K, 1.0))
    assert abs(float(D[4])) <= 1e-15 and abs(float(p[4]) - 1.0 / 9.0) <= 1e-15
    assert np.all(np.abs(D[5:]) <= 1e-15)                # (the four words of 1/16 everywhere too)
    assert D[:4].min() > 0.1


def test_planted_stop_word():
    """Word 3 is the largest of every topic: first everywhere at weight 1, nowhere at weight 0.3."""
    K, V, top_n = 6, 200, 10
    rng = np.random.RandomState(5)
    lam = np.full((K, V), 0.05)
    for k in range(K):                                   # each topic's own 30 words
        lam[k, 20 + 30 * k:50 + 30 * k] += rng.gamma(2.0, 1.0, 30) + 1.0
    lam[:, 3] = 9.0 + 0.01 * np.arange(K)
    assert np.all(lam[:, 3] > np.delete(lam, 3, axis=1).max(axis=1))
    ids1, _, _ = vh.relevant_words(lam, top_n, 1.0)
    assert np.all(ids1[:, 0] == 3)
    ids03, _, _ = vh.relevant_words(lam, top_n, 0.3)
    assert not np.any(ids03 == 3)
    for k in range(K):                                   # what takes its place is the topic's own
        assert np.all((ids03[k] >= 20 + 30 * k) & (ids03[k] < 50 + 30 * k))
    sal, _, _ = vh.salient_words(lam, 30)
    assert 3 not in sal


def test_rank_ties_and_gap():
    ids, scores, gap = vh.rank(np.array([0.5, 2.0, 0.5, 2.0, -1.0]), 4, relative=False)
    assert list(ids) == [1, 3, 0, 2] and gap == 0.0
    ids, scores, gap = vh.rank(np.array([1.0, 4.0, 2.0]), 2, relative=True)
    assert list(ids) == [1, 2] and abs(gap - 0.5) <= 1e-18          # (4-2)/4 and (2-1)/2
    assert vh.rank(np.array([3.0]), 1, relative=True)[2] == np.inf


def test_prevalence_by_hand():
    """Two documents: theta_0 = (1/4, 3/4) with 3 + 1 = 4 tokens (the count 0 and the count -2 do
    not count), theta_1 = (1/2, 1/2) with 2 tokens; an empty one and one with counts <= 0 between."""
    gamma = np.array([[1.0, 9.0, 5.0, 2.0], [3.0, 1.0, 5.0, 2.0]])
    docs = [[(0, 3), (4, 0), (2, 1), (1, -2)], [], [(3, 0), (1, -1)], [(5, 2)]]
    pi = vh.prevalence(gamma, docs)
    want = np.array([4 * 0.25 + 2 * 0.5, 4 * 0.75 + 2 * 0.5]) / 6.0
    assert np.max(np.abs(pi.astype(np.float64) - want)) <= 1e-16
    pi = vh.prevalence(gamma, docs, weight_by_length=False)
    assert np.max(np.abs(pi.astype(np.float64) - [0.375, 0.625])) <= 1e-16
    assert vh.prevalence(gamma[:, 1:3], docs[1:3]) is None
