"""The NumPy restatement of the query-likelihood search (tests/querylik_host.py) against a brute-force
triple loop, and its edges: the empty query, a word no topic of a document gives any probability,
and the per-word form."""
import math

import numpy as np

import querylik_host as qh

LAM = np.array([[4.0, 1.0, 0.5, 2.0, 0.5],
                [0.25, 3.0, 3.0, 0.5, 1.25],
                [1.0, 1.0, 1.0, 1.0, 4.0]])
THETA = np.array([[0.7, 0.2, 0.1],
                  [0.1, 0.8, 0.1],
                  [0.3, 0.3, 0.4],
                  [0.05, 0.05, 0.9]])
QUERIES = [[(0, 2)], [(1, 1), (2, 3)], [(4, 1), (0, 1), (3, 2)], []]


def _brute(theta, lam, queries):
    out = np.zeros((len(queries), theta.shape[0]))
    for b, query in enumerate(queries):
        for d in range(theta.shape[0]):
            s = 0.0
            for w, c in query:
                p = 0.0
                for k in range(lam.shape[0]):
                    p += theta[d, k] * lam[k, w] / sum(lam[k])
                s += c * (math.log(p) if p > 0 else -math.inf)
            out[b, d] = s
    return out


def test_against_the_triple_loop():
    want = _brute(THETA, LAM, QUERIES)
    got = qh.scores(THETA, LAM, QUERIES)
    assert got.dtype == np.longdouble and got.shape == (4, 4)
    assert np.allclose(got.astype(np.float64), want, rtol=1e-14, atol=0)
    assert np.allclose(qh.word_rows(LAM).sum(axis=1).astype(np.float64), 1.0, rtol=1e-15)
    ids, s, gap = qh.search(THETA, LAM, QUERIES, 2)
    for b in range(3):
        order = sorted(range(4), key=lambda d: (-want[b, d], d))
        assert list(ids[b]) == order[:2]
        assert np.allclose(s[b].astype(np.float64), want[b, order[:2]], rtol=1e-14)
        ranked = want[b, order]
        assert abs(gap[b] - min(ranked[0] - ranked[1], ranked[1] - ranked[2])) < 1e-14
    # word 0 belongs to topic 0: the document that holds most of topic 0 explains it best
    assert ids[0, 0] == 0


def test_the_empty_query():
    ids, s, gap = qh.search(THETA, LAM, QUERIES, 3)
    assert np.all(s[3] == 0.0) and list(ids[3]) == [0, 1, 2] and gap[3] == 0.0
    assert np.all(qh.scores(THETA, LAM, [[]]) == 0.0)
    # a count of 0 adds nothing
    assert np.array_equal(qh.scores(THETA, LAM, [[(1, 0), (0, 2)]]), qh.scores(THETA, LAM, [[(0, 2)]]))


def test_no_probability_is_minus_infinity_and_ranks_last():
    lam = LAM.copy()
    lam[1:, 0] = 0.0                                     # word 0 has its mass in topic 0 alone
    theta = THETA.copy()
    theta[1] = [0.0, 0.6, 0.4]                           # documents 1 and 3 hold nothing of topic 0
    theta[3] = [0.0, 0.1, 0.9]
    ids, s, gap = qh.search(theta, lam, [[(0, 1)], [(0, 2), (1, 1)]], 4)
    for b in range(2):
        assert list(ids[b, 2:]) == [1, 3] and np.all(np.isneginf(s[b, 2:])) and np.all(np.isfinite(s[b, :2]))
        assert not np.any(np.isnan(s[b]))
    assert gap[0] == 0.0                                 # (the tie of the two -inf)
    # a query that does not hold word 0 is finite everywhere
    assert np.all(np.isfinite(qh.scores(theta, lam, [[(1, 1), (4, 2)]])))


def test_per_word_keeps_the_ranking():
    s = qh.scores(THETA, LAM, QUERIES)
    pw = qh.per_word(s, QUERIES)
    assert np.array_equal(qh.rank(pw), qh.rank(s))
    assert np.allclose((pw[2] * 4).astype(np.float64), s[2].astype(np.float64), rtol=1e-15)
    assert np.array_equal(pw[0] * 2, s[0]) and np.all(pw[3] == 0.0)
