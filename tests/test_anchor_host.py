"""The restatement of the spectral initialisation (tests/anchor_host.py) on its own, without a GPU:
on the planted separable inputs it selects exactly the planted anchors and recovers the planted
topics; the fixed-order sum, the projection and the co-occurrence loop are what they claim to be.

A near-tie -- a round whose winner leads the runner-up by less than 1e-9 relative -- is reported, not
failed: the device may then legitimately pick the other word.  No planted input the GPU tests use
(GPU_PLANTED) has one, which is asserted here, so there the anchors must agree."""
import numpy as np
import pytest

import anchor_host as ah

GPU_PLANTED = [(5, 60), (20, 500), (130, 600)]          # what tests/test_gpu_anchor.py runs
SIZES = [(3, 16)] + GPU_PLANTED + [(50, 1000)]


@pytest.mark.parametrize("K,V", SIZES)
def test_planted_anchors_are_selected(K, V):
    Q, beta, anchors = ah.planted(K, V)
    assert np.array_equal(Q, Q.T) and (Q >= 0).all() and abs(Q.sum() - 1) < 1e-12
    ids, score, runner, _ = ah.anchor_words(Q, K)
    ties = ah.near_ties(score, runner)
    margin = float(np.min((score - runner) / score))
    print("K=%d V=%d: smallest relative margin %.3g, near-ties %r" % (K, V, margin, ties))
    assert sorted(ids) == sorted(anchors)
    if (K, V) in GPU_PLANTED:
        assert not ties


def test_longdouble_scores_lie_within_the_bound_of_float64():
    """the recursion's bound holds between the restatement's own two precisions"""
    Q, _, _ = ah.planted(5, 60)
    i64, s64, r64, _ = ah.anchor_words(Q, 5)
    ild, sld, rld, bound = ah.anchor_words(Q, 5, dtype=np.longdouble)
    assert np.array_equal(i64, ild) and bound.shape == (2, 5)
    assert (np.abs(s64.astype(np.longdouble) - sld) <= bound[0]).all()
    assert (np.abs(r64.astype(np.longdouble) - rld) <= bound[1]).all()
    assert (bound[0] < 1e-9 * sld).all() and (bound[1] < 1e-9 * rld).all()


def test_recovery_reaches_the_planted_topics():
    Q, beta, anchors = ah.planted(5, 60)
    r, total = ah.row_sums(Q)
    W = ah.normalise(Q, r).astype(np.longdouble)
    ids = ah.anchor_words(Q, 5)[0]
    X, iters, gaps = ah.recover(W, ids, tol=1e-10, max_iter=5000)
    assert iters.max() < 5000 and (gaps <= 1e-10).all()
    assert (X >= 0).all() and np.abs(X.sum(axis=1) - 1).max() < 1e-15
    bh, pi = ah.topics_of(X, (r / total).astype(np.longdouble))
    tv = ah.total_variation(bh, beta, ids, anchors)
    print("total variation to the planted beta: %.3g" % tv)
    assert tv < 1e-5 and abs(float(pi.sum()) - 1) < 1e-12


def test_fixed_sum_and_projection():
    rng = np.random.RandomState(1)
    X = rng.rand(3, 700)
    s = ah.fixed_sum(X)
    assert np.allclose(s, X.sum(axis=1), rtol=1e-14) and s.shape == (3,)
    # by hand, row 0: the partial sums, then the folding
    p = [0.0] * 256
    for v in range(700):
        p[v % 256] += X[0, v]
    w = 128
    while w:
        for t in range(w):
            p[t] += p[t + w]
        w //= 2
    assert p[0] == s[0]
    Y = rng.randn(50, 7) * 2
    P = ah.project_simplex(Y)
    assert (P >= 0).all() and np.abs(P.sum(axis=1) - 1).max() < 1e-14
    # optimality: v - P = tau on the support, v <= tau off it
    for y, q in zip(Y, P):
        tau = (y - q)[q > 0]
        assert np.ptp(tau) < 1e-14 and (y[q == 0] <= tau.mean() + 1e-14).all()


def test_cooccurrence_is_the_plain_loop():
    from trlda_amd.documents import CSRDocuments
    docs = CSRDocuments([0, 3, 4, 4, 6], [1, 4, 2, 3, 0, 4], [2, 1, 3, 1, 1, 1])
    Q, df, wc, n, skipped, tokens = ah.cooccurrence([docs], 5)
    want = np.zeros((5, 5))
    for ids, c in (([1, 4, 2], [2, 1, 3]), ([0, 4], [1, 1])):
        m = sum(c)
        for i, ci in zip(ids, c):
            for j, cj in zip(ids, c):
                want[i, j] += float(ci * cj - (ci if i == j else 0)) / float(m * (m - 1))
    assert np.array_equal(Q, want) and np.array_equal(Q, Q.T)
    assert (n, skipped, tokens) == (2, 2, 8)
    assert df.tolist() == [1, 1, 1, 0, 2] and wc.tolist() == [1, 2, 3, 0, 2]
    assert abs(Q.sum() - n) < 1e-14
