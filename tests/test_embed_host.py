"""The restatement of the map of an indexed corpus (tests/embed_host.py) on the CPU: its gradient
against torch.autograd's gradient of its own KL, the calibration's contract and its two limit rows,
the symmetrisation, the planted groups the GPU is later asked to separate, and the gain decisions of
the trajectory cases in float64 and longdouble."""
import numpy as np
import pytest

import docindex_host as dh
import embed_host as eh

U = eh.U


def _rows(N, seed, measure="hellinger"):
    gamma, group = eh.planted(N, seed)
    return dh.rows(gamma, measure), group


def test_gradient_is_the_derivative_of_the_kl():
    """grad = 4 (A - R / Z) is d KL / d Y for a symmetric P that sums to 1.  Both sides are float64
    evaluations of the same sums in different orders; the bar is the gradient bound itself (and the KL
    bound for the value), though each side alone may use all of it."""
    import torch
    rows, _ = _rows(60, 3)
    P = eh.affinities(rows, 8.0)
    for scale in (1e-4, 1.0, 30.0):
        Y = np.random.RandomState(11).normal(0.0, scale, size=(60, 2))
        grad, kl, parts = eh.gradient(Y, P, parts=True)
        y = torch.tensor(Y, dtype=torch.float64, requires_grad=True)
        Pt = torch.tensor(P, dtype=torch.float64)
        one = 1.0 + ((y[:, None, :] - y[None, :, :]) ** 2).sum(dim=2)
        q = (1.0 / one) * (1.0 - torch.eye(60, dtype=torch.float64))
        hit = Pt > 0
        loss = (Pt[hit] * torch.log(Pt[hit] * q.sum() * one[hit])).sum()
        loss.backward()
        bound = eh.gradient_bound(60, parts)
        err = np.abs(grad - y.grad.numpy())
        print("scale %g: worst share of the bar %.3f, kl %.6f vs %.6f" % (scale, float((err / bound).max()), kl,
                                                                         float(loss.detach())))
        assert np.all(err <= bound)
        assert abs(float(loss.detach()) - kl) <= eh.kl_bound(60, parts)


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("perplexity", [1.0, 5.0, 30.0, 33.0])
def test_calibrated_rows(dtype, perplexity):
    rows, _ = _rows(120, 5)
    k = min(119, int(3 * perplexity))
    ids, s, _ = eh.knn(rows, k)
    D = eh.distances(s)
    p, beta = eh.calibrate(D, perplexity, dtype)
    assert np.all(np.abs(p.sum(axis=1) - 1) <= (2 * k + 1) * U)
    d = eh.offsets(D).astype(np.longdouble)
    for i in range(120):
        if not (0 < beta[i] < np.inf):
            continue
        H = eh.entropy(np.longdouble(beta[i]), d[i])[0]
        slack = abs(float(eh.entropy_slope(np.longdouble(beta[i]), d[i]))) * float(beta[i]) * 2.0 ** -49
        assert abs(float(H - np.log(np.longdouble(perplexity)))) <= slack + eh.entropy_bound(k, beta[i], d[i])


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_limit_rows(dtype):
    # k <= perplexity: uniform over the k neighbours, beta 0
    p, beta = eh.calibrate_row(np.array([.1, .2, .3, .4]), 5.0, dtype)
    assert beta == 0 and np.array_equal(p, np.full(4, dtype(1) / dtype(4)))
    p, beta = eh.calibrate_row(np.array([.1, .2, .3, .4]), 4.0, dtype)
    assert beta == 0
    # the m nearest exactly tied, m >= perplexity: uniform over those m, beta +inf
    D = np.array([.2] * 6 + [.3, .5, .9, .95])
    p, beta = eh.calibrate_row(D, 5.5, dtype)
    assert beta == np.inf and np.array_equal(p, np.where(D == .2, dtype(1) / dtype(6), 0))
    # tied but fewer than the perplexity: an ordinary row
    p, beta = eh.calibrate_row(D, 7.0, dtype)
    assert 0 < beta < np.inf and p[0] == p[5] > p[6] > p[9] > 0


def test_symmetrisation():
    from trlda_amd.index import _symmetrise
    rows, _ = _rows(90, 9)
    ids, s, _ = eh.knn(rows, 15)
    p, _ = eh.calibrate(eh.distances(s), 5.0)
    P = eh.symmetrise(ids, p)
    assert np.array_equal(P, P.T) and abs(P.sum() - 1) <= (2 * 15 + 64) * U
    indptr, cols, val = _symmetrise(ids, p)
    assert indptr[0] == 0 and indptr[-1] == len(cols) == len(val)
    for i in range(90):
        assert np.all(np.diff(cols[indptr[i]:indptr[i + 1]]) > 0)           # ascending id within a row
    assert np.array_equal(eh.dense(indptr, cols, val), P)
    # an empty graph
    indptr, cols, val = _symmetrise(np.empty((1, 0), dtype=np.int64), np.empty((1, 0)))
    assert list(indptr) == [0, 0] and len(cols) == len(val) == 0


@pytest.mark.parametrize("N,perplexity", [(150, 10.0), (300, 10.0), (90, 5.0)])
def test_planted_groups_come_apart(N, perplexity):
    rows, group = _rows(N, 40 + N)
    Y, kl = eh.embed(rows, perplexity, 500)
    purity, between, within = eh.separation(Y, group)
    print("N = %d: purity %.3f, centroids %.1f apart, members within %.1f" % (N, purity, between, within))
    assert purity == 1.0
    assert between > 2 * within
    assert kl[-1] < kl[250]


@pytest.mark.parametrize("N", eh.TRAJECTORY_SIZES)
def test_gain_decisions_agree_between_the_precisions(N):
    gamma, Y0 = eh.trajectory_case(N)
    rows = dh.rows(gamma)
    P = eh.affinities(rows, eh.TRAJECTORY_PERPLEXITY, np.longdouble)
    _, _, same64, _ = eh.loop(Y0, P.astype(np.float64), trace=True, **eh.TRAJECTORY)
    Yl, _, samel, _ = eh.loop(Y0, P.astype(np.float64), dtype=np.longdouble, trace=True, **eh.TRAJECTORY)
    Y64 = eh.loop(Y0, P.astype(np.float64), **eh.TRAJECTORY)[0]
    for a, b in zip(same64, samel):
        assert np.array_equal(a, b)
    E = float(np.max(np.abs(Y64 - Yl)) / np.max(np.abs(Yl)))
    print("N = %d: float64 vs longdouble after 5 iterations: %.2e of the extent" % (N, E))
    assert E < 1e-12
