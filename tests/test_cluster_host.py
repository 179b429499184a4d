"""The restatement of the document groups (tests/cluster_host.py) itself, without a GPU, on the shapes
and inputs of tests/test_gpu_cluster.py: its labels against a brute-force argmax, the objective never
rises, the loop converges within 50 updates, no cluster runs empty, and -- what the GPU tests rest on
-- no assignment of any run is closer than GAP_FLOOR to a different answer."""
import numpy as np
import pytest

import cluster_host as ch
import docindex_host as dh

LD = np.longdouble
GAP_FLOOR = 1e-9
MEASURES = ["hellinger", "cosine"]
KS = [1, 3, 15, 16, 17, 63, 65, 130]
NCS = [(300, 1), (300, 2), (300, 7), (300, 16), (300, 17), (300, 65), (1100, 5), (17, 17), (2, 2), (1, 1)]


def _gammas(K, n, seed):
    """n gamma columns: sparse-ish topic weights of very different totals (as test_gpu_topicdocs.py)."""
    rng = np.random.RandomState(seed)
    g = rng.gamma(0.3, 1.0, size=(K, n)) + 0.01
    return np.asfortranarray(g * rng.uniform(0.5, 40.0, size=n))


def case(K, N, C, measure):
    """(document rows N x K, initial centroid rows C x K) of one shape."""
    g = _gammas(K, 1100, 4000 + K)[:, :N]
    x = dh.rows(g, measure)
    ids = np.linspace(0, N - 1, C).astype(int)
    theta = x[ids] ** 2 if measure == "hellinger" else x[ids] / x[ids].sum(axis=1)[:, None]
    return x, dh.rows(theta.T, measure)


def test_assignment_is_the_brute_force_argmax():
    x, m = case(17, 300, 16, "cosine")
    labels, s, margin = ch.assign(x, m)
    for n in range(len(x)):
        v = [sum(LD(x[n, k]) * LD(m[c, k]) for k in range(x.shape[1])) for c in range(len(m))]
        best = 0
        for c in range(1, len(m)):
            if v[c] > v[best]:                               # (strictly: a tie stays with the smaller c)
                best = c
        second = max(v[c] for c in range(len(m)) if c != best)
        assert labels[n] == best
        assert abs(float(s[n] - v[best])) <= 1e-17 and abs(margin[n] - float(v[best] - second)) <= 1e-16


def test_exact_ties_go_to_the_smaller_cluster():
    x, m = case(15, 300, 7, "hellinger")
    m = np.vstack([m, m[2:3], m[0:1]])                       # clusters 7 and 8 repeat 2 and 0
    labels, _, margin = ch.assign(x, m)
    assert labels.max() <= 6 and np.all(margin[(labels == 2) | (labels == 0)] == 0.0)
    kept = ch.update(x, m, labels)
    assert np.array_equal(kept[7], m[7].astype(LD)) and np.array_equal(kept[8], m[8].astype(LD))
    assert ch.assign(x, np.ones((1, 15)) / np.sqrt(15.0))[2][0] == np.inf


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("N,C", NCS)
@pytest.mark.parametrize("K", KS)
def test_loop(K, N, C, measure):
    x, m = case(K, N, C, measure)
    run = ch.run(x, m, 50)
    assert run.converged and run.iterations <= 50
    assert len(run.labels) == run.iterations + 1 == len(run.objective)
    assert np.array_equal(run.labels[-1], run.labels[-2]) if run.iterations else True
    # an update and an assignment each lower the objective (or leave it) for centroids of length 1; the
    # initial rows are float64 rows, whose length is 1 within the (K + 16) u of their K roundings, and
    # that much of every s is all that may show
    slack = N * (K + 16) * 2.0 ** -53
    assert all(float(b - a) <= slack for a, b in zip(run.objective, run.objective[1:])), run.objective
    for j in range(len(run.labels)):
        assert run.sizes(j).sum() == N
        if K > 1:
            assert run.sizes(j).min() > 0, (j, run.sizes(j))  # (the initial centroids are documents)
    if K == 1:
        # (one topic: every row is [1], every similarity 1, every label 0, nothing to separate)
        assert all(np.all(l == 0) for l in run.labels) and run.iterations == 1
        assert all(np.all(s == 1) for s in run.similarity)
    else:
        assert run.margin > GAP_FLOOR, run.margin
    # the loop stopped early is a prefix of the loop
    for max_iter in (0, 1, 2, 3):
        short = ch.run(x, m, max_iter)
        j, iterations, converged = run.after(max_iter)
        assert short.iterations == iterations and short.converged == converged
        assert np.array_equal(short.labels[-1], run.labels[j])
    # theta^ of the centroid rows are distributions
    theta = ch.theta_hat(run.rows[-1], measure)
    assert theta.shape == (K, C) and np.all(np.abs(theta.sum(axis=0) - 1) <= 1e-15)
