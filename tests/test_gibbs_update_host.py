"""Invariants of the NumPy restatement of the Gibbs update loops (tests/gibbs_update_host.py).
CPU only."""
import math

import numpy as np
import pytest

import gibbs_update_host as gu


def _psi(x):
    # digamma by recurrence and the asymptotic series (enough for these invariants; the GPU
    # parity tests use the oracle's)
    r = 0.0
    while x < 6.0:
        r -= 1.0 / x
        x += 1.0
    f = 1.0 / (x * x)
    return r + math.log(x) - 0.5 / x - f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f / 240)))


def _case(K=4, V=12, B=5, seed=0):
    rng = np.random.RandomState(seed)
    lam = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    docs = [[(int(rng.randint(V)), int(rng.randint(1, 4))) for _ in range(rng.randint(1, 5))]
            for _ in range(B)]
    alpha = np.full(K, 0.1)
    return lam, alpha, docs


@pytest.mark.parametrize("T", [0, 1, 3])
def test_no_samples_blends_to_eta(T):
    """num_samples = 0: no statistics, so lambda = (1 - rho) lambda' + rho eta on every column."""
    lam, alpha, docs = _case()
    rho, eta = 0.3, 0.2
    out, sstats, theta, _, _ = gu.online(lam, alpha, eta, docs, 100, rho, T, True, 0, 2,
                                      [11, 12, 13], _psi)
    assert not sstats.any()
    assert np.allclose(out, (1. - rho) * lam + rho * eta, rtol=1e-15, atol=0)
    assert np.allclose(theta.sum(axis=0), 1.0)


@pytest.mark.parametrize("epochs,ns", [(1, 1), (3, 1), (2, 3)])
def test_batch_mass_balance(epochs, ns):
    """lambda = eta + sstats, and every token adds num_samples x 1 / num_samples: the total is
    K V eta + tokens."""
    lam, alpha, docs = _case(seed=epochs)
    K, V = lam.shape
    eta = 0.3
    out, sstats, _, _, _ = gu.batch(lam, alpha, eta, docs, epochs, ns, 1, [5, 6, 7], _psi)
    tokens = sum(c for d in docs for _, c in d)
    assert math.isclose(out.sum(), K * V * eta + tokens, rel_tol=1e-12)
    assert math.isclose(sstats.sum(), tokens, rel_tol=1e-12)


def test_words_outside_the_batch_get_the_final_value_once():
    lam, alpha, docs = _case(V=30, seed=4)
    rho, eta = 0.25, 0.1
    out, _, _, _, _ = gu.online(lam, alpha, eta, docs, 1000, rho, 2, False, 1, 1, [1, 2], _psi)
    outside = np.setdiff1d(np.arange(lam.shape[1]), [w for d in docs for w, _ in d])
    assert len(outside)
    assert np.array_equal(out[:, outside], (1. - rho) * lam[:, outside] + rho * (eta + 0.0))


def test_same_keys_same_result_other_keys_differ():
    lam, alpha, docs = _case(seed=7)
    a = gu.online(lam, alpha, 0.3, docs, 100, 0.5, 2, True, 1, 2, [3, 4], _psi)[0]
    b = gu.online(lam, alpha, 0.3, docs, 100, 0.5, 2, True, 1, 2, [3, 4], _psi)[0]
    c = gu.online(lam, alpha, 0.3, docs, 100, 0.5, 2, True, 1, 2, [3, 5], _psi)[0]
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)


@pytest.mark.parametrize("x,want", [(1.0, math.pi ** 2 / 6), (0.5, math.pi ** 2 / 2),
                                    (2.0, math.pi ** 2 / 6 - 1.0)])
def test_trigamma_known_values(x, want):
    assert math.isclose(gu.trigamma(x), want, rel_tol=1e-14)


def test_trigamma_recurrence_across_the_series_threshold():
    """psi'(x) - psi'(x + 1) = 1 / x^2, with x + 1 taken by the asymptotic series and x by one
    step of the recurrence (and both by the series further out)."""
    for x in (19.25, 19.5, 20.0, 40.0, 900.0):
        assert math.isclose(gu.trigamma(x) - gu.trigamma(x + 1.0), 1.0 / (x * x), rel_tol=1e-11)
    assert math.isclose(gu.trigamma(1e6), 1e-6 + 0.5e-12, rel_tol=1e-12)


def test_eta_step_moves_towards_the_stationary_point():
    """g = 0 at the eta that maximises the bound for this lambda: a step of rho = 1 from either
    side moves eta the right way, and a lambda of all eta is (nearly) at rest only when the
    statistics are zero."""
    rng = np.random.RandomState(3)
    lam = 0.2 + rng.gamma(0.5, 0.1, size=(5, 40))
    lo, hi = gu.eta_step(lam, 0.05, 1.0, _psi), gu.eta_step(lam, 5.0, 1.0, _psi)
    assert lo > 0.05 and hi < 5.0
    assert gu.eta_step(lam, 0.05, 0.0, _psi) == 0.05
    assert gu.eta_step(lam, 1e-7, 1.0, _psi, min_eta=1e-3) >= 1e-3


def test_adaptive_first_steps():
    a = gu.Adaptive((2, 3))
    assert a.rho == 1e-3
    upd = np.arange(6.0).reshape(2, 3)
    a.step(upd + 1.0, np.ones((2, 3)))
    t = 1000.
    sq = (1 - 1 / t) + np.sum(upd ** 2) / t
    assert math.isclose(a.sq_norm, sq, rel_tol=1e-15)
    assert math.isclose(a.rho, np.sum((upd / t) ** 2) / sq, rel_tol=1e-14)
    assert math.isclose(a.tau, t * (1 - a.rho) + 1, rel_tol=1e-15)
    # a constant update direction drives rho up
    r0 = a.rho
    for _ in range(50):
        a.step(upd + 1.0, np.ones((2, 3)))
    assert a.rho > r0
