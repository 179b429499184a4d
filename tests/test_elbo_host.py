"""CPU checks of tests/elbo_host.py, the restatement of the lower bound that the GPU tests
(test_gpu_lower_bound.py) hold trlda_model_lower_bound to: it equals the pinned oracle
(oracle_lower_bound with the column read of lda.cpp:334), the f11 fixture's recorded bounds, and
it tells the column read from the reference's row read by far more than its own tolerance."""
import numpy as np
import pytest

import elbo_host
from helpers import golden

RTOL = 1e-12          # of the sum of the absolute values of the addends


def _f11(sfx):
    f = golden("f11_lower_bound")
    B = len(f["indptr" + sfx]) - 1
    D = float(f["D"]) if sfx == "" else float(f["num_documents2"])
    args = (f["lam" + sfx], .1, .3, f["indptr" + sfx], f["ids" + sfx], f["cnts" + sfx],
            f["gamma_ref" + sfx], f["sstats_ref" + sfx])
    return f, args, D / B


def _case(K, V, B, seed, mean=20, alpha=None, eta=.3):
    rng = np.random.RandomState(seed)
    lam = rng.gamma(100., 1. / 100., size=(K, V)) * np.exp(rng.uniform(-2, 3, size=(K, 1)))
    n = rng.poisson(mean, size=B)
    n[0] = max(n[0], 1)
    indptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    ids = rng.randint(0, V, size=indptr[-1]).astype(np.int32)
    cnts = rng.randint(0, 7, size=indptr[-1]).astype(np.int32)
    if alpha is None:
        alpha = rng.uniform(.05, .5, size=K)
    gamma = rng.gamma(2., 3., size=(K, B)) + 1e-3
    sstats = rng.gamma(.3, 2., size=(K, V)) * (rng.uniform(size=(K, V)) < .3)
    return (np.asfortranarray(lam), alpha, eta, indptr, ids, cnts, np.asfortranarray(gamma),
            np.asfortranarray(sstats))


@pytest.mark.parametrize("sfx", ["", "2"])
def test_f11_against_the_oracle_and_the_fixture(oracle, sfx):
    f, args, factor = _f11(sfx)
    t = elbo_host.terms(*args)
    got, sc = elbo_host.bound(t, factor), elbo_host.scale(t, factor)
    want = oracle.lower_bound(*args, factor=factor)
    assert abs(got - want) <= RTOL * sc, (got, want, sc)
    rec = float(f["elbo_oracle" + sfx])
    assert abs(got - rec) <= RTOL * sc, (got, rec)
    if sfx == "":
        # Hoffman's approx_bound (onlineldavb.py) on the same gamma: another program, the same sum
        hof = float(f["elbo_hoffman"])
        assert abs(got - hof) <= 1e-12 * sc, (got, hof)
    # the row read of lda.cpp:334 is visible far above the tolerance
    slip = oracle.lower_bound(*args, factor=factor, reference_indexing=True)
    assert abs(slip - got) > 1e4 * RTOL * sc, (slip, got, sc)
    assert abs(slip - float(f["elbo_ref" + sfx])) < 1e-10 * abs(slip)


@pytest.mark.parametrize("K,V,B", [(1, 40, 6), (2, 50, 9), (7, 300, 12), (33, 120, 5),
                                   (64, 500, 10), (129, 700, 4), (300, 400, 3)])
def test_random_cases_against_the_oracle(oracle, K, V, B):
    args = _case(K, V, B, seed=K * 1000 + V)
    t = elbo_host.terms(*args)
    for factor in (1.0, 3.7, 0.0):
        want = oracle.lower_bound(*args, factor=factor)
        got, sc = elbo_host.bound(t, factor), elbo_host.scale(t, factor)
        assert abs(got - want) <= RTOL * sc, (K, factor, got, want, sc)
    # the dense term alone is the bound at factor 0; the slope is the batch part
    assert elbo_host.bound(t, 0.0) == t["dense"]
    slope = (oracle.lower_bound(*args, factor=3.7) - oracle.lower_bound(*args, factor=1.0)) / 2.7
    assert abs(slope - elbo_host.batch_part(t)) <= 1e-11 * t["scale_batch"] + RTOL * t["scale_dense"]
    if K > 1:
        slip = oracle.lower_bound(*args, reference_indexing=True)
        assert abs(slip - elbo_host.bound(t)) > 1e3 * RTOL * elbo_host.scale(t)


def test_edges_against_the_oracle(oracle):
    """empty documents, zero counts, repeated ids, a wide spread of lambda, eta at both ends"""
    K, V = 5, 30
    rng = np.random.RandomState(4)
    lam = np.asfortranarray(np.exp(rng.uniform(np.log(1e-3), np.log(1e4), size=(K, V))))
    indptr = np.array([0, 0, 4, 4, 9], np.int32)
    ids = np.array([3, 3, 7, 29, 0, 0, 0, 11, 3], np.int32)
    cnts = np.array([2, 1, 0, 5, 1, 0, 3, 2, 1], np.int32)
    gamma = np.asfortranarray(rng.gamma(1., 2., size=(K, 4)) + 1e-3)
    sstats = np.asfortranarray(rng.gamma(.5, 1., size=(K, V)))
    alpha = np.array([.01, .1, 1., 2., 5.])
    for eta in (1e-3, .3, 10.):
        args = (lam, alpha, eta, indptr, ids, cnts, gamma, sstats)
        t = elbo_host.terms(*args)
        for factor in (1.0, 2.5):
            want = oracle.lower_bound(*args, factor=factor)
            assert abs(elbo_host.bound(t, factor) - want) <= RTOL * elbo_host.scale(t, factor)


def test_documents_without_entries_add_only_their_theta_terms():
    """a document of length 0 adds ptheta and the :355 constant, nothing to pz"""
    args = list(_case(4, 20, 3, seed=8))
    t = elbo_host.terms(*args)
    indptr = args[3]
    ip2 = np.concatenate([indptr[:2], indptr[1:]]).astype(np.int32)      # an empty 2nd document
    g2 = np.asfortranarray(np.insert(args[6], 1, args[6][:, 0], axis=1))
    t2 = elbo_host.terms(args[0], args[1], args[2], ip2, args[4], args[5], g2, args[7])
    assert t2["pz"] == t["pz"] and t2["dense"] == t["dense"] and t2["s_term"] == t["s_term"]
    assert t2["ptheta_const"] == t["ptheta_const"] * 4 / 3
