"""CPU checks of the Gibbs path: the restatement's Philox against Random123's known answers, the
exact-posterior enumerator against brute force, and the library's Gibbs entry points."""
import os

import numpy as np

import gibbs_host


def _words(ws):
    return ["%08x" % int(w) for w in ws]


def test_philox_known_answers():
    # Random123's kat_vectors for philox4x32_10
    out = gibbs_host.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert _words(out) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    out = gibbs_host.philox4x32_10(f, f, f, f, f, f)
    assert _words(out) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    out = gibbs_host.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert _words(out) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_philox_vectorised_matches_scalar():
    idx = np.arange(5)
    vec = gibbs_host.philox4x32_10(idx, 7, 3, gibbs_host.SWEEP, 11, 12)
    for i in idx:
        one = gibbs_host.philox4x32_10(int(i), 7, 3, gibbs_host.SWEEP, 11, 12)
        assert [int(w[i]) for w in vec] == [int(w) for w in one]


def test_uniform_mapping():
    assert gibbs_host.uniform(0, 0) == 0.0
    assert gibbs_host.uniform(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53
    assert gibbs_host.uniform_open(0, 0) == 2.0 ** -53
    assert 0.0 < gibbs_host.uniform_open(0xFFFFFFFF, 0xFFFFFFFF) < 1.0


def test_exact_posterior_matches_brute_force():
    rng = np.random.RandomState(3)
    K, V = 3, 4
    e = rng.uniform(0.1, 1.0, size=(K, V))
    e /= e.sum(axis=1, keepdims=True)
    alpha = np.array([0.3, 1.2, 0.05])
    words = [0, 2, 2, 3, 1]
    ecounts, etheta = gibbs_host.exact_posterior(e, alpha, words)
    pi = gibbs_host.sweep_stationary(e, alpha, words)
    import itertools
    states = np.array(list(itertools.product(range(K), repeat=len(words))))
    bc = np.zeros((K, V))
    for i, w in enumerate(words):
        for k in range(K):
            bc[k, w] += pi[states[:, i] == k].sum()
    n = np.stack([(states == k).sum(axis=1) for k in range(K)], axis=1)
    bt = ((alpha + n) / (alpha.sum() + len(words)) * pi[:, None]).sum(axis=0)
    assert np.allclose(ecounts, bc, rtol=0, atol=1e-10)
    assert np.allclose(etheta, bt, rtol=0, atol=1e-10)
    assert abs(ecounts.sum() - len(words)) < 1e-12


def test_restatement_invariants():
    rng = np.random.RandomState(5)
    K, V = 7, 30
    e = rng.uniform(0.01, 1.0, size=(K, V))
    alpha = np.full(K, 0.1)
    indptr = np.array([0, 3, 3, 6])
    ids = np.array([1, 4, 4, 9, 0, 29])
    cnts = np.array([2, 0, 3, 5, 1, 1])
    theta, counts, nfin = gibbs_host.gibbs(e, alpha, indptr, ids, cnts, None, 3, 2, 0x1234567890ABCDEF)
    assert counts.sum() == 3 * cnts.sum()
    assert np.allclose(theta.sum(axis=0), 1.0, atol=1e-12) and (theta >= 0).all()
    assert (nfin.sum(axis=0) == [5, 0, 7]).all()
    again = gibbs_host.gibbs(e, alpha, indptr, ids, cnts, None, 3, 2, 0x1234567890ABCDEF)
    assert (again[1] == counts).all() and (again[0] == theta).all()


def test_library_exports_gibbs():
    from trlda_amd import _ffi
    from trlda_amd.build import LIB_PATH
    assert os.path.exists(LIB_PATH)
    for name in ("trlda_model_gibbs", "trlda_model_gibbs_host", "trlda_gibbs"):
        assert name in _ffi.EXPORTED_SYMBOLS
        assert hasattr(_ffi.lib(), name)
    with open(os.path.join(os.path.dirname(LIB_PATH), "..", "include", "trlda_hip.h")) as f:
        header = f.read()
    for name in ("trlda_model_gibbs(", "trlda_model_gibbs_host(", "trlda_gibbs("):
        assert name in header
