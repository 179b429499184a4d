"""CPU checks of sampling documents: trlda_sample_lengths against the restatement (bitwise) and
the Poisson law, its error cases, the key draw, and the sampler restatement's own invariants."""
import ctypes
import math

import numpy as np
import pytest

import sample_host

KEYS = (0, 0x1234567890ABCDEF, 0x7FFFFFFF7FFFFFFF)


def _lengths(lib, B, length, key):
    indptr = np.full(B + 1, -7, dtype=np.int32)
    rc = lib.trlda_sample_lengths(B, float(length), key, indptr)
    return rc, indptr


@pytest.mark.parametrize("length", [0, 1, 7, 100, 745, 1000, 50000])
def test_lengths_match_the_restatement(hip_lib, length):
    for key in KEYS:
        B = 300 if length < 50000 else 40
        rc, indptr = _lengths(hip_lib, B, length, key)
        assert rc == 0, hip_lib.trlda_last_error()
        assert np.array_equal(indptr, sample_host.lengths(B, length, key)), (length, key)
        if length == 0:
            assert (indptr == 0).all()


def test_lengths_follow_the_poisson_law(hip_lib):
    B, lam = 20000, 7.0
    rc, indptr = _lengths(hip_lib, B, lam, 0xC0FFEE)
    assert rc == 0
    n = np.diff(indptr)
    assert (n >= 0).all()
    hi = 18                                                 # bins 0 .. 17 and a tail bin
    obs = np.bincount(np.minimum(n, hi), minlength=hi + 1).astype(np.float64)
    pmf = np.array([math.exp(-lam + k * math.log(lam) - math.lgamma(k + 1)) for k in range(hi)])
    exp_ = B * np.append(pmf, 1.0 - pmf.sum())
    chi2 = float(((obs - exp_) ** 2 / exp_).sum())
    df = hi
    assert chi2 < df + 8 * math.sqrt(2 * df), chi2        # a fixed key: deterministic
    assert abs(n.mean() - lam) < 5 * math.sqrt(lam / B)


def test_lengths_beyond_the_product_method(hip_lib):
    # the reference's Knuth product underflows from exp(-745) on; inversion does not
    for lam in (745.0, 5000.0):
        rc, indptr = _lengths(hip_lib, 2000, lam, 99)
        assert rc == 0
        n = np.diff(indptr)
        assert abs(n.mean() - lam) < 5 * math.sqrt(lam / 2000)
        assert abs(n.var() / lam - 1) < 0.15


def test_lengths_errors(hip_lib):
    from trlda_amd import _ffi
    for B, length in ((3, -1.0), (3, float("nan")), (3, float("inf")), (-1, 5.0)):
        rc, _ = _lengths(hip_lib, max(B, 0), length, 1) if B >= 0 else \
            (hip_lib.trlda_sample_lengths(B, length, 1, np.zeros(1, dtype=np.int32)), None)
        assert rc == _ffi.ERR_ARG, (B, length)
    # a total that does not fit in int32
    rc, _ = _lengths(hip_lib, 3000, 1.0e6, 5)
    assert rc == _ffi.ERR_ARG
    assert b"32 bits" in hip_lib.trlda_last_error()
    rc, indptr = _lengths(hip_lib, 0, 1.0e12, 5)             # no documents: nothing to overflow
    assert rc == 0 and indptr[0] == 0


def test_draw_key_takes_two_draws_of_the_seeded_stream(hip_lib):
    import trlda_amd
    libc = ctypes.CDLL("libc.so.6")
    key = ctypes.c_uint64()
    trlda_amd.seed(1234)
    assert hip_lib.trlda_rng_draw_key(ctypes.byref(key)) == 0
    first = key.value
    assert hip_lib.trlda_rng_draw_key(ctypes.byref(key)) == 0
    second = key.value
    libc.srand(1234)
    r = [libc.rand() for _ in range(4)]
    assert first == r[0] | (r[1] << 32)
    assert second == r[2] | (r[3] << 32)


def test_restatement_invariants():
    key = 0xABCDEF
    rng = np.random.RandomState(1)
    K, V, B = 5, 9000, 40
    lam = rng.gamma(0.5, 1.0, size=(K, V))
    lam[0, :4000] = 0.0
    C = sample_host.beta_table(lam, key)
    assert (np.diff(C, axis=1) >= 0).all()
    assert (C[0, :4000] == 0).all()
    th = sample_host.theta(np.full(K, 0.3), B, key)
    assert np.allclose(th.sum(axis=0), 1.0, atol=1e-12) and (th >= 0).all()
    indptr = sample_host.lengths(B, 20, key)
    w, z = sample_host.tokens(indptr, th, C, key)
    assert len(w) == indptr[-1] and (w >= 0).all() and (w < V).all()
    assert not ((z == 0) & (w < 4000)).any()                 # weight-0 words are never drawn
    # a prefix is a prefix: the first documents do not depend on B
    assert np.array_equal(sample_host.lengths(10, 20, key), indptr[:11])
    assert np.array_equal(sample_host.tokens(indptr[:11], th[:, :10], C, key)[0], w[:indptr[10]])
