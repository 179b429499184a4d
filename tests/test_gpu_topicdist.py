"""LDA.topic_distances and LDA.match_topics on the GPU (csrc/topicdist_kernels.h):
every measure against the longdouble restatement (tests/topicdist_host.py) within a bound derived from
the arithmetic, the model against itself, the forms of `other`, determinism, the matching, the models'
state and the errors.

The bound.  With U = 2^-53 every entry must satisfy |device - restatement| <= (V + 16) 2 U A_ij, A_ij
being the sum of the absolute values of the terms of the sum the device forms: any order of n additions
errs by at most (n - 1) U sum|terms| to first order, each term carries about 2 U of its own (the square
root or logarithm, the product, the scaling), and the factor 2 and the + 16 cover that and the closing
formula.  It is not fitted to what the device gives.

    hellinger       compared as d^2 against 1 - BC (the root near 0 would amplify the error), A = BC,
                    4 U added for the squaring
    cosine          compared as d against 1 - c with (V + 16) 4 U c
    kl              the device forms (sum lambda log lambda - sum lambda log mu) / S - log S + log T:
                    A = (1/S) sum lambda (|log lambda| + |log mu|) + |log S| + |log T|
    jensen_shannon  A = H(m) + H(p) / 2 + H(q) / 2.  The device adds the -m log m (positive terms: H(m)
                    is its own sum of absolute values) and takes H(p) = log S - sum lambda log lambda / S
                    from the row statistics; the bound is kept as the definition's A, which is the
                    smaller of the two and so asks no less.

Every array is small: the largest case is 65 x 100 topics of 1031 words; the restatement of a case is
computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import topicdist_host as th

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LN2 = float(np.log(2.0))
MEASURES = list(th.MEASURES)
SYMMETRIC = ["hellinger", "cosine", "jensen_shannon"]
CASES = [(1, 1, 1), (3, 5, 3), (15, 17, 33), (16, 16, 64), (37, 21, 1500), (65, 100, 1031), (130, 64, 257)]


@pytest.fixture(scope="module")
def hip():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


def _lambda(K, V, seed):
    return np.random.RandomState(seed).gamma(0.3, 1.0, (K, V)) * \
        np.random.RandomState(seed).uniform(0.5, 40, (K, 1)) + 0.01


@functools.lru_cache(maxsize=None)
def _inputs(K, K2, V):
    """(lambda K x V, mu K2 x V): the first min(K, K2) // 2 topics of mu are near-duplicates of lambda's."""
    lam, mu = _lambda(K, V, 1000 + K + V), _lambda(K2, V, 2000 + K2 + V)
    n = min(K, K2) // 2
    mu[:n] = lam[:n] * np.exp(0.05 * np.random.RandomState(3000 + V).standard_normal((n, V)))
    lam, mu = np.asfortranarray(lam), np.asfortranarray(mu)
    lam.flags.writeable = mu.flags.writeable = False
    return lam, mu


@functools.lru_cache(maxsize=None)
def _ref(K, K2, V):
    return th.distances(*_inputs(K, K2, V))


@functools.lru_cache(maxsize=None)
def _ref_self(K, V):
    lam = _inputs(K, K, V)[0]
    return th.distances(lam, lam)


def _model(lam, cls=None, alpha=.1, eta=.3):
    """A model holding `lam` without the constructor's K V 100 draws."""
    from trlda_amd.models import OnlineLDA
    cls = cls or OnlineLDA
    m = cls.__new__(cls)
    if cls is OnlineLDA:
        m._num_documents = 1000
        m._update_count = 0
        m._ada_tau = 1000.
        m._ada_rho = 1. / m._ada_tau
        m._ada_sq_norm = 1.
    m._setup(lam.shape[1], lam.shape[0], alpha, eta, None, _lambda=np.asfortranarray(lam))
    return m


def _forced_chunk(V):
    """Words per chunk giving at least 5 chunks with a ragged last one -- where V allows it: below 11
    words there is no such cut and every word is a chunk of its own."""
    for w in range(V // 5, 1, -1):
        if V % w and -(-V // w) >= 5:
            return w
    return 1


def _within(measure, dev, ref, V, off_diagonal=False):
    """Asserts the bound of the module's docstring; returns the largest error / bound."""
    D, A = ref[measure]
    dev = dev.astype(np.longdouble)
    if measure == "hellinger":
        err, bound = np.abs(dev * dev - (1 - A)), (V + 16) * 2 * U * A + 4 * U
    elif measure == "cosine":
        err, bound = np.abs(dev - (1 - A[0])), (V + 16) * 4 * U * A[0]
    else:
        err, bound = np.abs(dev - D), (V + 16) * 2 * U * A
    if off_diagonal:
        err = err.copy()
        np.fill_diagonal(err, 0.0)
    bound = np.abs(bound)
    # (a bound of 0 -- the entropies of one-word topics -- admits an error of 0 only)
    ratio = np.where(err > bound, np.inf, err / np.where(bound > 0, bound, 1)).astype(np.float64)
    print("%s V = %d: max err %.3g, bound there %.3g, max err / bound %.3g"
          % (measure, V, float(err.ravel()[np.argmax(ratio)]), float(np.ravel(bound)[np.argmax(ratio)]),
             float(ratio.max())))
    assert np.all(ratio <= 1), (measure, float(ratio.max()))
    return float(ratio.max())


def _in_range(measure, D, shape):
    assert D.shape == shape and D.dtype == np.float64 and np.all(np.isfinite(D))
    assert np.all(D >= 0)
    if measure in ("hellinger", "cosine"):
        assert np.all(D <= 1)
    if measure == "jensen_shannon":
        assert np.all(D <= LN2)


def _buffers(hip):
    live, total = C.c_longlong(), C.c_longlong()
    assert hip.trlda_debug_device_buffers(C.byref(live), C.byref(total)) == 0
    return live.value, total.value


def _state():
    from trlda_amd import _ffi
    s = np.zeros(33, dtype=np.uint32)
    _ffi.lib().trlda_rng_get_state(s)
    return s


# 1. every measure, every shape, the automatic chunk and a forced one --------------------------------
@pytest.mark.parametrize("K,K2,V", CASES)
def test_against_the_restatement(hip, K, K2, V):
    from trlda_amd import _ffi
    lam, mu = _inputs(K, K2, V)
    ref = _ref(K, K2, V)
    a, b = _model(lam), _model(mu)
    for words in (0, _forced_chunk(V)):
        _ffi.check(hip.trlda_model_set_topicdist_chunk(a._handle, words))
        for measure in MEASURES:
            D = a.topic_distances(b, measure)
            _in_range(measure, D, (K, K2))
            assert D.flags.f_contiguous
            _within(measure, D, ref, V)
    b.close()
    a.close()


# 2. the model against itself ---------------------------------------------------------------------
def test_against_itself(hip):
    K, V = 37, 1500
    lam = _inputs(K, K, V)[0]
    ref = _ref_self(K, V)
    m = _model(lam)
    for measure in MEASURES:
        D = m.topic_distances(measure=measure)
        _in_range(measure, D, (K, K))
        assert np.all(np.diag(D) == 0) and not np.any(np.signbit(np.diag(D)))
        assert np.array_equal(m.topic_distances(m, measure), D)         # the model itself is None
        off = D[~np.eye(K, dtype=bool)]
        assert np.all(off > 0)
        _within(measure, D, ref, V, off_diagonal=True)
        if measure in SYMMETRIC:
            assert np.array_equal(D, D.T), measure
        else:
            assert np.sum(D != D.T) >= K * (K - 1) - 2                  # kl is not symmetric
    # a copy is another model: the general path, the diagonal near 0 and within the bound
    copy = _model(lam)
    for measure in MEASURES:
        D = m.topic_distances(copy, measure)
        _within(measure, D, ref, V)
        # (the bound at 0 is (V + 16) 2 U = 3.4e-13, for hellinger on d^2: d <= 5.8e-7)
        assert np.all(np.diag(D) <= (6e-7 if measure == "hellinger" else 1e-11))
    copy.close()
    m.close()


# 3. - 5. the forms of `other`, two calls, the subclasses ------------------------------------------
def test_forms_of_other_and_calls_agree_bitwise(hip):
    from trlda_amd.models import BatchLDA, CumulativeLDA
    K, K2, V = 37, 21, 1500
    lam, mu = _inputs(K, K2, V)
    a, b = _model(lam), _model(mu)
    batch_a, batch_b, cumulative_b = _model(lam, BatchLDA), _model(mu, BatchLDA), _model(mu, CumulativeLDA)
    held = np.asarray(b.lambdas)
    assert held.flags.f_contiguous and np.array_equal(held, mu)
    for measure in MEASURES:
        D = a.topic_distances(b, measure)
        assert np.array_equal(a.topic_distances(b, measure), D)                      # two calls
        assert np.array_equal(a.topic_distances(held, measure), D)                   # its lambdas
        c_ordered = np.ascontiguousarray(held)
        assert c_ordered.flags.c_contiguous and not c_ordered.flags.f_contiguous
        assert np.array_equal(a.topic_distances(c_ordered, measure), D)
        assert np.array_equal(a.topic_distances(held.tolist(), measure), D)          # array-like
        assert np.array_equal(a.topic_distances(batch_b, measure), D)                # OnlineLDA x BatchLDA
        assert np.array_equal(batch_a.topic_distances(b, measure), D)
        assert np.array_equal(batch_a.topic_distances(cumulative_b, measure), D)
        assert np.array_equal(a.topic_distances(b, measure.upper()), D)
    assert np.array_equal(a.topic_distances(b, "js"), a.topic_distances(b, "jensen_shannon"))
    assert np.array_equal(a.topic_distances(b), a.topic_distances(b, "hellinger"))   # the default
    for m in (a, b, batch_a, batch_b, cumulative_b):
        m.close()


# 6. padding never leaks --------------------------------------------------------------------------
@pytest.mark.parametrize("last", [(1e300, 1e300), (1e-300, 1e-300), (1e300, 1e-300)])
def test_extreme_last_word_stays_finite(hip, last):
    """A huge and a tiny last word column -- V = 33, so the column is staged alone next to 31 words of
    padding, and 15 x 17 topics leave padding in both directions of the one tile."""
    K, K2, V = 15, 17, 33
    lam, mu = (np.array(x) for x in _inputs(K, K2, V))
    lam[:, -1], mu[:, -1] = last
    a = _model(lam)
    for measure in ("hellinger", "jensen_shannon"):
        for other in (mu, None):
            D = a.topic_distances(other, measure)
            _in_range(measure, D, (K, K2 if other is not None else K))
    if last == (1e300, 1e300):
        # every topic is that word, to 1e-298: all distances are rounding
        assert np.all(a.topic_distances(mu, "hellinger") <= 1e-6)
        assert np.all(a.topic_distances(mu, "jensen_shannon") <= 1e-10)
    a.close()


# 7. the matching ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K,K2,V", [(37, 21, 1500), (16, 16, 5000)])
def test_match_topics(hip, K, K2, V):
    lam, mu = _inputs(K, K2, V)
    ref = _ref(K, K2, V)
    a, b = _model(lam), _model(mu)
    n = min(K, K2) // 2
    for measure in MEASURES:
        want_D = ref[measure][0].astype(np.float64)
        assert th.min_gap(want_D) > 1e-9, (measure, th.min_gap(want_D))
        want, _ = th.greedy_match(want_D)
        match, dist = a.match_topics(b, measure)
        assert match.dtype == np.int64 and dist.dtype == np.float64 and match.shape == dist.shape == (K,)
        assert np.array_equal(match, want), measure
        D = a.topic_distances(b, measure)
        paired = match >= 0
        assert np.array_equal(dist[paired], D[np.nonzero(paired)[0], match[paired]])
        assert np.array_equal(match[:n], np.arange(n))              # the near-duplicates, to their originals
        assert paired.sum() == min(K, K2) and len(set(match[paired])) == min(K, K2)
        assert np.all(match[~paired] == -1) and np.all(np.isinf(dist[~paired]))
        assert (~paired).sum() == max(0, K - K2)
        # an array as `other`
        m2, d2 = a.match_topics(np.asarray(b.lambdas), measure)
        assert np.array_equal(m2, match) and np.array_equal(d2, dist)
    b.close()
    a.close()


# 8. state ----------------------------------------------------------------------------------------
def test_state_is_left_alone_and_buffers_are_returned(hip):
    import trlda_amd
    K, K2, V = 15, 17, 33
    lam, mu = _inputs(K, K2, V)
    live0, total0 = _buffers(hip)
    a, b = _model(lam, alpha=.2), _model(mu)
    live1, total1 = _buffers(hip)
    trlda_amd.seed(9)
    state = _state()
    for measure in MEASURES:
        for other in (None, b, mu):
            a.topic_distances(other, measure)
        a.match_topics(b, measure)
    assert _buffers(hip)[0] == live1                     # every temporary went with its call
    assert _buffers(hip)[1] >= total1 + 4 * 4 * 4        # ... and was a counted buffer
    assert np.array_equal(state, _state())
    for m, want in ((a, lam), (b, mu)):
        assert np.array_equal(np.asarray(m.lambdas), want)
    assert np.array_equal(np.ravel(a.alpha), np.full(K, .2)) and np.array_equal(np.ravel(b.alpha), np.full(K2, .1))
    b.close()
    a.close()
    assert _buffers(hip)[0] == live0                     # closing returns what the models held


def test_in_a_deferred_statistics_stream(hip):
    """Statistics left pending by a deferred E-step are launched by topic_distances -- on either model
    -- as by an explicit flush: the same matrix, the same statistics."""
    from trlda_amd import _ffi
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.utils.synthetic import make_corpus
    K, K2, V, B = 10, 12, 40, 256                        # (a shape tests/test_gpu_deferred.py defers at)
    lam, mu = _inputs(K, K2, V)
    csr = CSRDocuments(*make_corpus(B, V, seed=5, lengths=np.full(B, 3)))
    g0 = np.asfortranarray(np.random.RandomState(6).gamma(1.0, 1.0, (K, B)) + 0.1)

    def run(how):
        a, b = _model(lam), _model(mu)
        _ffi.check(hip.trlda_model_set_deferred_stats(a._handle, 1))
        dev = a.upload(csr)
        sizes = (K * B * 8, K * B * 8, K * V * 8, B * 4)
        ptrs = [_ffi.vp() for _ in sizes]
        for p, nbytes in zip(ptrs, sizes):
            _ffi.check(hip.trlda_dev_alloc(0, nbytes, C.byref(p)))
        _ffi.check(hip.trlda_dev_upload(0, ptrs[0], g0.ctypes.data, g0.nbytes))
        nan = np.full(K * V, np.nan)
        _ffi.check(hip.trlda_dev_upload(0, ptrs[2], nan.ctypes.data, nan.nbytes))
        _ffi.check(hip.trlda_model_estep_io_next(a._handle, dev.handle, None, ptrs[0], ptrs[1], ptrs[2], 20, 1e-3,
                                                 ptrs[3]))
        pending = hip.trlda_model_last_deferred(a._handle) & 1
        if how == "flush":
            _ffi.check(hip.trlda_model_flush(a._handle))
            D = a.topic_distances(b, "kl")
        elif how == "first":
            D = a.topic_distances(b, "kl")
        else:                                            # the model with pending statistics is `other`
            D = b.topic_distances(a, "kl").T.copy()
        _ffi.check(hip.trlda_dev_synchronize(0))
        s = np.empty((K, V), order="F")
        _ffi.check(hip.trlda_dev_download(0, s.ctypes.data, ptrs[2], s.nbytes))
        for p in ptrs:
            hip.trlda_dev_free(0, p)
        dev.close()
        b.close()
        a.close()
        return pending, D, s

    flushed, first, second = run("flush"), run("first"), run("other")
    assert flushed[0] and first[0] and second[0]         # the statistics were pending
    assert not np.isnan(flushed[2]).any()
    assert np.array_equal(first[1], flushed[1]) and np.array_equal(first[2], flushed[2])
    assert np.array_equal(second[2], flushed[2])
    # (b against a is the other direction of kl: the same numbers only through the restatement)
    _within("kl", first[1], _ref(K, K2, V), V)
    back = th.distances(mu, lam)
    _within("kl", np.asfortranarray(second[1].T), back, V)


# 9. errors ---------------------------------------------------------------------------------------
def test_errors_come_before_anything_runs(hip):
    from trlda_amd import _ffi
    K, K2, V = 15, 17, 33
    lam, mu = _inputs(K, K2, V)
    a, b = _model(lam), _model(mu)
    wider = _model(np.ones((3, V + 1)))
    elsewhere = _model(mu)
    elsewhere._device = a.device + 1                     # (what Python checks; the handle stays where it is)
    tall = _model(np.ones((1, 70000)))
    before = (_buffers(hip), hip.trlda_model_d2h_bytes(a._handle), _state())
    out = np.full((K, K2), -7.0, order="F")
    host = np.array(mu, order="F")

    def refused(other, lam_host, k2, measure, dist=out):
        assert hip.trlda_model_topic_distances(a._handle, other, lam_host, k2, measure,
                                               None if dist is None else dist.ctypes.data) == _ffi.ERR_ARG

    refused(b._handle, host.ctypes.data, K2, 0)          # both
    refused(b._handle, None, K2, 4)                      # unknown measures
    refused(b._handle, None, K2, -1)
    refused(b._handle, None, K2 + 1, 0)                  # not the second lambda's K
    refused(None, None, K2, 0)
    refused(None, host.ctypes.data, 0, 0)
    refused(wider._handle, None, 3, 0)                   # another V
    refused(b._handle, None, K2, 0, dist=None)
    assert hip.trlda_model_topic_distances(None, b._handle, None, K2, 0, out.ctypes.data) == _ffi.ERR_ARG
    assert hip.trlda_model_set_topicdist_chunk(a._handle, -1) == _ffi.ERR_ARG
    # more chunks than a grid takes: 70 000 words in chunks of one
    _ffi.check(hip.trlda_model_set_topicdist_chunk(tall._handle, 1))
    one = np.full((1, 1), -7.0)
    assert hip.trlda_model_topic_distances(tall._handle, None, None, 1, 0, one.ctypes.data) == _ffi.ERR_ARG
    with pytest.raises(_ffi.TrldaError, match="chunks") as info:
        tall.topic_distances()
    assert info.value.code == _ffi.ERR_ARG and one[0, 0] == -7.0
    _ffi.check(hip.trlda_model_set_topicdist_chunk(tall._handle, 0))
    for call in (a.topic_distances, a.match_topics):
        with pytest.raises(ValueError, match="number of words"):
            call(wider)
        with pytest.raises(ValueError, match="device"):
            call(elsewhere)
        for bad in ("hellinger", 3, 2.5, {"lambda": mu}, object()):
            with pytest.raises(TypeError):
                call(bad)
        for bad in (np.ones(V), np.ones((K2, V + 1)), np.ones((2, K2, V))):
            with pytest.raises(ValueError):
                call(bad)
        for value in (0.0, -1.0, np.nan, np.inf):
            spoiled = np.array(mu)
            spoiled[K2 - 1, V - 1] = value
            with pytest.raises(ValueError, match="finite and positive"):
                call(spoiled)
        with pytest.raises(ValueError):
            call(b, "manhattan")
        with pytest.raises(TypeError):
            call(b, 1)
    with pytest.raises(ValueError, match="identity"):
        a.match_topics(None)
    # nothing was allocated, copied, drawn or written
    assert before[0] == _buffers(hip) and before[1] == hip.trlda_model_d2h_bytes(a._handle)
    assert np.array_equal(before[2], _state()) and np.all(out == -7.0)
    # the models still work after the refusals, and not after close()
    D = a.topic_distances(b)
    _within("hellinger", D, _ref(K, K2, V), V)
    assert hip.trlda_model_d2h_bytes(a._handle) == before[1] + K * K2 * 8
    b.close()
    with pytest.raises(RuntimeError, match="closed"):
        a.topic_distances(b)
    a.close()
    with pytest.raises(RuntimeError, match="closed"):
        a.topic_distances()
    with pytest.raises(RuntimeError, match="closed"):
        a.match_topics(mu)
    assert np.array_equal(tall.topic_distances(measure="kl"), [[0.0]])
    for m in (wider, elsewhere, tall):
        m.close()
