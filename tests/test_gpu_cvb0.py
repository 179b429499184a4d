"""CVB0 on the GPU: update_variables(inference_method='cvb0') (csrc/cvb0_kernels.h) against the
NumPy restatement of its contract (tests/cvb0_host.py), bit for bit.  In-process, except the count of
the process's device buffers (tests/cvb0_buffers_worker.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cvb0_host

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
V, B = 50, 9                       # nine documents: two workgroups of four waves and one wave left over
KS = [3, 64, 65, 100, 130, 1024]   # every KPL (1, 1, 2, 2, 4, 16), full and partial last lanes
CASES = [(7, 0.0), (100, 0.001)]   # (max_iter, threshold)


@pytest.fixture(scope="module")
def hipdev():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return 0


def make_docs(seed=0):
    """The batch of every test here: an empty document, a single entry of count 1, only counts <= 0,
    counts up to 7, 300 entries (ids repeat: V = 50), and four documents drawn from ten words, so
    that a word's list spans documents."""
    rng = np.random.RandomState(seed)
    docs = [[],
            [(7, 1)],
            [(3, 0), (9, -2)],
            [(int(w), int(c)) for w, c in zip(rng.choice(V, 9, replace=False), [7, 1, 0, 3, 5, 2, 7, 4, 6])],
            [(int(rng.randint(V)), int(rng.randint(0, 4))) for _ in range(300)]]
    for _ in range(4):
        docs.append([(int(w), int(rng.randint(1, 5))) for w in rng.choice(10, rng.randint(3, 9), replace=False)])
    assert len(docs) == B
    return docs


def _csr(docs):
    indptr = np.zeros(len(docs) + 1, dtype=np.int32)
    ids, cnts = [], []
    for i, d in enumerate(docs):
        indptr[i + 1] = indptr[i] + len(d)
        ids += [w for w, _ in d]
        cnts += [c for _, c in d]
    return indptr, np.array(ids, dtype=np.int32), np.array(cnts, dtype=np.int32)


def make_alpha(K):
    return np.random.RandomState(1000 + K).gamma(2.0, 0.1, size=K) + 0.02


def make_lambda(K):
    return np.random.RandomState(K).gamma(2.0, 1.0, size=(K, V)) + 0.05


def make_latents(K):
    return np.asfortranarray(np.random.RandomState(2000 + K).dirichlet(np.ones(K), size=B).T)


def _model(K, alpha=None):
    from trlda_amd.models import OnlineLDA
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=make_alpha(K) if alpha is None else alpha,
                  eta=.3, device=0)
    m.lambdas = make_lambda(K)
    return m


def _table(model):
    from trlda_amd import _ffi
    e = np.empty((model.num_topics, model.num_words), order="F")
    _ffi.check(_ffi.lib().trlda_debug_gibbs_table(model._handle, e))
    return e


_REFERENCE = {}


def reference(K, e, max_iter, threshold, latents):
    """The restatement's (theta, sstats, iters, deltas), computed once per configuration (e is the
    same for every call on a K: it depends on lambda alone)."""
    key = (K, max_iter, threshold, latents is not None)
    if key not in _REFERENCE:
        indptr, ids, cnts = _csr(make_docs())
        _REFERENCE[key] = cvb0_host.cvb0(e, make_alpha(K), indptr, ids, cnts, latents, max_iter, threshold)
    return _REFERENCE[key]


def no_near_tie(deltas, iters, max_iter, threshold):
    """No document's final delta lies within 1e-9 relative of the threshold: a last-bit difference
    in delta could then not change the sweep a document stops at.  (Documents that ran no sweep
    have no delta.)"""
    ran = iters > 0
    return bool(np.all(np.abs(deltas[ran] - threshold) > 1e-9 * threshold)) if threshold > 0 else True


@pytest.mark.parametrize("K", KS)
def test_bitwise_against_the_restatement(hipdev, K):
    model = _model(K)
    docs = make_docs()
    try:
        for max_iter, threshold in CASES:
            theta, sstats, iters = model.update_variables(docs, inference_method="cvb0", max_iter=max_iter,
                                                          threshold=threshold, return_iterations=True)
            th, ss, it, deltas = reference(K, _table(model), max_iter, threshold, None)
            assert no_near_tie(deltas, it, max_iter, threshold), (K, deltas)     # (no document excluded)
            assert theta.flags.f_contiguous and sstats.flags.f_contiguous
            assert theta.shape == (K, B) and sstats.shape == (K, V) and iters.shape == (B,)
            assert np.array_equal(iters, it), (K, max_iter, threshold, iters, it)
            assert np.array_equal(theta, th), (K, max_iter, threshold)
            assert np.array_equal(sstats, ss), (K, max_iter, threshold)
            if threshold == 0.0:
                assert np.array_equal(iters, [0, 7, 0, 7, 7, 7, 7, 7, 7])
            else:
                assert (iters[[1, 3, 4, 5, 6, 7, 8]] >= 1).all() and not iters[[0, 2]].any()
    finally:
        model.close()


@pytest.mark.parametrize("K", [3, 100])
def test_latents(hipdev, K):
    model = _model(K)
    docs = make_docs()
    lat = make_latents(K)
    try:
        for max_iter, threshold in CASES:
            theta, sstats, iters = model.update_variables(docs, latents=lat, inference_method="cvb0",
                                                          max_iter=max_iter, threshold=threshold,
                                                          return_iterations=True)
            th, ss, it, deltas = reference(K, _table(model), max_iter, threshold, lat)
            assert no_near_tie(deltas, it, max_iter, threshold), (K, deltas)
            assert np.array_equal(iters, it) and np.array_equal(theta, th) and np.array_equal(sstats, ss)
        # max_iter = 0: the init state, which the latents decide
        t0, s0, i0 = model.update_variables(docs, latents=lat, inference_method="cvb0", max_iter=0,
                                            return_iterations=True)
        th, ss, it, _ = reference(K, _table(model), 0, 0.001, lat)
        assert not i0.any() and np.array_equal(t0, th) and np.array_equal(s0, ss)
        with pytest.raises(RuntimeError, match="Initial theta has wrong dimensionality."):
            model.update_variables(docs, latents=np.ones((K, B + 1)), inference_method="cvb0")
        with pytest.raises(TypeError):
            model.update_variables(docs, latents="no array", inference_method="cvb0")
    finally:
        model.close()


def _buffers():
    from trlda_amd import _ffi
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return live.value, total.value


def test_too_many_topics_allocates_nothing(hipdev):
    from trlda_amd import _ffi
    from trlda_amd.models import OnlineLDA
    big = OnlineLDA(num_words=V, num_topics=1025, num_documents=10, device=0)
    batch = big.upload(make_docs())
    try:
        before = _buffers()
        with pytest.raises(_ffi.TrldaError, match="1024"):
            big.update_variables(batch, inference_method="cvb0")
        assert _buffers() == before
    finally:
        batch.close()
        big.close()


def test_failure_has_its_own_message(hipdev):
    """alpha = 0 and a one-token document: in a sweep the token's weights are all zero."""
    model = _model(3, alpha=0.0)
    try:
        with pytest.raises(RuntimeError, match="CVB0: a token's topic weights sum to zero"):
            model.update_variables([[(2, 1)]], latents=np.ones((3, 1)), inference_method="cvb0")
        with pytest.raises(RuntimeError, match="max_iter"):
            model.update_variables([[(2, 1)]], inference_method="cvb0", max_iter=-1)
    finally:
        model.close()


def _slabs(docs, rows):
    """The slab rule of trlda_model_set_cvb0_slab_bytes: consecutive documents whose entries number at
    most `rows`; a longer document is a slab of its own."""
    n, first, total = 1, 0, 0
    for d, doc in enumerate(docs):
        if d > first and total + len(doc) > rows:
            n, first, total = n + 1, d, 0
        total += len(doc)
    return n


def test_repeatable_whatever_the_launch(hipdev):
    from trlda_amd import _ffi
    K = 100
    L = _ffi.lib()
    model = _model(K)
    docs = make_docs()

    def run(d):
        return model.update_variables(d, inference_method="cvb0", max_iter=100, threshold=0.001,
                                      return_iterations=True)

    def same(x, y):
        return all(np.array_equal(p, q) for p, q in zip(x, y))
    try:
        first = run(docs)
        assert same(first, run(docs))                                 # the call twice
        batch = model.upload(docs)
        try:
            assert same(first, run(batch))                            # a list against an uploaded batch
            rows = 40
            assert _slabs(docs, rows) >= 3
            _ffi.check(L.trlda_model_set_cvb0_slab_bytes(model._handle, rows * K * 8))
            assert same(first, run(batch)) and same(first, run(docs))  # at least three slabs
            _ffi.check(L.trlda_model_set_cvb0_slab_bytes(model._handle, 1))   # a slab per document
            assert same(first, run(batch))
            _ffi.check(L.trlda_model_set_cvb0_slab_bytes(model._handle, 0))
            _ffi.check(L.trlda_model_set_stream_lanes(model._handle, 2))
            assert same(first, run(batch))                            # stream lanes 1 against 2
            _ffi.check(L.trlda_model_set_stream_lanes(model._handle, 1))
        finally:
            batch.close()
    finally:
        model.close()


def test_random_stream_is_not_advanced(hipdev):
    """seed(1), a CVB0 call, a VI E-step from a drawn gamma: bitwise the gamma of seed(1) and the VI
    E-step alone."""
    import trlda_amd
    K = 20
    docs = make_docs()

    def run(with_cvb0):
        model = _model(K)
        try:
            trlda_amd.seed(1)
            if with_cvb0:
                model.update_variables(docs, inference_method="cvb0", max_iter=5)
            return model.update_variables(docs, max_iter=20)
        finally:
            model.close()

    a, b = run(False), run(True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("deferred", [False, True])
def test_cvb0_leaves_vi_alone(hipdev, deferred):
    """A CVB0 call between two VI E-steps with explicit latents leaves both VI results bitwise equal
    to the same steps without it -- also with deferred statistics and two stream lanes (the check
    tests/test_gpu_gibbs.py makes for Gibbs)."""
    from trlda_amd import _ffi
    K, W = 32, 400
    rng = np.random.RandomState(21)

    def random_docs():
        return [[(int(rng.randint(W)), int(rng.randint(0, 6))) for _ in range(rng.randint(0, 31))]
                for _ in range(64)]
    docs1, docs2 = random_docs(), random_docs()
    g1 = rng.gamma(100., .01, size=(K, 64))
    g2 = rng.gamma(100., .01, size=(K, 64))
    lam = rng.gamma(2.0, 1.0, size=(K, W)) + 0.05

    def run(with_cvb0):
        from trlda_amd.models import OnlineLDA
        m = OnlineLDA(num_words=W, num_topics=K, num_documents=1000, device=0)
        m.lambdas = lam
        if deferred:
            _ffi.check(_ffi.lib().trlda_model_set_deferred_stats(m._handle, 1))
            _ffi.check(_ffi.lib().trlda_model_set_stream_lanes(m._handle, 2))
        out = [m.update_variables(docs1, latents=g1, max_iter=20)]
        if with_cvb0:
            theta, _ = m.update_variables(docs2, inference_method="cvb0", max_iter=5)
            assert np.allclose(theta.sum(axis=0), 1.0, atol=1e-12)
        out.append(m.update_variables(docs2, latents=g2, max_iter=20))
        m.close()
        return out

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def test_training_is_not_built_yet(hipdev):
    from trlda_amd.models import BatchLDA
    docs = make_docs()
    online = _model(5)
    batch = BatchLDA(num_words=V, num_topics=5, device=0)
    try:
        for m in (online, batch):
            with pytest.raises(NotImplementedError, match="not built yet"):
                m.update_parameters(docs, inference_method="cvb0")
            with pytest.raises(NotImplementedError, match="not built yet"):
                m.lower_bound(docs, inference_method="cvb0")
            with pytest.raises(TypeError):
                m.update_variables(docs, inference_method="map")
    finally:
        online.close()
        batch.close()


def test_closing_releases_every_device_buffer(hipdev):
    out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(HERE, "cvb0_buffers_worker.py")],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "buffers ok" in out.stdout
