"""Gibbs inference on the GPU: update_variables(inference_method='gibbs') (reference
src/lda.cpp:224-293; csrc/gibbs_kernels.h).  In-process only."""
import ctypes as C

import numpy as np
import pytest

import gibbs_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipdev():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return 0


def _model(K, V, alpha=.1, seed=1):
    from trlda_amd.models import OnlineLDA
    rng = np.random.RandomState(seed)
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=alpha, eta=.3, device=0)
    m.lambdas = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    return m


def _csr(docs):
    indptr = np.zeros(len(docs) + 1, dtype=np.int32)
    ids, cnts = [], []
    for i, d in enumerate(docs):
        indptr[i + 1] = indptr[i] + len(d)
        ids += [w for w, _ in d]
        cnts += [c for _, c in d]
    return indptr, np.array(ids, dtype=np.int32), np.array(cnts, dtype=np.int32)


def _device_gibbs(model, docs, theta0, num_samples, burn_in, key):
    """trlda_model_gibbs with an explicit key: (theta, sstats, e table the kernel read)."""
    from trlda_amd import _ffi
    from trlda_amd.documents import DeviceBatch
    L = _ffi.lib()
    K, V = model.num_topics, model.num_words
    batch = DeviceBatch(docs, V, 0)
    B = len(batch)
    bufs = []

    def alloc(nbytes):
        p = _ffi.vp()
        _ffi.check(L.trlda_dev_alloc(0, max(nbytes, 8), C.byref(p)))
        bufs.append(p)
        return p
    try:
        th_out = alloc(K * B * 8)
        ss = alloc(K * V * 8)
        th_in = None
        if theta0 is not None:
            t0 = np.asfortranarray(theta0, dtype=np.float64)
            th_in = alloc(K * B * 8)
            _ffi.check(L.trlda_dev_upload(0, th_in, t0.ctypes.data, t0.nbytes))
        _ffi.check(L.trlda_model_gibbs(model._handle, batch.handle, th_in, th_out, ss, num_samples, burn_in,
                                       key))
        theta = np.empty((K, B), order="F")
        sstats = np.empty((K, V), order="F")
        _ffi.check(L.trlda_dev_download(0, theta.ctypes.data, th_out, theta.nbytes))
        _ffi.check(L.trlda_dev_download(0, sstats.ctypes.data, ss, sstats.nbytes))
        e = np.empty((K, V), order="F")
        _ffi.check(L.trlda_debug_gibbs_table(model._handle, e))
    finally:
        for p in bufs:
            L.trlda_dev_free(0, p)
        batch.close()
    return theta, sstats, e


def _host_table(oracle, lam, words):
    """e = exp(psi(lambda) - psi(rowsum(lambda))) on the host, from the oracle's digamma, for the
    columns `words` (K x len(words))."""
    psi = np.vectorize(oracle.digamma, otypes=[np.float64])
    lam = np.asarray(lam, dtype=np.float64)
    return np.exp(psi(lam[:, words]) - psi(lam.sum(axis=1))[:, None])


def _random_docs(rng, B, V, max_len=12, max_cnt=5):
    docs = []
    for _ in range(B):
        n = rng.randint(0, max_len + 1)
        docs.append([(int(rng.randint(V)), int(rng.randint(0, max_cnt + 1))) for _ in range(n)])
    return docs


def _check_chain(model, docs, theta0, ns, bi, key):
    theta, sstats, e = _device_gibbs(model, docs, theta0, ns, bi, key)
    indptr, ids, cnts = _csr(docs)
    th_h, cnt_h, _ = gibbs_host.gibbs(e, model.alpha[:, 0], indptr, ids, cnts, theta0, ns, bi, key)
    unit = 1.0 / ns if ns > 0 else 0.0
    assert np.array_equal(sstats, cnt_h * unit), (model.num_topics, ns, bi)
    assert np.allclose(theta, th_h, rtol=1e-12, atol=1e-300)
    # (exact counts: sstats / unit are integers)
    if ns:
        assert np.array_equal(np.rint(sstats * ns), cnt_h)
    return theta, sstats


@pytest.mark.parametrize("K", [1, 3, 64, 65, 100, 200, 500, 1000])
def test_bitwise_chain_every_kpl(hipdev, K):
    V = 60
    rng = np.random.RandomState(K)
    model = _model(K, V, alpha=.1, seed=K)
    docs = _random_docs(rng, 6, V, max_len=6, max_cnt=4)
    docs[1] = []                                               # an empty document
    docs[2] = [(3, 2), (3, 1), (7, 0), (9, 3)]                 # a duplicate id, a zero count
    theta0 = rng.dirichlet(np.ones(K), size=len(docs)).T
    _check_chain(model, docs, theta0, 1, 2, 0x0123456789ABCDEF + K)
    _check_chain(model, docs, None, 1, 0, 0xFEDCBA9876543210 + K)


@pytest.mark.parametrize("ns,bi", [(0, 2), (1, 0), (3, 7), (3, 2), (1, 7), (0, 0)])
def test_bitwise_chain_samples_burn_in(hipdev, ns, bi):
    K, V = 20, 80
    rng = np.random.RandomState(ns * 10 + bi)
    model = _model(K, V, alpha=.1, seed=3)
    docs = _random_docs(rng, 5, V, max_len=8, max_cnt=50)
    docs.append([])
    theta0 = rng.dirichlet(np.ones(K), size=len(docs)).T
    theta, sstats = _check_chain(model, docs, theta0, ns, bi, 99 + ns + 100 * bi)
    if ns == 0:
        assert not sstats.any()


@pytest.mark.parametrize("alpha", [1e-3, 0.1, 5.0])
def test_bitwise_chain_alpha_long_document(hipdev, alpha):
    K, V = 70, 300
    rng = np.random.RandomState(int(alpha * 1000))
    model = _model(K, V, alpha=alpha, seed=4)
    long_doc = [(int(w), 20) for w in rng.choice(V, 100, replace=False)]     # 2000 tokens
    docs = [long_doc, [(5, 50)], [], [(1, 1), (1, 2)]]
    theta0 = rng.dirichlet(np.ones(K), size=len(docs)).T
    theta, _ = _check_chain(model, docs, theta0, 1, 1, 7777)
    assert np.allclose(theta.sum(axis=0), 1.0, atol=1e-12)


@pytest.mark.parametrize("K,V", [(20, 300), (100, 50000)])
def test_table_is_normalised(hipdev, oracle, K, V):
    """The table the sampler reads is exp(psi(lambda) - psi(rowsum(lambda))), formed on the host
    from lambda with the oracle's digamma -- not the unnormalised exp(psi(lambda)) of the fused
    preambles.  K = 100, V = 50 000 (K V >= 2^22, V / 32 > 64 row-sum blocks) takes the preamble's
    branch with many row-sum blocks and rowsum_combine_kernel."""
    rng = np.random.RandomState(K + V)
    model = _model(K, V, alpha=.1, seed=K)
    lam = np.array(model.lambdas)
    docs = _random_docs(rng, 8, V, max_len=30, max_cnt=3)
    docs[0] = docs[0] + [(V - 1, 2), (0, 1)]
    model.update_variables(docs, inference_method="gibbs")
    e = np.empty((K, V), order="F")
    from trlda_amd import _ffi
    _ffi.check(_ffi.lib().trlda_debug_gibbs_table(model._handle, e))
    words = sorted({w for d in docs for w, _ in d})
    want = _host_table(oracle, lam, words)
    rel = np.abs(e[:, words] - want) / want
    assert rel.max() < 1e-12, rel.max()
    # (the unnormalised exp(psi(lambda)) differs by the factor exp(psi(row sum)): far outside that)
    psi = np.vectorize(oracle.digamma, otypes=[np.float64])
    unnormalised = np.exp(psi(lam[:, words]))
    assert np.min(np.abs(unnormalised - want) / want) > 1e-3


def test_exact_posterior(hipdev, oracle):
    """20 000 chains of one 6-token document, K = 3: means of the statistics and of theta against
    the posterior enumerated from the host's own table (lambda and the oracle's digamma, not the
    kernel's buffer).  The tolerance is t * SE, SE from the spread of 20 sub-batches of 1 000 chains
    (independent of the big batch: a t distribution with 19 degrees of freedom).  Fifteen
    quantities are tested (12 count cells, 3 theta means); t = 9.0 > t_19's two-sided 1e-6 / 15
    quantile (8.51), so the test fails by chance with probability below 1e-6."""
    import trlda_amd
    from trlda_amd.documents import DeviceBatch
    K, V = 3, 4
    model = _model(K, V, alpha=np.array([0.5, 0.2, 1.0]), seed=11)
    model.lambdas = np.array([[5., 1., 2., .5], [1., 4., 1., 3.], [2., 2., 6., 1.]])
    doc = [(0, 2), (1, 1), (2, 2), (3, 1)]
    words = [0, 0, 1, 2, 2, 3]
    trlda_amd.seed(5)
    ns, bi = 50, 30

    def run(n):
        batch = DeviceBatch([doc] * n, V, 0)
        try:
            theta, sstats = model.update_variables(batch, inference_method="gibbs", num_samples=ns,
                                                   burn_in=bi)
        finally:
            batch.close()
        return theta, sstats / n

    theta, mean_counts = run(20000)
    e_host = _host_table(oracle, model.lambdas, list(range(V)))
    e = np.empty((K, V), order="F")
    from trlda_amd import _ffi
    _ffi.check(_ffi.lib().trlda_debug_gibbs_table(model._handle, e))
    assert np.max(np.abs(e - e_host) / e_host) < 1e-12
    want_counts, want_theta = gibbs_host.exact_posterior(e_host, model.alpha[:, 0], words)
    subs = [run(1000) for _ in range(20)]
    sub_counts = np.stack([s[1] for s in subs])
    sub_theta = np.stack([s[0].mean(axis=1) for s in subs])
    se_counts = sub_counts.std(axis=0, ddof=1) / np.sqrt(20)
    se_theta = sub_theta.std(axis=0, ddof=1) / np.sqrt(20)
    t = 9.0
    assert np.all(np.abs(mean_counts - want_counts) <= t * se_counts + 1e-12)
    assert np.all(np.abs(theta.mean(axis=1) - want_theta) <= t * se_theta)


def test_invariants_and_seed(hipdev):
    import trlda_amd
    K, V = 30, 500
    rng = np.random.RandomState(2)
    model = _model(K, V, alpha=.1, seed=2)
    docs = _random_docs(rng, 200, 400, max_len=20, max_cnt=6)       # words 400.. never occur
    indptr, ids, cnts = _csr(docs)
    trlda_amd.seed(17)
    theta, sstats = model.update_variables(docs, inference_method="gibbs", num_samples=3, burn_in=2)
    assert theta.shape == (K, len(docs)) and sstats.shape == (K, V)
    assert theta.flags.f_contiguous and sstats.flags.f_contiguous
    wc = np.bincount(ids, weights=np.maximum(cnts, 0), minlength=V)
    assert np.allclose(sstats.sum(axis=0), wc, rtol=1e-12, atol=1e-9)
    assert abs(sstats.sum() - np.maximum(cnts, 0).sum()) < 1e-6
    assert not sstats[:, 400:].any()
    assert (theta >= 0).all() and np.allclose(theta.sum(axis=0), 1.0, atol=1e-12)
    trlda_amd.seed(17)
    again = model.update_variables(docs, inference_method="gibbs", num_samples=3, burn_in=2)
    assert np.array_equal(again[0], theta) and np.array_equal(again[1], sstats)
    third = model.update_variables(docs, inference_method="gibbs", num_samples=3, burn_in=2)
    assert not np.array_equal(third[0], theta)


def test_same_document_same_index(hipdev):
    K, V = 40, 200
    rng = np.random.RandomState(8)
    model = _model(K, V, seed=8)
    a = _random_docs(rng, 10, V)
    b = _random_docs(rng, 10, V)
    b[4] = a[4]
    b[6] = sorted(b[6]) + [(1, 30)]                            # other lengths: another order
    theta0 = rng.dirichlet(np.ones(K), size=10).T
    ta, _, _ = _device_gibbs(model, a, theta0, 2, 2, 4242)
    tb, _, _ = _device_gibbs(model, b, theta0, 2, 2, 4242)
    assert np.array_equal(ta[:, 4], tb[:, 4])


def test_reference_test_gibbs_setup(hipdev):
    """python/tests/onlinelda_test.py:99-109 (test_gibbs), through both import paths."""
    import trlda
    from trlda.models import OnlineLDA as RefOnlineLDA
    from trlda_amd.models import OnlineLDA
    rng = np.random.RandomState(0)
    docs = [list(zip(rng.permutation(100)[:rng.randint(1, 20)].tolist(),
                     rng.randint(0, 10, size=100).tolist())) for _ in range(1000)]
    for cls in (OnlineLDA, RefOnlineLDA):
        model = cls(num_words=100, num_topics=10, num_documents=10000)
        trlda.seed(3)
        theta, sstats = model.update_variables(docs, inference_method='gibbs')
        assert theta.shape == (10, 1000) and sstats.shape == (10, 100)
        theta2, sstats2 = model.do_e_step(docs, inference_method='GIBBS', num_samples=2, burn_in=1)
        assert theta2.shape == (10, 1000)
        assert np.allclose(sstats2.sum(), sum(c for d in docs for _, c in d))
        batch = model.upload(docs)
        try:
            theta3, _ = model.update_variables(batch, inference_method='gibbs')
        finally:
            batch.close()
        assert np.allclose(theta3.sum(axis=0), 1.0, atol=1e-12)


def test_errors(hipdev):
    from trlda_amd.models import OnlineLDA
    model = _model(5, 50)
    docs = [[(1, 2)], [(3, 1)]]
    with pytest.raises(RuntimeError, match="Initial theta has wrong dimensionality."):
        model.update_variables(docs, latents=np.ones((5, 3)), inference_method='gibbs')
    with pytest.raises(RuntimeError):
        model.update_variables(docs, inference_method='gibbs', num_samples=-1)
    with pytest.raises(RuntimeError):
        model.update_variables(docs, inference_method='gibbs', burn_in=-1)
    with pytest.raises(TypeError):
        model.update_variables(docs, inference_method='gibbs', return_iterations=True)
    with pytest.raises(NotImplementedError):
        model.lower_bound(docs, inference_method='gibbs')
    big = OnlineLDA(num_words=20, num_topics=1025, num_documents=10, device=0)
    with pytest.raises(RuntimeError, match="1024"):
        big.update_variables([[(1, 1)]], inference_method='gibbs')
    # alpha = 0 and a one-token document: the token's histogram is all zeros after its removal
    zero = _model(3, 10, alpha=0.0)
    with pytest.raises(RuntimeError, match="Something went wrong while sampling from histogram."):
        zero.update_variables([[(2, 1)]], inference_method='gibbs')
    # the model still works afterwards
    theta, _ = model.update_variables(docs, inference_method='gibbs')
    assert np.allclose(theta.sum(axis=0), 1.0, atol=1e-12)


@pytest.mark.parametrize("deferred", [False, True])
def test_gibbs_leaves_vi_alone(hipdev, deferred):
    """A Gibbs call between two VI E-steps with explicit latents leaves both VI results bitwise equal
    to the same steps without it -- also with deferred statistics and two stream lanes."""
    from trlda_amd import _ffi
    K, V = 32, 400
    rng = np.random.RandomState(21)
    docs1 = _random_docs(rng, 64, V, max_len=30)
    docs2 = _random_docs(rng, 64, V, max_len=30)
    g1 = rng.gamma(100., .01, size=(K, 64))
    g2 = rng.gamma(100., .01, size=(K, 64))
    lam = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05

    def run(with_gibbs):
        from trlda_amd.models import OnlineLDA
        m = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, device=0)
        m.lambdas = lam
        if deferred:
            _ffi.check(_ffi.lib().trlda_model_set_deferred_stats(m._handle, 1))
            _ffi.check(_ffi.lib().trlda_model_set_stream_lanes(m._handle, 2))
        out = [m.update_variables(docs1, latents=g1, max_iter=20)]
        if with_gibbs:
            m.update_variables(docs2, inference_method='gibbs', num_samples=2, burn_in=1)
        out.append(m.update_variables(docs2, latents=g2, max_iter=20))
        m.close()
        return out

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


@pytest.mark.parametrize("K,V", [(3, 300), (65, 300), (200, 2100)])
def test_table_equals_vi_split_preamble(hipdev, K, V):
    """The sampler's table and the table of the VI E-step's two-kernel preamble (row sums from
    lambda itself, nothing carried over) are the same computation: bitwise equal at the batch's
    word columns.  V = 300: 9 row-sum blocks; V = 2100: the cap of 64; K V < 2^22 throughout, so
    both hand the uncombined block partials to exp_elog_beta_kernel."""
    from trlda_amd import _ffi
    L = _ffi.lib()
    rng = np.random.RandomState(K + V)
    model = _model(K, V, alpha=.1, seed=K)
    docs = _random_docs(rng, 4, V, max_len=8, max_cnt=3)
    docs[0] = docs[0] + [(V - 1, 2), (0, 1)]
    words = sorted({w for d in docs for w, _ in d})
    _ffi.check(L.trlda_model_set_split_preamble(model._handle, 1))
    _ffi.check(L.trlda_model_set_carry_rowsums(model._handle, 0))
    model.update_variables(docs, max_iter=2)
    vi = np.empty((K, V), order="F")
    _ffi.check(L.trlda_debug_peek(model._handle, 0, vi.ctypes.data, vi.size))
    model.update_variables(docs, inference_method="gibbs", num_samples=1, burn_in=0)
    e = np.empty((K, V), order="F")
    _ffi.check(L.trlda_debug_gibbs_table(model._handle, e))
    model.close()
    assert np.all(e[:, words] > 0)
    assert np.array_equal(vi[:, words], e[:, words])
