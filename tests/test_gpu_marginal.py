"""LDA.document_log_likelihood on the GPU (csrc/marginal_kernels.h): parity with the NumPy
restatement (tests/marginal_host.py) under the same key for both proposals across the register and
LDS variants, the exact marginal of a short document by enumeration, the determinism rules, the
random stream, the errors, and what the number means."""
import ctypes as C
import math

import numpy as np
import pytest

import marginal_host as mh

pytestmark = pytest.mark.gpu

PARITY_RTOL = 1e-9          # the project's parity tolerance (README, last paragraph)
T_BOUND = 9.0               # test_gpu_gibbs.py, test_exact_posterior


@pytest.fixture(scope="module")
def hip(hip_lib):
    from trlda_amd import _ffi
    assert _ffi.device_count() >= 1, "GPU tests need a visible MI355X"
    return hip_lib


def _model(K, V, lam, alpha=.1, eta=.3):
    """An OnlineLDA holding `lam` without the constructor's K V 100 draws."""
    from trlda_amd.models import OnlineLDA
    m = OnlineLDA.__new__(OnlineLDA)
    m._num_documents = 1000
    m._update_count = 0
    m._ada_tau = 1000.
    m._ada_rho = 1. / m._ada_tau
    m._ada_sq_norm = 1.
    m._setup(V, K, alpha, eta, None, _lambda=np.asfortranarray(lam))
    return m


def _lambda(K, V, seed):
    return np.asfortranarray(np.random.RandomState(seed).gamma(.5, 1., (K, V)) + .01)


def _docs(V, seed, long_len=300):
    """Random documents; among them empty ones, entries with c = 0, an id three times, a document of
    zero counts only and one long document."""
    rng = np.random.RandomState(seed)
    docs = []
    for n in (0, 1, 7, 40, 0, 23):
        docs.append([(int(w), int(c)) for w, c in zip(rng.randint(0, V, n), rng.randint(1, 5, n))])
    z = [(int(w), 0 if i % 2 == 0 else 3) for i, w in enumerate(rng.randint(0, V, 12))]
    docs.append(z)
    r = rng.randint(0, V, 9)
    r[[2, 5, 8]] = r[0]
    docs.append([(int(w), int(c)) for w, c in zip(r, rng.randint(1, 6, 9))])
    docs.append([(int(w), 0) for w in rng.randint(0, V, 3)])
    docs.append([(int(w), int(c)) for w, c in zip(rng.randint(0, V, long_len), rng.randint(1, 4, long_len))])
    return docs


def _csr(docs):
    indptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int32)
    ids = np.array([w for d in docs for w, _ in d], dtype=np.int32)
    cnts = np.array([c for d in docs for _, c in d], dtype=np.int32)
    return indptr, ids, cnts


def _state():
    from trlda_amd import _ffi
    s = np.zeros(33, dtype=np.uint32)
    _ffi.lib().trlda_rng_get_state(s)
    return s


def _key():
    from trlda_amd import _ffi
    key = C.c_uint64(0)
    _ffi.check(_ffi.lib().trlda_rng_draw_key(C.byref(key)))
    return key.value


def _gamma0(K, B):
    from trlda_amd import _ffi
    g = np.empty((K, B), order="F")
    _ffi.lib().trlda_sample_gamma_init(K, B, g)
    return g


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# --------------------------------------------------------------------------------------------
# 1. parity with the restatement
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,V,S", [(3, 50, 128), (30, 200, 128), (100, 300, 128), (600, 200, 48), (2304, 120, 16)])
def test_parity_with_the_restatement(hip, K, V, S):
    """Device loglik and ess against marginal_host under the same key, both proposals: 1e-9
    relative.  The restatement shares every draw, but not the device's log / exp / cos / lgamma nor
    its FMAs, so the comparison is to rounding; the observed maxima are printed (1e-12 is what
    test_gpu_gibbs.py asserts where every draw is shared: it is asserted here for loglik, whose
    error is a few ulp of a sum of logs; ess is a ratio of sums of exp(log w - max) and takes the
    absolute error of log w as its relative one, so it keeps the 1e-9).  Observed maxima: loglik
    2.2e-14 (K = 600, 'vi'; 1.2e-13 at K = 6814 in test_at_the_vi_bound), ess 1.9e-13 (K = 30, 'vi').
    For 'vi' the gamma the call leaves in its in/out array is bitwise update_variables' under the
    same gamma0."""
    import trlda_amd
    from trlda_amd import _ffi
    lam = _lambda(K, V, K)
    alpha = np.random.RandomState(K + 1).gamma(2., .1, K) + .02
    docs = _docs(V, K + 2, long_len=300 if K <= 600 else 60)
    indptr, ids, cnts = _csr(docs)
    B = len(docs)
    m = _model(K, V, lam, alpha=alpha)
    batch = m.upload(docs)
    try:
        for proposal in ("vi", "prior"):
            trlda_amd.seed(100 + K)
            g0 = _gamma0(K, B) if proposal == "vi" else None
            key = _key()
            trlda_amd.seed(100 + K)
            ll, ess = m.document_log_likelihood(batch, num_samples=S, proposal=proposal, return_ess=True)
            gamma = None
            if proposal == "vi":
                gamma, _ = m.update_variables(batch, latents=g0)
                # the call's own gamma, through the C entry (in: gamma0, out: gamma)
                g_io = np.array(g0, order="F", copy=True)
                ll_c, ess_c = np.empty(B), np.empty(B)
                trlda_amd.seed(100 + K)
                _gamma0(K, B)
                _ffi.check(hip.trlda_model_document_loglik(m._handle, batch.handle, g_io.ctypes.data,
                                                           _ffi.PROPOSAL_VI, S, 100, 1e-3, ll_c,
                                                           ess_c.ctypes.data))
                assert np.array_equal(g_io, gamma)
                assert np.array_equal(ll_c, ll) and np.array_equal(ess_c, ess)
            want_ll, want_ess = mh.document_loglik(indptr, ids, cnts, lam, alpha, key, S, gamma=gamma)
            assert np.all(np.isfinite(ll)) and ll.shape == (B,) and ll.dtype == np.float64
            empty = np.diff(indptr) == 0
            assert np.all(ll[empty] == 0.0) and np.all(ess[empty] == S)
            # (documents whose counts are all 0: gamma = alpha, every weight is 1 and loglik is 0 up to
            # the rounding of gamma -- an absolute comparison there)
            tok = np.add.reduceat(np.append(cnts, 0), indptr[:-1]) * ~empty > 0
            assert np.all(np.abs(ll[~tok]) < 1e-12) and np.all(np.abs(want_ll[~tok]) < 1e-12)
            e_ll, e_ess = _rel(ll[tok], want_ll[tok]), _rel(ess, want_ess)
            print("K=%d %s: max rel err loglik %.3e ess %.3e" % (K, proposal, e_ll, e_ess))
            assert e_ll < PARITY_RTOL and e_ess < PARITY_RTOL, (K, proposal, e_ll, e_ess)
            assert e_ll < 1e-12, (K, proposal, e_ll)
            assert np.all(ess >= 1.0) and np.all(ess <= S)
    finally:
        batch.close()
        m.close()


# --------------------------------------------------------------------------------------------
# 2. exactness: the enumerated marginal of a 6-token document
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proposal", ["vi", "prior"])
def test_exact_marginal_of_a_short_document(hip, proposal):
    """The CPU test of test_marginal_host.py through the model: the K = 3 document 20 000 times in
    one batch (d supplies independent streams), S = 1000 each; R_d = exp(loglik_d - exact).  Their
    mean is within t SE of 1, SE from the spread of the means of 20 groups of 1 000 documents
    (t_19), t = 9.0.  Observed |mean - 1| / SE: 'prior' 0.48 (mean 0.99998, SE 4.6e-5, mean ess 950),
    'vi' 2.70 (mean 0.9803, SE 7.3e-3, mean ess 126): the heavy right tail of the 'vi' weights on
    so short a document (test_marginal_host.py has the reason) keeps finite runs below 1."""
    import trlda_amd
    lam = np.array([[5., 1., 2., .5], [1., 4., 1., 3.], [2., 2., 6., 1.]])
    alpha = np.array([0.5, 0.2, 1.0])
    doc = [(0, 2), (1, 1), (2, 2), (3, 1)]
    words = [0, 0, 1, 2, 2, 3]
    exact = mh.exact_log_marginal(lam / lam.sum(axis=1)[:, None], alpha, words)
    m = _model(3, 4, lam, alpha=alpha)
    try:
        trlda_amd.seed(5)
        ll, ess = m.document_log_likelihood([doc] * 20000, num_samples=1000, proposal=proposal,
                                            return_ess=True)
    finally:
        m.close()
    R = np.exp(ll - exact)
    groups = R.reshape(20, 1000).mean(axis=1)
    se = groups.std(ddof=1) / math.sqrt(20)
    print("%s: mean %.6f SE %.3e |mean - 1| / SE %.3f, mean ess %.1f" %
          (proposal, R.mean(), se, abs(R.mean() - 1) / se, ess.mean()))
    assert se > 0 and abs(R.mean() - 1.0) <= T_BOUND * se, (R.mean(), se)


# --------------------------------------------------------------------------------------------
# 3. invariants
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proposal", ["vi", "prior"])
def test_determinism_and_the_random_stream(hip, proposal):
    import trlda_amd
    K, V, S = 30, 200, 64
    lam = _lambda(K, V, 1)
    docs = _docs(V, 2, long_len=150)
    B = len(docs)
    m = _model(K, V, lam)
    try:
        lam_before, alpha_before = np.array(m.lambdas), m.alpha
        eta_before, count_before = m.eta, m.update_count
        trlda_amd.seed(17)
        a, ess = m.document_log_likelihood(docs, num_samples=S, proposal=proposal, return_ess=True)
        got = _state()
        trlda_amd.seed(17)
        if proposal == "vi":
            _gamma0(K, B)
        _key()
        assert np.array_equal(got, _state())           # exactly gamma0's draws (vi) and one key
        trlda_amd.seed(17)
        b = m.document_log_likelihood(docs, num_samples=S, proposal=proposal)
        assert np.array_equal(a, b)                     # the same seed: the same bits
        trlda_amd.seed(18)
        c = m.document_log_likelihood(docs, num_samples=S, proposal=proposal)
        full = np.array([len(d) > 0 and any(cn for _, cn in d) for d in docs])
        assert np.all(a[full] != c[full])               # another seed: other values
        assert np.all((ess >= 1.0) & (ess <= S))
        assert a[0] == 0.0 and a[4] == 0.0 and ess[0] == S
        # DeviceBatch and list input
        batch = m.upload(docs)
        trlda_amd.seed(17)
        e = m.document_log_likelihood(batch, num_samples=S, proposal=proposal)
        batch.close()
        assert np.array_equal(a, e)
        # a document at the same index of a larger batch: the same bits (for 'vi' under the same gamma0)
        more = docs + _docs(V, 3, long_len=80)
        g0 = np.random.RandomState(4).gamma(100., .01, (K, len(more)))
        lat = dict(latents=g0[:, :B]) if proposal == "vi" else {}
        lat_more = dict(latents=g0) if proposal == "vi" else {}
        trlda_amd.seed(19)
        small, ess_small = m.document_log_likelihood(docs, num_samples=S, proposal=proposal, return_ess=True, **lat)
        trlda_amd.seed(19)
        big, ess_big = m.document_log_likelihood(more, num_samples=S, proposal=proposal, return_ess=True,
                                                 **lat_more)
        assert np.array_equal(small, big[:B]) and np.array_equal(ess_small, ess_big[:B])
        # the model is as it was
        assert np.array_equal(lam_before, m.lambdas) and np.array_equal(alpha_before, m.alpha)
        assert m.eta == eta_before and m.update_count == count_before
        # an empty batch is a valid call: one key, no values
        trlda_amd.seed(21)
        none = m.document_log_likelihood([], num_samples=S, proposal=proposal)
        got = _state()
        trlda_amd.seed(21)
        _key()
        assert none.shape == (0,) and np.array_equal(got, _state())
    finally:
        m.close()


# --------------------------------------------------------------------------------------------
# 4. errors: each before anything is drawn
# --------------------------------------------------------------------------------------------
def test_errors_draw_nothing(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K, V = 3, 20
    m = _model(K, V, _lambda(K, V, 5))
    docs = [[(1, 2), (3, 1)], []]
    batch = m.upload(docs)
    try:
        trlda_amd.seed(3)
        before = _state()

        def refused(exc, match=None, **kw):
            with pytest.raises(exc, match=match):
                m.document_log_likelihood(batch, **kw)
            assert np.array_equal(before, _state())

        refused(TypeError, "proposal", proposal="gibbs")
        refused(TypeError, "latents", proposal="prior", latents=np.ones((K, 2)))
        refused(RuntimeError, "num_samples", num_samples=0)
        refused(RuntimeError, "2\\^32", num_samples=2 ** 32 // K + 1)
        refused(RuntimeError, "Initial gamma has wrong dimensionality.", latents=np.ones((K, 3)))
        refused(RuntimeError, "Initial gamma has wrong dimensionality.", latents=np.ones((K + 1, 2)))
        # the C entry refuses the same on its own
        ll = np.empty(2)
        g = np.ones((K, 2), order="F")
        for proposal, S in ((7, 8), (_ffi.PROPOSAL_VI, 0), (_ffi.PROPOSAL_PRIOR, -1),
                            (_ffi.PROPOSAL_PRIOR, 2 ** 32 // K + 1)):
            rc = hip.trlda_model_document_loglik(m._handle, batch.handle, g.ctypes.data, proposal, S, 10, 1e-3,
                                                 ll, None)
            assert rc == _ffi.ERR_ARG, (proposal, S, rc)
            assert np.array_equal(before, _state())
        assert hip.trlda_model_document_loglik(m._handle, batch.handle, None, _ffi.PROPOSAL_VI, 8, 10, 1e-3,
                                               ll, None) == _ffi.ERR_ARG
        assert np.array_equal(before, _state())
        # 'prior' needs no gamma and ess may be NULL
        _ffi.check(hip.trlda_model_document_loglik(m._handle, batch.handle, None, _ffi.PROPOSAL_PRIOR, 8, 10,
                                                   1e-3, ll, None))
        assert np.isfinite(ll[0]) and ll[0] < 0 and ll[1] == 0.0
        # case-insensitive names
        trlda_amd.seed(3)
        a = m.document_log_likelihood(batch, num_samples=8, proposal="PRIOR")
        trlda_amd.seed(3)
        assert np.array_equal(a, m.document_log_likelihood(batch, num_samples=8, proposal="prior"))
    finally:
        batch.close()
        m.close()


@pytest.mark.parametrize("proposal", ["vi", "prior"])
def test_above_the_vi_bound(hip, proposal):
    import trlda_amd
    from trlda_amd import _ffi
    K = _ffi.vi_max_topics() + 1
    m = _model(K, 3, np.ones((K, 3)))
    try:
        trlda_amd.seed(3)
        before = _state()
        with pytest.raises(_ffi.TrldaError, match="TRLDA_VI_MAX_TOPICS"):
            m.document_log_likelihood([[(0, 1)]], num_samples=2, proposal=proposal)
        assert np.array_equal(before, _state())
        ll = np.empty(1)
        batch = m.upload([[(0, 1)]])
        rc = hip.trlda_model_document_loglik(m._handle, batch.handle, None, _ffi.PROPOSAL_PRIOR, 2, 10, 1e-3,
                                             ll, None)
        batch.close()
        assert rc == _ffi.ERR_ARG and np.array_equal(before, _state())
    finally:
        m.close()


def test_at_the_vi_bound(hip):
    """K = TRLDA_VI_MAX_TOPICS: two waves per document; against the restatement."""
    import trlda_amd
    from trlda_amd import _ffi
    K, V, S = _ffi.vi_max_topics(), 40, 6
    assert mh.waves(K) == 2
    lam = _lambda(K, V, 9)
    docs = [[(1, 2), (3, 1), (7, 0), (1, 1)], [], [(int(w), 1) for w in range(30)]]
    indptr, ids, cnts = _csr(docs)
    m = _model(K, V, lam)
    try:
        for proposal in ("prior", "vi"):
            trlda_amd.seed(8)
            g0 = _gamma0(K, 3) if proposal == "vi" else None
            key = _key()
            trlda_amd.seed(8)
            ll, ess = m.document_log_likelihood(docs, num_samples=S, proposal=proposal, return_ess=True)
            gamma = m.update_variables(docs, latents=g0)[0] if proposal == "vi" else None
            want_ll, want_ess = mh.document_loglik(indptr, ids, cnts, lam, np.full(K, .1), key, S, gamma=gamma)
            print("K=%d %s: max rel err loglik %.3e ess %.3e" % (K, proposal, _rel(ll[[0, 2]], want_ll[[0, 2]]),
                                                                 _rel(ess, want_ess)))
            assert _rel(ll[[0, 2]], want_ll[[0, 2]]) < PARITY_RTOL and _rel(ess, want_ess) < PARITY_RTOL
            assert ll[1] == 0.0
    finally:
        m.close()


# --------------------------------------------------------------------------------------------
# 5. what the number means
# --------------------------------------------------------------------------------------------
def test_the_generating_model_scores_higher(hip):
    """Documents sampled from the model: the generating lambda explains them better than the same
    lambda with its word columns permuted, under the same seed, for both proposals."""
    import trlda_amd
    K, V = 20, 400
    rng = np.random.RandomState(6)
    lam = np.asfortranarray(200. * rng.dirichlet(np.full(V, .05), K) + .01)
    m = _model(K, V, lam)
    try:
        trlda_amd.seed(31)
        docs = m.sample(200, 60)
        tokens = sum(c for d in docs for _, c in d)
        for proposal in ("vi", "prior"):
            trlda_amd.seed(32)
            m.lambdas = lam
            true = m.document_log_likelihood(docs, proposal=proposal)
            m.lambdas = lam[:, rng.permutation(V)]
            trlda_amd.seed(32)
            perm = m.document_log_likelihood(docs, proposal=proposal)
            print("%s: per-word perplexity %.1f (generating) %.1f (permuted)" %
                  (proposal, math.exp(-true.sum() / tokens), math.exp(-perm.sum() / tokens)))
            assert np.all(np.isfinite(true)) and np.all(np.isfinite(perm))
            assert true.sum() > perm.sum()
    finally:
        m.close()
