"""LDA.left_to_right on the GPU (csrc/l2r_kernels.h): parity with the NumPy restatement
(tests/l2r_host.py) under the same key across the per-lane variants, the enumerated marginal of a
short document, the determinism rules and the random stream, the errors, and what the number
means."""
import ctypes as C
import math

import numpy as np
import pytest

import l2r_host as lh
from marginal_host import exact_log_marginal

pytestmark = pytest.mark.gpu

PARITY_RTOL = 1e-12         # every draw is shared and the weights take no transcendental function
T_BOUND = 9.0


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
    """Multiples of 2^-10 below 2: their row sums are exact in any order of addition, so the
    restatement's 1 / rs_k are the device's bits and so is every draw."""
    return np.asfortranarray(np.random.RandomState(seed).randint(1, 2048, (K, V)) / 1024.)


def _docs(V, seed, long_tokens=131):
    """test_gpu_marginal._docs' kinds: empty, short, an entry with c = 0, an id three times, all
    counts 0, one token, and one long document of `long_tokens` tokens."""
    rng = np.random.RandomState(seed)
    docs = [[]]
    for n in (1, 7):
        docs.append([(int(w), int(c)) for w, c in zip(rng.randint(0, V, n), rng.randint(1, 5, n))])
    docs.append([(int(w), 0 if i % 2 == 0 else 3) for i, w in enumerate(rng.randint(0, V, 6))])
    r = rng.randint(0, V, 9)
    r[[2, 5, 8]] = r[0]
    docs.append([(int(w), int(c)) for w, c in zip(r, rng.randint(1, 3, 9))])
    docs.append([(int(w), 0) for w in rng.randint(0, V, 3)])
    docs.append([(int(rng.randint(0, V)), 1)])
    long, left = [], long_tokens
    while left > 0:
        c = min(int(rng.randint(1, 4)), left)
        long.append((int(rng.randint(0, V)), c))
        left -= c
    docs.append(long)
    docs.append([])
    return docs


def _csr(docs):
    indptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int32)
    ids = np.array([w for d in docs for w, _ in d], dtype=np.int32)
    cnts = np.array([c for d in docs for _, c in d], dtype=np.int32)
    return indptr, ids, cnts


def _tokens(docs):
    return np.array([float(sum(c for _, c in d)) for d in docs])


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


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# --------------------------------------------------------------------------------------------
# 1. parity with the restatement
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5, 8])
@pytest.mark.parametrize("K,V", [(3, 50), (64, 120), (65, 120), (100, 300), (1024, 60)])
def test_parity_with_the_restatement(hip, K, V, R):
    """Device loglik against l2r_host under the same key, both `resample` values and both
    combinations: 1e-12 relative (the draws and the weights are shared bit for bit, the logarithms
    are not; a flipped draw would show as a gross error).  K = 3, 64 (one topic per lane and its
    edge), 65 and 100 (two), 1024 (sixteen, the limit); R = 5 leaves a workgroup's last wave without
    an item and puts two documents' particles into one workgroup.  The long document has 131 tokens:
    its prefix passes through the lanes in three chunks.  Token counts are exact.  Observed maximum
    over all cases: 2.2e-16 (K = 1024, R = 5); ten of the fifteen agree bit for bit."""
    import trlda_amd
    lam = _lambda(K, V, K)
    alpha = np.random.RandomState(K + 1).gamma(2., .1, K) + .02
    docs = _docs(V, K + 2)
    indptr, ids, cnts = _csr(docs)
    B = len(docs)
    assert _tokens(docs)[7] == 131
    m = _model(K, V, lam, alpha=alpha)
    batch = m.upload(docs)
    try:
        worst = 0.
        for resample in (True, False):
            trlda_amd.seed(100 + K)
            key = _key()
            want, want_tokens = lh.left_to_right(indptr, ids, cnts, lam, alpha, key, R, resample)
            for combine in ("particle", "position"):
                trlda_amd.seed(100 + K)
                ll, tokens = m.left_to_right(batch, num_particles=R, resample=resample, combine=combine,
                                             return_tokens=True)
                assert ll.shape == (B,) and ll.dtype == np.float64 and tokens.dtype == np.float64
                assert np.array_equal(tokens, want_tokens) and np.array_equal(tokens, _tokens(docs))
                full = tokens > 0
                assert np.all(ll[~full] == 0.0) and np.all(want[combine][~full] == 0.0)
                assert np.all(np.isfinite(ll)) and np.all(ll[full] < 0)
                err = _rel(ll[full], want[combine][full])
                worst = max(worst, err)
                assert err < PARITY_RTOL, (K, R, resample, combine, err)
                if R == 1:
                    first = ll if combine == "particle" else first
                    assert np.array_equal(ll, first)            # one particle: the same bits
        print("K=%d R=%d: max rel err loglik %.3e" % (K, R, worst))
    finally:
        batch.close()
        m.close()


# --------------------------------------------------------------------------------------------
# 2. exactness: the enumerated marginal of a 6-token document
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 4])
def test_exact_marginal_of_a_short_document(hip, R):
    """The CPU test of test_l2r_host.py through the model: the K = 3 document 20 000 times in one
    batch (d supplies independent streams), resample, combine='particle'; R_d = exp(loglik_d -
    exact).  Their mean is within t = 9 SE of 1, SE from the spread of the means of 20 groups of
    1 000 documents.  The same batch with combine='position' is printed, not asserted: it is biased
    for R > 1 (at R = 1 it is the same bits).  Observed |mean - 1| / SE: 'particle' 0.45 (mean 1.00175,
    SE 3.9e-3) at R = 1 and 0.50 (1.00089, 1.8e-3) at R = 4; 'position' 6.76 (0.98798, 1.8e-3) at R = 4."""
    import trlda_amd
    lam = np.array([[5., 1., 2., .5], [1., 4., 1., 3.], [2., 2., 6., 1.]])
    alpha = np.array([0.5, 0.2, 1.0])
    doc = [(0, 2), (1, 1), (2, 2), (3, 1)]
    words = [0, 0, 1, 2, 2, 3]
    exact = exact_log_marginal(lam / lam.sum(axis=1)[:, None], alpha, words)
    m = _model(3, 4, lam, alpha=alpha)
    batch = m.upload([doc] * 20000)
    try:
        trlda_amd.seed(5)
        ll = m.left_to_right(batch, num_particles=R, resample=True, combine="particle")
        trlda_amd.seed(5)
        pos = m.left_to_right(batch, num_particles=R, resample=True, combine="position")
    finally:
        batch.close()
        m.close()
    for name, x in (("particle", ll), ("position", pos)):
        ratio = np.exp(x - exact)
        se = ratio.reshape(20, 1000).mean(axis=1).std(ddof=1) / math.sqrt(20)
        print("R=%d %s: mean %.6f SE %.3e |mean - 1| / SE %.3f, mean(ll) - exact %.4f" %
              (R, name, ratio.mean(), se, abs(ratio.mean() - 1) / se, x.mean() - exact))
    ratio = np.exp(ll - exact)
    se = ratio.reshape(20, 1000).mean(axis=1).std(ddof=1) / math.sqrt(20)
    assert se > 0 and abs(ratio.mean() - 1.0) <= T_BOUND * se, (ratio.mean(), se)
    if R == 1:
        assert np.array_equal(ll, pos)


# --------------------------------------------------------------------------------------------
# 3. invariants
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", [True, False])
def test_determinism_and_the_random_stream(hip, resample, monkeypatch):
    import trlda_amd
    K, V, R = 30, 200, 5
    lam = _lambda(K, V, 1)
    docs = _docs(V, 2, long_tokens=150)
    B = len(docs)
    kw = dict(num_particles=R, resample=resample)
    m = _model(K, V, lam)
    try:
        lam_before, alpha_before = np.array(m.lambdas), m.alpha
        eta_before, count_before = m.eta, m.update_count
        trlda_amd.seed(17)
        a = m.left_to_right(docs, **kw)
        got = _state()
        trlda_amd.seed(17)
        _key()
        assert np.array_equal(got, _state())            # exactly one key
        trlda_amd.seed(17)
        b = m.left_to_right(docs, **kw)
        assert np.array_equal(a, b)                     # the same seed: the same bits
        trlda_amd.seed(18)
        c = m.left_to_right(docs, **kw)
        full, many = _tokens(docs) > 0, _tokens(docs) > 1
        assert np.all(a[many] != c[many])               # another seed: other values
        assert np.array_equal(a[full & ~many], c[full & ~many])   # (one token: no draw in its value)
        assert np.all(a[~full] == 0.0)
        # DeviceBatch and list input
        batch = m.upload(docs)
        trlda_amd.seed(17)
        e = m.left_to_right(batch, **kw)
        batch.close()
        assert np.array_equal(a, e)
        # a document at the same index of a larger batch: the same bits
        more = docs + _docs(V, 3, long_tokens=80)
        trlda_amd.seed(17)
        big = m.left_to_right(more, **kw)
        assert np.array_equal(a, big[:B])
        # a workspace that holds little more than the longest document: many groups, the same bits
        monkeypatch.setenv("TRLDA_L2R_BUDGET", str(150 * R + 7))
        trlda_amd.seed(17)
        cut = m.left_to_right(more, **kw)
        got = _state()
        monkeypatch.delenv("TRLDA_L2R_BUDGET")
        assert np.array_equal(big, cut)
        trlda_amd.seed(17)
        _key()
        assert np.array_equal(got, _state())
        # the model is as it was
        assert np.array_equal(lam_before, m.lambdas) and np.array_equal(alpha_before, m.alpha)
        assert m.eta == eta_before and m.update_count == count_before
        # an empty batch is a valid call: one key, no values
        trlda_amd.seed(21)
        none, tokens = m.left_to_right([], return_tokens=True, **kw)
        got = _state()
        trlda_amd.seed(21)
        _key()
        assert none.shape == (0,) and tokens.shape == (0,) and np.array_equal(got, _state())
    finally:
        m.close()


# --------------------------------------------------------------------------------------------
# 4. errors: each before anything is drawn
# --------------------------------------------------------------------------------------------
def test_errors_draw_nothing(hip, monkeypatch):
    import trlda_amd
    from trlda_amd import _ffi
    K, V = 3, 20
    m = _model(K, V, _lambda(K, V, 5))
    docs = [[(1, 2), (3, 1)], [], [(2, 9)]]
    batch = m.upload(docs)
    try:
        trlda_amd.seed(3)
        before = _state()

        def refused(exc, match=None, **kw):
            with pytest.raises(exc, match=match) as info:
                m.left_to_right(batch, **kw)
            assert np.array_equal(before, _state())
            return info.value

        refused(RuntimeError, "num_particles", num_particles=0)
        refused(RuntimeError, "num_particles", num_particles=-3)
        refused(RuntimeError, "2\\^32", num_particles=2 ** 31)          # 3 documents
        refused(TypeError, "combine", combine="wallach")
        refused(TypeError, "combine", combine=1)
        refused(TypeError, "combine", combine=None)
        # a single document beyond the workspace: refused, and the message names the limit
        monkeypatch.setenv("TRLDA_L2R_BUDGET", "17")
        err = refused(_ffi.TrldaError, "17 token-particles", num_particles=2)
        assert err.code == _ffi.ERR_ARG
        monkeypatch.delenv("TRLDA_L2R_BUDGET")
        # the C entry refuses the same on its own
        ll = np.empty(3)
        for R, combine in ((0, _ffi.L2R_PARTICLE), (-1, _ffi.L2R_POSITION), (4, 7), (4, -1),
                           (2 ** 31 - 1, _ffi.L2R_PARTICLE)):
            rc = hip.trlda_model_left_to_right(m._handle, batch.handle, R, 1, combine, ll, None)
            assert rc == _ffi.ERR_ARG, (R, combine, rc)
            assert np.array_equal(before, _state())
        assert hip.trlda_model_left_to_right(m._handle, None, 4, 1, _ffi.L2R_PARTICLE, ll, None) == _ffi.ERR_ARG
        assert np.array_equal(before, _state())
        # tokens may be NULL
        _ffi.check(hip.trlda_model_left_to_right(m._handle, batch.handle, 4, 1, _ffi.L2R_PARTICLE, ll, None))
        assert np.isfinite(ll[0]) and ll[0] < 0 and ll[1] == 0.0
        # case-insensitive names
        trlda_amd.seed(3)
        a = m.left_to_right(batch, num_particles=4, combine="POSITION")
        trlda_amd.seed(3)
        assert np.array_equal(a, m.left_to_right(batch, num_particles=4, combine="position"))
    finally:
        batch.close()
        m.close()


def test_above_the_gibbs_limit(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K = 1025
    m = _model(K, 3, np.ones((K, 3)))
    try:
        trlda_amd.seed(3)
        before = _state()
        with pytest.raises(_ffi.TrldaError, match="1024 topics") as info:
            m.left_to_right([[(0, 1)]], num_particles=2)
        assert info.value.code == _ffi.ERR_ARG and np.array_equal(before, _state())
        ll = np.empty(1)
        batch = m.upload([[(0, 1)]])
        rc = hip.trlda_model_left_to_right(m._handle, batch.handle, 2, 1, _ffi.L2R_PARTICLE, ll, None)
        batch.close()
        assert rc == _ffi.ERR_ARG and np.array_equal(before, _state())
    finally:
        m.close()


# --------------------------------------------------------------------------------------------
# 5. what the number means
# --------------------------------------------------------------------------------------------
def test_the_generating_model_scores_higher(hip):
    """Documents sampled from the model: the generating lambda explains them better than the same
    lambda with its word columns permuted, under the same seed.  The per-word perplexity is printed
    next to document_log_likelihood('vi')'s; nothing is asserted between the two estimators."""
    import trlda_amd
    K, V = 20, 400
    rng = np.random.RandomState(6)
    lam = np.asfortranarray(200. * rng.dirichlet(np.full(V, .05), K) + .01)
    m = _model(K, V, lam)
    try:
        trlda_amd.seed(31)
        docs = m.sample(200, 60)
        batch = m.upload(docs)
        trlda_amd.seed(32)
        true, tokens = m.left_to_right(batch, return_tokens=True)
        trlda_amd.seed(32)
        vi = m.document_log_likelihood(batch)
        m.lambdas = lam[:, rng.permutation(V)]
        trlda_amd.seed(32)
        perm = m.left_to_right(batch)
        batch.close()
        assert tokens.sum() == sum(c for d in docs for _, c in d)
        print("per-word perplexity: left_to_right %.2f (generating) %.2f (permuted); "
              "document_log_likelihood('vi') %.2f (generating)" %
              (math.exp(-true.sum() / tokens.sum()), math.exp(-perm.sum() / tokens.sum()),
               math.exp(-vi.sum() / tokens.sum())))
        assert np.all(np.isfinite(true)) and np.all(np.isfinite(perm))
        assert true.sum() > perm.sum()
    finally:
        m.close()
