"""LDA.predictive_log_likelihood on the GPU (csrc/heldout_kernels.h): per-document values against the
restatement (tests/heldout_host.py) from the gamma the call returns, gamma bitwise that of
update_variables, the row sums after training, the closed form of identical topics, the model's
state left alone, the sample -> train -> evaluate loop, and the surface."""
import numpy as np
import pytest

import heldout_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipdev():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return 0


def _model(K, V, alpha=.1, eta=.3, lam=None, seed=1, cls=None):
    from trlda_amd.models import OnlineLDA
    if cls is None:
        m = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=alpha, eta=eta, device=0)
    else:
        m = cls(num_words=V, num_topics=K, alpha=alpha, eta=eta, device=0)
    if lam is None:
        lam = np.random.RandomState(seed).gamma(2.0, 1.0, size=(K, V)) + 0.05
    m.lambdas = lam
    return m


def _csr(lengths, V, rng, zero_every=0, first_last=False):
    from trlda_amd.documents import CSRDocuments
    lengths = np.asarray(lengths, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    ids = rng.randint(0, V, size=indptr[-1])
    cnts = rng.randint(1, 5, size=indptr[-1])
    if zero_every:
        cnts[::zero_every] = 0
    if first_last:
        for d in range(len(lengths)):
            if lengths[d] >= 2:
                ids[indptr[d]] = 0
                ids[indptr[d + 1] - 1] = V - 1
            if lengths[d] >= 4:
                ids[indptr[d] + 1] = ids[indptr[d] + 2]       # a duplicate id
    return CSRDocuments(indptr, ids, cnts)


def _device_predictive(model, observed, heldout, g0, max_iter=20, threshold=1e-3):
    """The C path: (gamma, loglik, tokens)."""
    from trlda_amd import _ffi
    L = _ffi.lib()
    B = g0.shape[1]
    gamma = np.array(g0, dtype=np.float64, order="F", copy=True)
    loglik = np.full(B, np.nan)
    tokens = np.full(B, np.nan)
    ob, hb = model.upload(observed), model.upload(heldout)
    try:
        _ffi.check(L.trlda_model_predictive(model._handle, ob.handle, hb.handle, gamma, max_iter,
                                            threshold, loglik, tokens))
    finally:
        ob.close()
        hb.close()
    return gamma, loglik, tokens


def _close(dev, host, rel=1e-12):
    return bool(np.all(np.abs(dev - host) <= rel * np.abs(host) + 1e-300))


def _g0(K, B, seed):
    return np.asfortranarray(np.random.RandomState(seed).gamma(1.0, 1.0, size=(K, B)) + 0.1)


HELD_LENGTHS = [0, 1, 63, 64, 65, 1100, 5, 12, 0, 30]


@pytest.mark.parametrize("K", [1, 7, 64, 100, 128, 129, 512, 600, 1000])
def test_against_the_restatement(hipdev, K):
    V = 3000
    rng = np.random.RandomState(K)
    B = len(HELD_LENGTHS)
    obs_len = rng.poisson(40, size=B)
    obs_len[[2, 6]] = 0                                          # observed part empty
    observed = _csr(obs_len, V, rng)
    heldout = _csr(HELD_LENGTHS, V, rng, zero_every=7, first_last=True)
    m = _model(K, V, seed=K)
    lam = np.asarray(m.lambdas)
    g0 = _g0(K, B, K + 1)
    gamma, loglik, tokens = _device_predictive(m, observed, heldout, g0)
    g_ref, _ = m.update_variables(observed, latents=g0, max_iter=20, threshold=1e-3)
    m.close()
    assert np.array_equal(gamma, np.asarray(g_ref))              # gamma bitwise that of the E-step
    want_ll, want_tok = heldout_host.score(heldout.indptr, heldout.ids, heldout.cnts, gamma, lam)
    assert np.array_equal(tokens, want_tok)
    assert _close(loglik, want_ll), np.max(np.abs(loglik - want_ll) / np.maximum(np.abs(want_ll), 1e-300))
    assert loglik[0] == 0 and tokens[0] == 0 and loglik[8] == 0


def test_results_do_not_depend_on_the_batch(hipdev):
    """A document's value is a function of its own gamma column, lambda and entries."""
    K, V, B = 100, 3000, 40
    rng = np.random.RandomState(3)
    observed = _csr(rng.poisson(30, size=B), V, rng)
    heldout = _csr(rng.poisson(20, size=B), V, rng)
    m = _model(K, V)
    g0 = _g0(K, B, 5)
    _, ll, tok = _device_predictive(m, observed, heldout, g0)
    _, ll2, tok2 = _device_predictive(m, observed, heldout, g0)
    lo, hi = 13, 29
    _, ll3, tok3 = _device_predictive(m, observed.slice(lo, hi), heldout.slice(lo, hi), g0[:, lo:hi])
    m.close()
    assert np.array_equal(ll, ll2) and np.array_equal(tok, tok2)
    assert np.array_equal(ll[lo:hi], ll3) and np.array_equal(tok[lo:hi], tok3)


@pytest.mark.parametrize("K,V", [(100, 2000), (300, 15000)])
def test_row_sums_after_training(hipdev, K, V):
    """update_parameters leaves carried or handed-over row sums behind: the kernel must read the
    ones of the current lambda."""
    import trlda_amd
    rng = np.random.RandomState(K)
    B = 200
    train = _csr(rng.poisson(50, size=B), V, rng)
    observed = _csr(rng.poisson(30, size=50), V, rng)
    heldout = _csr(rng.poisson(15, size=50), V, rng)
    trlda_amd.seed(17)
    m = _model(K, V, seed=2)
    for _ in range(2):
        m.update_parameters(train, max_iter_tr=10, max_iter_inference=20)
    g0 = _g0(K, 50, 8)
    gamma, loglik, tokens = _device_predictive(m, observed, heldout, g0)
    lam = np.asarray(m.lambdas)
    m.close()
    want_ll, want_tok = heldout_host.score(heldout.indptr, heldout.ids, heldout.cnts, gamma, lam)
    assert np.array_equal(tokens, want_tok)
    assert _close(loglik, want_ll)


@pytest.mark.parametrize("K", [1, 50, 700])
def test_identical_topics_give_the_unigram_score(hipdev, K):
    V, B = 1000, 30
    rng = np.random.RandomState(K)
    row = rng.gamma(0.7, 1.0, size=V) + 1e-3
    m = _model(K, V, lam=np.tile(row, (K, 1)))
    observed = _csr(rng.poisson(20, size=B), V, rng)
    heldout = _csr(rng.poisson(20, size=B), V, rng, zero_every=5)
    _, loglik, tokens = _device_predictive(m, observed, heldout, _g0(K, B, 1))
    score = m.predictive_log_likelihood(observed, heldout)        # whatever gamma
    m.close()
    doc = np.repeat(np.arange(B), np.diff(heldout.indptr))
    c = heldout.cnts.astype(np.float64)
    want = np.bincount(doc, weights=c * np.log(row[heldout.ids] / row.sum()), minlength=B)
    assert _close(loglik, want, 1e-12)
    assert abs(score - want.sum() / c.sum()) <= 1e-12 * abs(score)


def _split_pair(V, B, seed):
    rng = np.random.RandomState(seed)
    return _csr(rng.poisson(30, size=B), V, rng), _csr(rng.poisson(10, size=B), V, rng)


def test_state_is_left_alone(hipdev):
    K, V, B = 64, 2000, 50
    observed, heldout = _split_pair(V, B, 4)
    m = _model(K, V, alpha=.2, eta=.05)
    lam, alpha, eta, count = np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count
    m.predictive_log_likelihood(observed, heldout, latents=_g0(K, B, 2))
    m.predictive_log_likelihood(observed, heldout)
    assert np.array_equal(np.asarray(m.lambdas), lam)
    assert np.array_equal(np.asarray(m.alpha), alpha) and m.eta == eta and m.update_count == count
    m.close()


@pytest.mark.parametrize("K", [64, 300])
def test_updates_around_it_are_unchanged(hipdev, K):
    """update, predictive, update gives bitwise the lambda of update, update."""
    import trlda_amd
    V, B = 3000, 100
    rng = np.random.RandomState(9)
    train = [_csr(rng.poisson(40, size=B), V, rng) for _ in range(2)]
    observed, heldout = _split_pair(V, 30, 5)
    lams = []
    for between in (False, True):
        trlda_amd.seed(31)
        m = _model(K, V, seed=3)
        m.update_parameters(train[0], max_iter_tr=10, max_iter_inference=20)
        if between:
            m.predictive_log_likelihood(observed, heldout, latents=_g0(K, 30, 6))
        m.update_parameters(train[1], max_iter_tr=10, max_iter_inference=20)
        lams.append(np.asarray(m.lambdas).copy())
        m.close()
    assert np.array_equal(lams[0], lams[1])


def test_default_latents_consume_the_stream_like_update_variables(hipdev):
    import ctypes
    import trlda_amd
    from trlda_amd import _ffi
    L = _ffi.lib()
    K, V, B = 20, 1000, 40
    observed, heldout = _split_pair(V, B, 6)
    m = _model(K, V)
    key = ctypes.c_uint64()
    trlda_amd.seed(123)
    s1 = m.predictive_log_likelihood(observed, heldout)
    L.trlda_rng_draw_key(ctypes.byref(key))
    after_predictive = key.value
    trlda_amd.seed(123)
    m.update_variables(observed)
    L.trlda_rng_draw_key(ctypes.byref(key))
    assert key.value == after_predictive
    trlda_amd.seed(123)
    g0 = np.empty((K, B), dtype=np.float64, order="F")
    L.trlda_sample_gamma_init(K, B, g0)
    s2 = m.predictive_log_likelihood(observed, heldout, latents=g0)
    m.close()
    assert s1 == s2


def test_after_a_stream_pass_with_deferred_statistics_and_lanes(hipdev):
    import torch
    from trlda_amd.stream import EStepStream
    K, V, B = 100, 3000, 120
    rng = np.random.RandomState(12)
    lam = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    csrs = [_csr(rng.poisson(60, size=B), V, rng) for _ in range(5)]
    observed, heldout = _split_pair(V, 40, 7)
    g0 = _g0(K, 40, 3)
    fresh = _model(K, V, lam=lam)
    want = fresh.predictive_log_likelihood(observed, heldout, latents=g0, return_documents=True)
    fresh.close()
    m = _model(K, V, lam=lam)
    dev = torch.device("cuda", 0)
    batches = [m.upload(c) for c in csrs]
    g0_t = [torch.from_numpy(np.ascontiguousarray(_g0(K, B, 50 + i).T)).to(dev) for i in range(5)]
    gam = [torch.empty(B, K, dtype=torch.float64, device=dev) for _ in csrs]
    sst = [torch.empty(V, K, dtype=torch.float64, device=dev) for _ in csrs]
    with EStepStream(m, lanes=2, deferred=True) as s:
        for i, b in enumerate(batches):
            s.step(b, batches[i + 1:i + 3], g0_t[i], gam[i], sst[i], max_iter=20)
        inside = m.predictive_log_likelihood(observed, heldout, latents=g0, return_documents=True)
    torch.cuda.synchronize()
    after = m.predictive_log_likelihood(observed, heldout, latents=g0, return_documents=True)
    for b in batches:
        b.close()
    m.close()
    for got in (inside, after):
        assert got[0] == want[0]
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_planted_beats_trained_beats_untrained(hipdev):
    """sample -> train -> evaluate: a fresh model trained on a planted model's corpus scores between
    the planted model and an untrained one on held-out words of that corpus."""
    import trlda_amd
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils import split_documents
    K, V = 10, 2000
    lam = np.full((K, V), 1e-3)
    for k in range(K):
        lam[k, k * 200:(k + 1) * 200] = 1000.0
    planted = _model(K, V, alpha=0.1, lam=lam)
    trlda_amd.seed(9)
    train = planted.sample(2000, 100)
    test = planted.sample(500, 100)
    observed, heldout = split_documents(test, 0.2)
    untrained = OnlineLDA(num_words=V, num_topics=K, num_documents=2000, alpha=0.1, eta=0.3, device=0)
    trained = OnlineLDA(num_words=V, num_topics=K, num_documents=2000, alpha=0.1, eta=0.3, device=0)
    trained.lambdas = np.asarray(untrained.lambdas)
    train_list = list(train)
    for _ in range(3):
        for i in range(0, 2000, 250):
            trained.update_parameters(train_list[i:i + 250], max_iter_tr=10, kappa=0.5, tau=1.)
    scores = [mdl.predictive_log_likelihood(observed, heldout) for mdl in (planted, trained, untrained)]
    for mdl in (planted, trained, untrained):
        mdl.close()
    assert np.isfinite(scores).all()
    assert scores[0] > scores[1] > scores[2], scores


def test_surface(hipdev):
    import trlda.models
    from trlda_amd.models import BatchLDA, CumulativeLDA, OnlineLDA
    K, V, B = 30, 1500, 25
    observed, heldout = _split_pair(V, B, 8)
    lam = np.random.RandomState(2).gamma(2.0, 1.0, size=(K, V)) + 0.05
    g0 = _g0(K, B, 4)
    results = []
    for cls in (OnlineLDA, BatchLDA, CumulativeLDA, trlda.models.OnlineLDA, trlda.models.BatchLDA):
        m = _model(K, V, lam=lam, cls=None if cls in (OnlineLDA, trlda.models.OnlineLDA) else cls)
        results.append(m.predictive_log_likelihood(observed, heldout, latents=g0, return_documents=True))
        if cls is OnlineLDA:
            ob, hb = m.upload(observed), m.upload(heldout)
            on_device = m.predictive_log_likelihood(ob, hb, latents=g0, return_documents=True)
            as_lists = m.predictive_log_likelihood(observed.to_list(), heldout.to_list(), latents=g0,
                                                   return_documents=True)
            ob.close()
            hb.close()
        m.close()
    score, ll, tok = results[0]
    assert isinstance(score, float) and ll.dtype == np.float64 and ll.shape == (B,) and tok.shape == (B,)
    assert abs(score - ll.sum() / tok.sum()) <= 1e-14 * abs(score)
    for other in results[1:] + [on_device, as_lists]:
        assert other[0] == score and np.array_equal(other[1], ll) and np.array_equal(other[2], tok)


def test_errors(hipdev):
    from trlda_amd import _ffi
    from trlda_amd.documents import DeviceBatch
    K, V, B = 8, 500, 6
    observed, heldout = _split_pair(V, B, 10)
    m = _model(K, V)
    with pytest.raises(RuntimeError, match="equal in number"):
        m.predictive_log_likelihood(observed, heldout.slice(0, B - 1))
    with pytest.raises(RuntimeError, match="Initial gamma has wrong dimensionality."):
        m.predictive_log_likelihood(observed, heldout, latents=np.ones((K, B + 1)))
    nothing = heldout.to_list()
    nothing = [[(w, 0) for w, _ in doc] for doc in nothing]
    with pytest.raises(RuntimeError, match="no held-out tokens"):
        m.predictive_log_likelihood(observed, nothing)
    with pytest.raises(RuntimeError, match="no held-out tokens"):
        m.predictive_log_likelihood([], [])
    # the C checks
    L = _ffi.lib()
    g = np.ones((K, B), order="F")
    out1, out2 = np.zeros(B), np.zeros(B)
    ob, hb = m.upload(observed), m.upload(heldout)
    other = DeviceBatch(heldout, V + 1, 0)
    short = m.upload(heldout.slice(0, B - 1))
    empty = m.upload([])
    assert L.trlda_model_predictive(m._handle, None, hb.handle, g, 10, 1e-3, out1, out2) == _ffi.ERR_ARG
    assert L.trlda_model_predictive(m._handle, ob.handle, None, g, 10, 1e-3, out1, out2) == _ffi.ERR_ARG
    assert L.trlda_model_predictive(m._handle, ob.handle, short.handle, g, 10, 1e-3, out1, out2) == _ffi.ERR_ARG
    assert L.trlda_model_predictive(m._handle, empty.handle, empty.handle, g, 10, 1e-3, out1, out2) == \
        _ffi.ERR_ARG
    assert L.trlda_model_predictive(m._handle, ob.handle, other.handle, g, 10, 1e-3, out1, out2) == _ffi.ERR_ARG
    # the model still works after the refusals
    assert np.isfinite(m.predictive_log_likelihood(observed, heldout))
    for b in (ob, hb, other, short, empty):
        b.close()
    m.close()
