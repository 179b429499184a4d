"""Gibbs inside the update loops on the GPU: OnlineLDA / BatchLDA .update_parameters(...,
inference_method='gibbs') (reference src/onlinelda.cpp:53-179, src/batchlda.cpp:43-61;
csrc/gibbs_kernels.h, gibbs_mstep_kernel) against the NumPy restatement of tests/gibbs_update_host.py."""
import ctypes as C

import numpy as np
import pytest

import gibbs_update_host as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipdev():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return 0


def _docs(rng, B, V, max_len=6, max_cnt=4):
    docs = []
    for _ in range(B):
        n = rng.randint(1, max_len + 1)
        docs.append([(int(rng.randint(V)), int(rng.randint(1, max_cnt + 1))) for _ in range(n)])
    return docs


def _keys(seed, n):
    """The keys trlda_rng_draw_key gives after trlda.seed(seed)."""
    import trlda
    from trlda_amd import _ffi
    trlda.seed(seed)
    out = []
    for _ in range(n):
        k = C.c_uint64(0)
        _ffi.check(_ffi.lib().trlda_rng_draw_key(C.byref(k)))
        out.append(k.value)
    return out


def _table(model):
    from trlda_amd import _ffi
    e = np.empty((model.num_topics, model.num_words), order="F")
    _ffi.check(_ffi.lib().trlda_debug_gibbs_table(model._handle, e))
    return e


def _sstats(model):
    from trlda_amd import _ffi
    s = np.empty((model.num_topics, model.num_words), order="F")
    _ffi.check(_ffi.lib().trlda_model_get_sstats(model._handle, s))
    return s


def _online(K, V, seed, lam):
    from trlda_amd.models import OnlineLDA
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=5000, alpha=.1, eta=.3, device=0)
    m.lambdas = lam
    return m


def _close(a, b):
    return np.allclose(a, b, rtol=1e-12, atol=0)


def _check_table(e, seen, docs, oracle):
    """The table the last E-step read (from the row sums the inactive pass and the M-steps left) is
    exp(psi(lambda) - psi(rowsum(lambda))) of the lambda that E-step saw, to 1e-12 relative."""
    words = np.unique([w for d in docs for w, _ in d])
    want = gu.table(seen, words, oracle.digamma)[:, words]
    assert np.allclose(e[:, words], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("ns,bi", [(1, 2), (3, 0), (0, 2)])
@pytest.mark.parametrize("K", [1, 3, 64, 100, 500, 1000])
def test_online_and_batch_match_the_restatement(hipdev, oracle, K, ns, bi):
    import trlda
    V = 40
    rng = np.random.RandomState(K * 10 + ns)
    docs = _docs(rng, 6, V)
    lam0 = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    alpha = np.full(K, .1)
    for T, init in [(0, True), (1, True), (3, True), (3, False)]:
        seed = 1000 + K + T
        m = _online(K, V, seed, lam0)
        keys = _keys(seed, max(T, 1))
        trlda.seed(seed)
        rho = m.update_parameters(docs, max_iter_tr=T, init_gamma=init, inference_method='gibbs',
                                  num_samples=ns, burn_in=bi, adaptive=(T == 1), rho=(0.4 if T == 1 else -1.))
        assert m.update_count == 1
        want_rho = 0.4 if T == 1 else gu.online_rho(0, .7, 100.)
        assert rho == want_rho
        e = _table(m)
        lam, sstats, _, _, seen = gu.online(lam0, alpha, .3, docs, 5000, want_rho, T, init, ns, bi, keys,
                                            oracle.digamma, last_table=e)
        assert _close(m.lambdas, lam), (K, ns, bi, T, init)
        _check_table(e, seen, docs, oracle)
        if T == 1:                                 # keep_sstats on (adaptive): the statistics stay
            assert np.array_equal(_sstats(m), sstats)
        m.close()
    for epochs in (1, 3):
        from trlda_amd.models import BatchLDA
        seed = 2000 + K + epochs
        m = BatchLDA(num_words=V, num_topics=K, alpha=.1, eta=.3, device=0)
        m.lambdas = lam0
        keys = _keys(seed, epochs)
        trlda.seed(seed)
        m.update_parameters(docs, max_epochs=epochs, inference_method='g', num_samples=ns, burn_in=bi)
        e = _table(m)
        lam, _, _, _, seen = gu.batch(lam0, alpha, .3, docs, epochs, ns, bi, keys, oracle.digamma,
                                      last_table=e)
        assert _close(m.lambdas, lam), (K, ns, bi, epochs)
        _check_table(e, seen, docs, oracle)
        m.close()


@pytest.mark.parametrize("T", [2, 0])
def test_adaptive_rate_and_eta(hipdev, oracle, T):
    """Five online Gibbs updates with adaptive=True, update_eta=True (max_iter_tr = 2, and 0: the
    branch that copies lambda' whole) match the restatement's rho sequence and eta to 1e-12: the
    adaptive rate (onlinelda.cpp:167-175) from the restatement's statistics, lambda' and running
    gradient, and the Newton step on eta (:147-162) from its lambda."""
    import trlda
    K, V, D = 20, 300, 5000
    rng = np.random.RandomState(5 + T)
    batches = [_docs(rng, 40, V, max_len=10) for _ in range(5)]
    lam0 = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    alpha = np.full(K, .1)
    m = _online(K, V, 1, lam0)
    keys = _keys(77, 5 * max(T, 1))
    trlda.seed(77)
    rhos, etas = [], []
    for b in batches:
        rhos.append(m.update_parameters(b, max_iter_tr=T, inference_method='gibbs', adaptive=True,
                                        update_eta=True))
        etas.append(m.eta)
    lam_dev = m.lambdas.copy()
    m.close()
    ada = gu.Adaptive((K, V))
    lam, eta = lam0, .3
    for i, b in enumerate(batches):
        rho = ada.rho                                       # onlinelda.cpp:61-62
        assert abs(rhos[i] - rho) <= 1e-12 * rho, (i, rhos[i], rho)
        n = max(T, 1)
        new, sstats, _, _, _ = gu.online(lam, alpha, eta, b, D, rho, T, True, 1, 2,
                                         keys[i * n:(i + 1) * n], oracle.digamma)
        eta_new = gu.eta_step(new, eta, rho, oracle.digamma)
        ada.step(eta + float(D) / len(b) * sstats, lam)    # lambdaHat with the eta of the update
        lam, eta = new, eta_new
        assert abs(etas[i] - eta) <= 1e-12 * eta, (i, etas[i], eta)
    assert len(set(rhos)) == 5
    assert _close(lam_dev, lam)


@pytest.mark.parametrize("K,V", [(32, 400), (200, 3000)])
def test_vi_after_gibbs_is_vi_on_the_same_lambda(hipdev, K, V):
    """A stream of VI E-steps with deferred statistics and two lanes (EStepStream) leaves work
    pending and announces the Gibbs batch and a later VI batch; then a Gibbs update, a VI update,
    do_e_step and lower_bound.  The stream's results are those of the same stream on a model without
    the Gibbs update, and the VI results after it are bitwise those of a model whose lambda and
    update count are set to the Gibbs-trained values at that point, with the same stream before."""
    import torch
    import trlda
    from trlda_amd.stream import EStepStream
    rng = np.random.RandomState(K)
    B = 48
    vi_docs = [_docs(rng, B, V, max_len=25) for _ in range(3)]
    g_docs = _docs(rng, B, V, max_len=25)
    lam0 = rng.gamma(2.0, 1.0, size=(K, V)) + 0.05
    dev = torch.device("cuda", 0)
    g0 = [torch.from_numpy(np.ascontiguousarray(rng.gamma(100., .01, size=(B, K)))).to(dev)
          for _ in range(3)]

    def run(trained=None):
        m = _online(K, V, 1, lam0)
        batches = [m.upload(d) for d in vi_docs]
        gb = m.upload(g_docs)
        gam = [torch.empty(B, K, dtype=torch.float64, device=dev) for _ in range(3)]
        sst = [torch.empty(V, K, dtype=torch.float64, device=dev) for _ in range(3)]
        with EStepStream(m, lanes=2, deferred=True) as s:
            s.step(batches[0], [batches[1]], g0[0], gam[0], sst[0], max_iter=20)
            s.step(batches[1], [gb, batches[2]], g0[1], gam[1], sst[1], max_iter=20)
            if trained is None:
                trlda.seed(3)                      # statistics pending, gb and batches[2] announced
                m.update_parameters(gb, max_iter_tr=3, inference_method='gibbs')
                state = (m.lambdas.copy(), m.update_count)
            else:
                m.lambdas, m.update_count = trained
                state = trained
            trlda.seed(11)
            out = [m.update_parameters(batches[2], max_iter_tr=2), m.lambdas.copy()]
            out += list(m.do_e_step(batches[0], max_iter=20))
            out.append(m.lower_bound(batches[1]))
            s.step(batches[2], [], g0[2], gam[2], sst[2], max_iter=20)
        torch.cuda.synchronize()
        out += [t.cpu().numpy() for t in gam + sst]
        for b in batches + [gb]:
            b.close()
        m.close()
        return state, out

    state, a = run()
    assert not np.array_equal(state[0], lam0) and state[1] == 1
    _, b = run(state)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), i


def _draw_state():
    from trlda_amd import _ffi
    k = C.c_uint64(0)
    _ffi.check(_ffi.lib().trlda_rng_draw_key(C.byref(k)))
    return k.value


def test_errors_leave_everything_alone(hipdev):
    import trlda
    from trlda_amd import _ffi
    from trlda_amd.models import OnlineLDA, BatchLDA
    V = 50
    rng = np.random.RandomState(9)
    docs = _docs(rng, 5, V)
    m = _online(16, V, 1, rng.gamma(2.0, 1.0, size=(16, V)) + .05)
    bm = BatchLDA(num_words=V, num_topics=16, device=0)
    big = OnlineLDA(num_words=V, num_topics=1025, num_documents=100, device=0)
    cases = [
        (m, NotImplementedError, dict(inference_method='gibbs', update_alpha=True)),
        (bm, NotImplementedError, dict(inference_method='gibbs', update_alpha=True)),
        (m, RuntimeError, dict(inference_method='gibbs', num_samples=-1)),
        (bm, RuntimeError, dict(inference_method='gibbs', burn_in=-1)),
        (m, TypeError, dict(inference_method='map')),
        (big, _ffi.TrldaError, dict(inference_method='gibbs')),
    ]
    for model, exc, kw in cases:
        lam = model.lambdas.copy()
        count = getattr(model, "update_count", None)
        trlda.seed(5)
        with pytest.raises(exc) as info:
            model.update_parameters(docs, **kw)
        if model is big:
            assert "at most 1024 topics" in str(info.value)
        assert _draw_state() == _keys(5, 1)[0], kw            # the stream was not advanced
        assert np.array_equal(model.lambdas, lam), kw
        assert getattr(model, "update_count", None) == count
    big.close()
    bm.close()
    m.close()


def _hungarian_cos(a, b):
    """mean cosine of the best one-to-one matching of the rows of a and b (the Hungarian matching's
    optimum, found exactly by dynamic programming over subsets: K <= 10 here)."""
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    c = a @ b.T
    K = c.shape[0]
    best = np.full(1 << K, -np.inf)
    best[0] = 0.0
    for mask in range(1 << K):
        if best[mask] == -np.inf:
            continue
        i = bin(mask).count("1")
        if i >= K:
            continue
        for j in range(K):
            if not mask & (1 << j):
                nm = mask | (1 << j)
                best[nm] = max(best[nm], best[mask] + c[i, j])
    return best[-1] / K


def test_it_trains(hipdev):
    """50 online Gibbs updates on documents drawn from a known K = 10 model recover its topics.
    Thresholds from a first run, which showed a mean cosine of 0.9973 and a held-out log-likelihood
    per word from -6.215 to -4.834, set with a clear margin below it (0.95 and a rise of 1.0); the
    run is deterministic under its seed."""
    import trlda
    from trlda_amd.models import OnlineLDA
    K, V = 10, 500
    rng = np.random.RandomState(0)
    truth_lam = np.full((K, V), 0.01)
    for k in range(K):                                        # each topic 50 words of its own
        truth_lam[k, k * 50:(k + 1) * 50] = rng.gamma(5.0, 1.0, size=50)
    src = OnlineLDA(num_words=V, num_topics=K, num_documents=1, alpha=.1, eta=.01, device=0)
    src.lambdas = truth_lam * 100.
    trlda.seed(1)
    corpus = src.sample(5200, 60)
    src.close()
    train, held = corpus[:5000], corpus[5000:]
    obs = [d[:len(d) // 2] for d in held]
    out = [d[len(d) // 2:] for d in held]

    def run():
        trlda.seed(2)
        m = OnlineLDA(num_words=V, num_topics=K, num_documents=5000, alpha=.1, eta=.01, device=0)
        trlda.seed(3)
        before = m.predictive_log_likelihood(obs, out)
        for i in range(50):
            m.update_parameters(train[i * 100:(i + 1) * 100], max_iter_tr=3, kappa=.6, tau=1.,
                                inference_method='gibbs', num_samples=2, burn_in=3)
        trlda.seed(3)
        after = m.predictive_log_likelihood(obs, out)
        lam = m.lambdas.copy()
        m.close()
        return before, after, lam

    before, after, lam = run()
    cos = _hungarian_cos(lam, truth_lam)
    print("gibbs training: mean cosine %.4f, held-out %.4f -> %.4f" % (cos, before, after))
    assert cos > THRESH_COS
    assert after > before + THRESH_LL
    b2, a2, lam2 = run()
    assert (b2, a2) == (before, after) and np.array_equal(lam, lam2)


THRESH_COS = 0.95
THRESH_LL = 1.0
