"""The variational path above 512 topics against the oracle: the general document kernel
(estep_docs_kernel), the two-kernel preamble, the segmented statistics (sstats_words_kernel) and the
element-wise M-step passes, which the fused and streaming kernels (K <= 512) leave to themselves there.

K runs from 513 up to the library's bound TRLDA_VI_MAX_TOPICS (read from the library): across the
preamble's LDS limits (9 K doubles up to K = 2272, K doubles beyond), the statistics kernel's (8, 4, 2
waves of K partial sums per workgroup), and the document kernel's word cap n_cap, which falls from 36
words at K = 513 to none from K = 5111.  Documents are made around n_cap.  Above the bound every VI
entry point fails with TRLDA_ERR_ARG before it draws, copies or launches anything.  All in this
process: no subprocesses."""
import ctypes as C
import math

import numpy as np
import pytest

import elbo_host
import heldout_host
from helpers import TIGHT_RTOL, HipSampler, relerr, seeded_gamma

pytestmark = pytest.mark.gpu

GEN = "estep_docs_kernel"
LDS_DYN_BYTES = 160 * 1024 - 256          # what a launch may ask for (csrc/trlda_hip.hip, kLdsDynBytes)
KMAX = "kmax"                             # stands for the library's TRLDA_VI_MAX_TOPICS


@pytest.fixture(scope="module")
def hip(hip_lib):
    from trlda_amd import _ffi
    assert _ffi.device_count() >= 1, "GPU tests need a visible MI355X"
    return hip_lib


@pytest.fixture(scope="module")
def sampler(hip):
    return HipSampler(hip)


@pytest.fixture(scope="module")
def k_max(hip):
    from trlda_amd import _ffi
    k = _ffi.vi_max_topics()
    assert k >= 4096 and n_cap(k) == 0
    return k


def n_cap(K, T=256):
    """Words of a document the general kernel keeps in LDS at K (csrc/trlda_hip.hip, docs_lds_bytes):
    beta[n][K | 1] | g[K] | e[K] | tw[n] | cnt[n] | part[max(T, K)] | wsum[T / 64]"""
    fixed = (2 * K + max(T, K) + T // 64) * 8
    return 0 if fixed >= LDS_DYN_BYTES else (LDS_DYN_BYTES - fixed) // (((K | 1) + 2) * 8)


def random_lambda(K, V, seed):
    # (the libc-stream sampler would need K V 100 draws: 3e8 at K = 6814, V = 400)
    rng = np.random.RandomState(seed)
    return np.asfortranarray(rng.gamma(100., .01, (K, V)))


def corpus(B, V, seed, mean_unique=40):
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.utils.synthetic import make_corpus
    return CSRDocuments(*make_corpus(B, V, seed=seed, mean_unique=mean_unique))


def edge_docs(K, V, seed, T=256):
    """Documents of 0, 1, n_cap - 1, n_cap, n_cap + 1, 3 n_cap and 300 distinct words, one with zero
    counts among its entries, one with an id three times"""
    from trlda_amd.documents import CSRDocuments
    rng = np.random.RandomState(seed)
    c = n_cap(K, T)
    lengths = [n for n in (0, 1, c - 1, c, c + 1, 3 * c, 300) if n >= 0]
    ids = [rng.choice(V, n, replace=False) for n in lengths]
    cnts = [rng.randint(1, 6, size=n) for n in lengths]
    z = rng.choice(V, 12, replace=False)
    ids.append(z)
    cnts.append(np.where(np.arange(12) % 2 == 0, 0, 3))
    r = rng.choice(V, 9, replace=False)
    r[[2, 5, 8]] = r[0]
    ids.append(r)
    cnts.append(rng.randint(1, 6, size=9))
    indptr = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.int32)
    return CSRDocuments(indptr, np.concatenate(ids).astype(np.int32),
                        np.concatenate(cnts).astype(np.int32))


def online_model(K, V, lam, D=20000, alpha=.1, eta=.3):
    """An OnlineLDA holding `lam` without paying for the constructor's K V 100 draws."""
    from trlda_amd.models import OnlineLDA
    m = OnlineLDA.__new__(OnlineLDA)
    m._num_documents = int(D)
    m._update_count = 0
    m._ada_tau = 1000.
    m._ada_rho = 1. / m._ada_tau
    m._ada_sq_norm = 1.
    m._setup(V, K, alpha, eta, None, _lambda=lam)
    return m


def batch_model(K, V, lam, alpha=.1, eta=.3):
    from trlda_amd.models import BatchLDA
    m = BatchLDA.__new__(BatchLDA)
    m._setup(V, K, alpha, eta, None, _lambda=lam)
    return m


def cumulative_model(K, V, alpha=.1, eta=.3):
    from trlda_amd.models import CumulativeLDA
    m = CumulativeLDA.__new__(CumulativeLDA)
    m._setup(V, K, alpha, eta, None, _lambda=np.full((K, V), float(eta), order="F"))
    m._psi_gamma_diff = np.zeros(K)
    m._num_documents = 0
    return m


def last_kernel(L, m):
    k = L.trlda_model_last_doc_kernel(m._handle)
    return k.decode() if isinstance(k, bytes) else k


# --------------------------------------------------------------------------------------------
# a. single E-steps against oracle.estep
# --------------------------------------------------------------------------------------------
def _estep_sweep(hip, oracle, sampler, K, V, T=None):
    from trlda_amd import _ffi
    docs = edge_docs(K, V, K, T or 256)
    B = len(docs)
    lam = random_lambda(K, V, K)
    g0 = seeded_gamma(sampler, K + 1, K, B)
    m = online_model(K, V, lam)
    if T:
        _ffi.check(hip.trlda_model_set_doc_threads(m._handle, T))
    batch = m.upload(docs)
    try:
        for max_iter in (0, 1, 100):
            go, so, ito = oracle.estep(lam, .1, docs.indptr, docs.ids, docs.cnts, g0, max_iter, 1e-3,
                                       nthreads=8)
            for mode in (_ffi.SSTATS_SEGMENTED, _ffi.SSTATS_ATOMIC):
                _ffi.check(hip.trlda_model_set_sstats_mode(m._handle, mode))
                g, s, it = m.update_variables(batch, latents=g0, max_iter=max_iter, return_iterations=True)
                where = (K, T, max_iter, mode)
                assert last_kernel(hip, m) == GEN, where
                assert relerr(g, go) < TIGHT_RTOL, (where, relerr(g, go))
                assert relerr(s, so) < TIGHT_RTOL, (where, relerr(s, so))
                assert np.array_equal(it, ito), where
    finally:
        batch.close()
        m.close()


@pytest.mark.parametrize("K", [513, 640, 1000, 1024, 1025, 2048, 2275, 2276, 2560, 2561, 4096, 5110,
                               5111, KMAX])
def test_estep_against_the_oracle(hip, oracle, sampler, k_max, K):
    """Both statistics modes, max_iter 0, 1 and until convergence, documents around n_cap."""
    K = k_max if K == KMAX else K
    _estep_sweep(hip, oracle, sampler, K, 400)


@pytest.mark.parametrize("K", [600, 1000])
@pytest.mark.parametrize("T", [64, 1024])
def test_estep_doc_threads(hip, oracle, sampler, K, T):
    """part[max(T, K)]: K above the workgroup (T = 64) and below it (T = 1024 > K)"""
    _estep_sweep(hip, oracle, sampler, K, 400, T)


def test_n_cap_formula():
    """the word caps the sweep is built around"""
    assert n_cap(513) == 36 and n_cap(2275) == 5
    assert n_cap(2276) == 5 and n_cap(5110) == 1 and n_cap(5111) == 0


# --------------------------------------------------------------------------------------------
# b. training trajectories: OnlineLDA, BatchLDA, CumulativeLDA
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,V", [(640, 1500), (2048, 600), (4096, 400), (2304, 2048)])
def test_training_against_the_oracle(hip, oracle, sampler, K, V):
    """(2304, 2048): K V >= 2^22 (the large-table path) with K > 2272 (the combined preamble)"""
    import trlda_amd
    D, B = 20000, 40
    lam0 = random_lambda(K, V, K + 7)
    docs = [corpus(B, V, seed=K + i) for i in range(3)]

    m = online_model(K, V, lam0, D)
    trlda_amd.seed(61)
    m.update_parameters(docs[0], max_iter_tr=3, max_iter_inference=20)
    m.update_parameters(docs[1], max_iter_tr=0, max_iter_inference=20)
    m.update_parameters(docs[2], max_iter_tr=2, max_iter_inference=20, init_gamma=False)
    assert last_kernel(hip, m) == GEN
    got = m.lambdas
    m.close()
    lam = lam0
    sampler.seed(61)
    for i, tr in enumerate((3, 0, 2)):
        rho = math.pow(100. + i, -.7)
        lam_prime = lam
        if tr > 0:
            lam = oracle.tr_init(lam_prime, docs[i].indptr, docs[i].ids, docs[i].cnts, D, rho, .3)
        g = None
        for _ in range(max(tr, 1)):
            if g is None or i == 2:                      # init_gamma=False on the third call
                g = sampler.sample_gamma(K, B, 100) / 100.
            g, s, _it = oracle.estep(lam, .1, docs[i].indptr, docs[i].ids, docs[i].cnts, g, 20, 1e-3,
                                     nthreads=8)
            lam = oracle.mstep_blend(lam_prime, s, rho, .3, float(D) / B)
    assert relerr(got, lam) < TIGHT_RTOL, ("online", relerr(got, lam))

    b = batch_model(K, V, lam0)
    trlda_amd.seed(63)
    b.update_parameters(docs[0], max_epochs=2, max_iter_inference=30)
    got = b.lambdas
    b.close()
    oracle.seed(63)
    _, want, _ = oracle.batch_update_parameters(lam0, .1, .3, docs[0].indptr, docs[0].ids, docs[0].cnts,
                                                max_epochs=2, max_iter_inference=30)
    assert relerr(got, want) < TIGHT_RTOL, ("batch", relerr(got, want))

    if K * V > 2000000:                                  # (the restatement's K V 100 draws per call)
        return
    c = cumulative_model(K, V)
    trlda_amd.seed(64)
    c.update_parameters(docs[0], max_epochs=2, max_iter_inference=30)
    c.update_parameters(docs[1], max_epochs=1, max_iter_inference=30)
    got = c.lambdas
    c.close()
    sampler.seed(64)
    lam = np.full((K, V), .3, order="F")
    for i, epochs in enumerate((2, 1)):                  # cumulativelda.cpp:57-71
        lam_prime = lam
        lam = sampler.sample_gamma(K, V, 100) / 100.
        for _ in range(epochs):
            g = sampler.sample_gamma(K, B, 100) / 100.
            _g, s, _it = oracle.estep(lam, .1, docs[i].indptr, docs[i].ids, docs[i].cnts, g, 30, 1e-3,
                                      nthreads=8)
            lam = lam_prime + s
    assert relerr(got, lam) < TIGHT_RTOL, ("cumulative", relerr(got, lam))


# --------------------------------------------------------------------------------------------
# c. empirical Bayes and the adaptive rate
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1000, 4096])
def test_eb_reductions_match_numpy(hip, K):
    """eb_gamma_kernel, eb_lambda_kernel and adaptive_kernel at large K (as the K = 200 test of
    test_gpu_update_loop.py)"""
    import trlda_amd
    from scipy import special as _special
    from trlda_amd import _ffi
    V, B, D = 500, 37, 5000
    lam0 = random_lambda(K, V, K + 12)
    m = online_model(K, V, lam0, D)
    docs = m.upload(corpus(B, V, seed=K + 22))
    hip.trlda_model_set_keep_sstats(m._handle, 1)
    trlda_amd.seed(9)
    gamma = np.empty((K, B), order="F")
    count, rho_out = C.c_int(0), C.c_double(0.)
    _ffi.check(hip.trlda_model_online_update(m._handle, docs.handle, D, .3, 2, 20, .7, 100., -1., 1, 1,
                                             0.001, C.byref(count), C.byref(rho_out), gamma.ctypes.data))
    want = (_special.digamma(gamma) - _special.digamma(gamma.sum(axis=0))[None, :]).sum(axis=1)
    assert relerr(m._psi_gamma_diff_device(B), want) < 1e-11
    lam = m.lambdas
    total, rowsums = m._lambda_psi_stats_device()
    assert relerr(rowsums, lam.sum(axis=1)) < 1e-13
    assert abs(total - _special.digamma(lam).sum()) < 1e-11 * abs(total)
    sstats = np.empty((K, V), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, sstats))
    upd = (.3 + D / float(B) * sstats) - lam0
    u2, g2 = C.c_double(0.), C.c_double(0.)
    _ffi.check(hip.trlda_model_adaptive_stats(m._handle, .3, D / float(B), 1000., C.byref(u2), C.byref(g2)))
    assert abs(u2.value - (upd * upd).sum()) < 1e-11 * u2.value
    grad = upd / 1000.
    assert abs(g2.value - (grad * grad).sum()) < 1e-11 * g2.value
    docs.close()
    m.close()


@pytest.mark.parametrize("K", [1000, 4096])
def test_eb_update_against_the_restatement(hip, oracle, sampler, K):
    """update_parameters(update_alpha, update_eta, adaptive): lambda from the oracle's pieces, then
    the host steps (onlinelda.cpp:123-175) on sums formed here with SciPy"""
    import trlda_amd
    from scipy import special as _special
    from trlda_amd.models import _online_alpha_step, _online_eta_step
    V, B, D = 500, 30, 20000
    lam0 = random_lambda(K, V, K + 3)
    docs = corpus(B, V, seed=K + 5)
    m = online_model(K, V, lam0, D)
    trlda_amd.seed(71)
    rho = m.update_parameters(docs, max_iter_tr=2, max_iter_inference=20, update_alpha=True,
                              update_eta=True, adaptive=True)
    got_lam, got_alpha, got_eta = m.lambdas, np.asarray(m.alpha, dtype=np.float64).ravel(), m.eta
    ada = (m._ada_sq_norm, m._ada_rho, m._ada_tau)
    m.close()
    assert rho == 1e-3                                   # the adaptive rate's first value (onlinelda.cpp:61)
    sampler.seed(71)
    g = sampler.sample_gamma(K, B, 100) / 100.
    lam = oracle.tr_init(lam0, docs.indptr, docs.ids, docs.cnts, D, rho, .3)
    for _ in range(2):
        g, s, _it = oracle.estep(lam, .1, docs.indptr, docs.ids, docs.cnts, g, 20, 1e-3, nthreads=8)
        lam = oracle.mstep_blend(lam0, s, rho, .3, float(D) / B)
    assert relerr(got_lam, lam) < TIGHT_RTOL
    pgd = (_special.digamma(g) - _special.digamma(g.sum(axis=0))[None, :]).sum(axis=1)
    alpha = _online_alpha_step(np.full(K, .1), pgd, B, rho, 1e-6)
    eta = _online_eta_step(.3, _special.digamma(lam).sum(), lam.sum(axis=1), K, V, rho, 1e-6)
    assert relerr(got_alpha, alpha) < TIGHT_RTOL
    assert abs(got_eta - eta) < TIGHT_RTOL * abs(eta)
    upd = (.3 + D / float(B) * s) - lam0
    u2 = (upd * upd).sum()
    g2 = ((upd / 1000.) ** 2).sum()
    sq = (1. - 1. / 1000.) + u2 / 1000.
    want = (sq, g2 / sq, 1000. * (1. - g2 / sq) + 1.)
    assert relerr(np.array(ada), np.array(want)) < 1e-9, (ada, want)


# --------------------------------------------------------------------------------------------
# d. the other readers of the E-step
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2276, 4096])
def test_lower_bound_term_by_term(hip, sampler, K):
    """factors 0, 1 and 3.7 against tests/elbo_host.py (as _check in test_gpu_lower_bound.py)"""
    from trlda_amd import _ffi
    tol = 1e-11
    V = 500
    docs = edge_docs(K, V, K + 9)
    B = len(docs)
    lam = random_lambda(K, V, K + 2)
    g0 = seeded_gamma(sampler, K + 4, K, B)
    m = online_model(K, V, lam)
    batch = m.upload(docs)
    out = {}
    for f in (0.0, 1.0, 3.7):
        gamma = np.array(g0, order="F", copy=True)
        res = C.c_double(np.nan)
        _ffi.check(hip.trlda_model_lower_bound(m._handle, batch.handle, gamma, m.eta, f, 100, 1e-3,
                                               C.byref(res)))
        assert last_kernel(hip, m) == GEN
        out[f] = (res.value, gamma)
    gamma, sstats = m.update_variables(batch, latents=g0, max_iter=100)
    batch.close()
    for f in out:
        assert np.array_equal(out[f][1], gamma), f
    t = elbo_host.terms(lam, np.full(K, .1), m.eta, docs.indptr, docs.ids, docs.cnts, gamma, sstats)
    m.close()
    b0, b1, b3 = out[0.0][0], out[1.0][0], out[3.7][0]
    assert abs(b0 - t["dense"]) <= tol * t["scale_dense"], (b0, t["dense"])
    slope = (b3 - b1) / 2.7
    want = elbo_host.batch_part(t)
    assert abs(slope - want) <= tol * t["scale_batch"] + 1e-14 * t["scale_dense"], (slope, want)
    assert abs(b1 - elbo_host.bound(t)) <= tol * elbo_host.scale(t)


@pytest.mark.parametrize("K", [2276, 4096])
def test_predictive_against_the_restatement(hip, sampler, K):
    from trlda_amd import _ffi
    V = 500
    observed = edge_docs(K, V, K + 11)
    B = len(observed)
    rng = np.random.RandomState(K)
    from trlda_amd.documents import CSRDocuments
    held_len = rng.poisson(20, size=B)
    held_len[1] = 0
    indptr = np.concatenate([[0], np.cumsum(held_len)]).astype(np.int32)
    heldout = CSRDocuments(indptr, rng.randint(0, V, size=indptr[-1]).astype(np.int32),
                           rng.randint(0, 4, size=indptr[-1]).astype(np.int32))
    lam = random_lambda(K, V, K + 6)
    g0 = seeded_gamma(sampler, K + 8, K, B)
    m = online_model(K, V, lam)
    ob, hb = m.upload(observed), m.upload(heldout)
    gamma = np.array(g0, order="F", copy=True)
    loglik, tokens = np.full(B, np.nan), np.full(B, np.nan)
    _ffi.check(hip.trlda_model_predictive(m._handle, ob.handle, hb.handle, gamma, 20, 1e-3, loglik, tokens))
    assert last_kernel(hip, m) == GEN
    ob.close()
    hb.close()
    g_ref, _ = m.update_variables(observed, latents=g0, max_iter=20)
    m.close()
    assert np.array_equal(gamma, g_ref)
    want_ll, want_tok = heldout_host.score(heldout.indptr, heldout.ids, heldout.cnts, gamma, lam)
    assert np.array_equal(tokens, want_tok)
    assert np.all(np.abs(loglik - want_ll) <= 1e-12 * np.abs(want_ll) + 1e-300), relerr(loglik, want_ll)


@pytest.mark.parametrize("K", [2276, 4096])
def test_stream_equals_plain_calls(hip, sampler, K):
    """EStepStream with deferred statistics and two lanes asked for: bitwise the plain E-steps"""
    import torch
    from trlda_amd.stream import EStepStream
    V, B = 500, 24
    lam = random_lambda(K, V, K + 13)
    csrs = [corpus(B, V, seed=K + 40 + i) for i in range(3)]
    g0s = [seeded_gamma(sampler, K + 50 + i, K, B) for i in range(3)]
    m = online_model(K, V, lam)
    dev = torch.device("cuda", 0)
    batches = [m.upload(c) for c in csrs]
    g0_t = [torch.from_numpy(np.ascontiguousarray(g.T)).to(dev) for g in g0s]
    gam = [torch.empty(B, K, dtype=torch.float64, device=dev) for _ in csrs]
    sst = [torch.full((V, K), float("nan"), dtype=torch.float64, device=dev) for _ in csrs]
    its = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in csrs]
    with EStepStream(m, lanes=2, deferred=True) as s:
        for i, b in enumerate(batches):
            s.step(b, batches[i + 1:i + 3], g0_t[i], gam[i], sst[i], max_iter=20, iterations=its[i])
    torch.cuda.synchronize()
    for i, c in enumerate(csrs):
        g, ss, it = m.update_variables(batches[i], latents=g0s[i], max_iter=20, return_iterations=True)
        assert np.array_equal(gam[i].cpu().numpy().T, g), i
        assert np.array_equal(sst[i].cpu().numpy().T, ss), i
        assert np.array_equal(its[i].cpu().numpy(), it), i
    for b in batches:
        b.close()
    m.close()


# --------------------------------------------------------------------------------------------
# e. the bound
# --------------------------------------------------------------------------------------------
def test_above_the_bound_every_vi_entry_point_fails_first(hip, k_max):
    """K = TRLDA_VI_MAX_TOPICS + 1: TRLDA_ERR_ARG naming the bound from every VI entry point, with
    lambda, alpha, eta, the update count and the seeded stream untouched; the readers that run no
    E-step still work"""
    import torch
    import trlda_amd
    from trlda_amd import _ffi
    from trlda_amd.stream import EStepStream, corpus_pass
    K, V, B = k_max + 1, 300, 6
    lam = random_lambda(K, V, 5)
    docs = corpus(B, V, seed=3, mean_unique=20)
    heldout = corpus(B, V, seed=4, mean_unique=10)
    m = online_model(K, V, lam, D=1000)
    m.update_count = 3
    bm = batch_model(K, V, lam)
    cm = cumulative_model(K, V)
    trlda_amd.seed(17)
    state0 = np.zeros(33, dtype=np.uint32)
    hip.trlda_rng_get_state(state0)
    dev = torch.device("cuda", 0)
    g_t = torch.ones(B, K, dtype=torch.float64, device=dev)
    s_t = [torch.zeros(V, K, dtype=torch.float64, device=dev) for _ in range(3)]
    batch = m.upload(docs)
    alpha0, eta0 = np.array(m.alpha, dtype=np.float64), m.eta

    def raw(rc):
        if rc != _ffi.OK:
            raise _ffi.TrldaError(rc, hip.trlda_last_error().decode())

    def stream_step():
        with EStepStream(m) as s:
            s.step(batch, [], g_t, g_t, s_t[0], max_iter=5)

    calls = {
        "update_variables": lambda: m.update_variables(docs, max_iter=5),
        "update_variables(latents)": lambda: m.update_variables(docs, latents=np.ones((K, B)), max_iter=5),
        "lower_bound": lambda: m.lower_bound(docs),
        "predictive_log_likelihood": lambda: m.predictive_log_likelihood(docs, heldout),
        "OnlineLDA.update_parameters": lambda: m.update_parameters(docs, max_iter_tr=2),
        "OnlineLDA.update_parameters(eb)": lambda: m.update_parameters(
            docs, update_alpha=True, update_eta=True, adaptive=True),
        "BatchLDA.update_parameters": lambda: bm.update_parameters(docs, max_epochs=1),
        "BatchLDA.update_parameters(eb)": lambda: bm.update_parameters(docs, max_epochs=1,
                                                                       update_alpha=True, update_eta=True),
        "CumulativeLDA.update_parameters": lambda: cm.update_parameters(docs, max_epochs=1),
        "EStepStream.step": stream_step,
        "corpus_pass": lambda: corpus_pass(m, docs.indptr.astype(np.int64), docs.ids, docs.cnts, B, g_t, g_t,
                                           s_t),
        "trlda_model_estep": lambda: raw(hip.trlda_model_estep(m._handle, batch.handle, None, None, 5, 1e-3,
                                                               None)),
        "trlda_model_estep_io": lambda: raw(hip.trlda_model_estep_io(m._handle, batch.handle, None, None, None,
                                                                     5, 1e-3, None)),
        "trlda_model_estep_io_next": lambda: raw(hip.trlda_model_estep_io_next(
            m._handle, batch.handle, None, None, None, None, 5, 1e-3, None)),
        "trlda_model_estep_resident": lambda: raw(hip.trlda_model_estep_resident(m._handle, batch.handle, 5,
                                                                                 1e-3)),
        "trlda_model_online_update": lambda: raw(hip.trlda_model_online_update(
            m._handle, batch.handle, 1000, .3, 2, 5, .7, 100., -1., 1, 1, 1e-3, None, None, None)),
        "trlda_estep": lambda: raw(hip.trlda_estep(
            K, V, B, docs.indptr, docs.ids, docs.cnts, lam, np.full(K, .1), np.ones((K, B), order="F"),
            np.zeros((K, V), order="F"), 5, 1e-3, None, 0)),
    }
    for name, call in calls.items():
        with pytest.raises(_ffi.TrldaError) as e:
            call()
        assert e.value.code == _ffi.ERR_ARG, (name, e.value.code, str(e.value))
        msg = str(e.value)
        assert "TRLDA_VI_MAX_TOPICS" in msg and str(k_max) in msg, (name, msg)
        state = np.zeros(33, dtype=np.uint32)
        hip.trlda_rng_get_state(state)
        assert np.array_equal(state, state0), name
    batch.close()
    assert np.array_equal(m.lambdas, lam) and np.array_equal(bm.lambdas, lam)
    assert np.array_equal(np.asarray(m.alpha, dtype=np.float64), alpha0) and m.eta == eta0
    assert np.array_equal(np.asarray(bm.alpha, dtype=np.float64), alpha0) and bm.eta == eta0
    assert m.update_count == 3
    assert np.array_equal(cm.lambdas, np.full((K, V), .3))

    # what runs no E-step still works at this K
    top = m.top_words(5)
    for k in (0, 1, K // 2, K - 1):
        assert np.array_equal(top[k], np.lexsort((np.arange(V), -lam[k]))[:5]), k
    sampled = m.sample(4, 20)
    assert len(sampled) == 4
    for d in sampled:
        assert all(0 <= w < V and c == 1 for w, c in d)
    for x in (m, bm, cm):
        x.close()


def test_bound_is_exported(hip, k_max):
    """header, library and binding agree; the check on its own"""
    import os
    import re
    from trlda_amd import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "trlda_hip.h")).read()
    assert int(re.search(r"#define TRLDA_VI_MAX_TOPICS (\d+)", header).group(1)) == k_max
    assert hip.trlda_vi_check_topics(k_max) == _ffi.OK
    assert hip.trlda_vi_check_topics(k_max + 1) == _ffi.ERR_ARG
    assert str(k_max) in hip.trlda_last_error().decode()
    assert n_cap(k_max) == 0 and (2 * k_max + k_max + 4) * 8 <= LDS_DYN_BYTES < (3 * (k_max + 1) + 4) * 8
