"""trlda_model_lower_bound (csrc/elbo_kernels.h, LDA::lowerBound of lda.cpp:297-360) against the
restatement of tests/elbo_host.py, term by term, on every variant of the E-step that runs in front
of it and in every model state that hands it a different origin of the row sums (psi_sum).

The bound reads what the E-step left behind: sstats, psi(row sums) at psi_sum[0, K) and the row sums
at psi_sum[K, 2K).  Called with factor 0 the result is the dense term alone (eta, lambda, the row
sums); the slope in the factor is the batch's part (sstats, the documents' terms).  Each is held to
1e-11 of the sum of the absolute values of its own addends, so a slip in the per-document terms is
not hidden by the large constant.  All in this process: no subprocesses."""
import ctypes as C

import numpy as np
import pytest

import elbo_host
import heldout_host

pytestmark = pytest.mark.gpu

TOL = 1e-11


@pytest.fixture(scope="module")
def L():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


def _lam(K, V, seed, lo=None, hi=None):
    rng = np.random.RandomState(seed)
    if lo is not None:
        lam = np.exp(rng.uniform(np.log(lo), np.log(hi), size=(K, V)))
    else:
        lam = rng.gamma(100., 1. / 100., size=(K, V)) * np.exp(rng.uniform(-1, 2, size=(K, 1)))
    return np.asfortranarray(lam)


def _model(K, V, lam, alpha=.1, eta=.3, D=1000):
    from trlda_amd.models import OnlineLDA
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=D, alpha=.1, eta=eta, device=0)
    m.lambdas = lam
    if not np.isscalar(alpha):
        m.alpha = np.asarray(alpha, dtype=np.float64)
    return m


def _alpha_vec(m):
    return np.asarray(m.alpha, dtype=np.float64).ravel()


def _docs(lengths, V, seed, zero_every=0):
    from trlda_amd.documents import CSRDocuments
    rng = np.random.RandomState(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ids = rng.randint(0, V, size=indptr[-1]).astype(np.int32)
    cnts = rng.randint(1, 6, size=indptr[-1]).astype(np.int32)
    if zero_every:
        cnts[::zero_every] = 0
    return CSRDocuments(indptr, ids, cnts)


def _g0(K, B, seed):
    return np.asfortranarray(np.random.RandomState(seed).gamma(100., 1. / 100., size=(K, B)))


def _bound(L, m, batch, g0, factor, max_iter=100, threshold=1e-3, eta=None):
    """(bound, converged gamma, the path the E-step took) through the C entry point"""
    from trlda_amd import _ffi
    gamma = np.array(g0, dtype=np.float64, order="F", copy=True)
    out = C.c_double(np.nan)
    _ffi.check(L.trlda_model_lower_bound(m._handle, batch.handle, gamma, m.eta if eta is None else eta,
                                         float(factor), int(max_iter), float(threshold), C.byref(out)))
    kern = L.trlda_model_last_doc_kernel(m._handle)
    path = dict(kernel=kern.decode() if isinstance(kern, bytes) else kern,
                fused=int(L.trlda_model_last_preamble_fused(m._handle)),
                split=int(L.trlda_model_last_split_workgroups(m._handle)),
                merged=int(L.trlda_model_last_merged(m._handle)))
    return out.value, gamma, path


def _check(L, m, docs, g0, max_iter=100, path=None, lam=None):
    """the bound at factors 0, 1 and 3.7 against the restatement's dense term and batch part; gamma
    of every call bitwise that of update_variables, whose sstats feed the restatement.  -> (terms,
    bound at factor 1, path of the last call)"""
    batch = m.upload(docs)
    b0, g_a, p0 = _bound(L, m, batch, g0, 0.0, max_iter)
    b1, g_b, p1 = _bound(L, m, batch, g0, 1.0, max_iter)
    b3, g_c, p3 = _bound(L, m, batch, g0, 3.7, max_iter)
    gamma, sstats = m.update_variables(batch, latents=g0, max_iter=max_iter)
    assert np.array_equal(gamma, g_a) and np.array_equal(gamma, g_b) and np.array_equal(gamma, g_c)
    assert p0 == p1 == p3, (p0, p1, p3)
    if path is not None:
        for k, v in path.items():
            if k == "kernel":
                assert p1["kernel"] == v, p1
            elif k == "split":
                assert (p1["split"] > 0) == v, p1
            else:
                assert p1[k] == v, p1
    lam = m.lambdas if lam is None else lam
    t = elbo_host.terms(lam, _alpha_vec(m), m.eta, docs.indptr, docs.ids, docs.cnts, gamma, sstats)
    assert abs(b0 - t["dense"]) <= TOL * t["scale_dense"], (b0, t["dense"], t["scale_dense"], p1)
    slope = (b3 - b1) / 2.7
    want = elbo_host.batch_part(t)
    assert abs(slope - want) <= TOL * t["scale_batch"] + 1e-14 * t["scale_dense"], (slope, want, t, p1)
    assert abs(b1 - elbo_host.bound(t)) <= TOL * elbo_host.scale(t)
    batch.close()
    return t, b1, p1


SMALL = "estep_docs_small_body"
REG = "estep_docs_reg_kernel"
TIER = "estep_docs_tiered_kernel"
WIDE = "estep_docs_wide_kernel"
GEN = "estep_docs_kernel"


# (K, V, lengths, the path: kernel, fused preamble, split workgroups)
PATHS = {
    "small-K2": (2, 300, [20] * 300, dict(kernel=SMALL, fused=1)),
    "small-K10": (10, 500, [30] * 280 + [5] * 20, dict(kernel=SMALL, fused=1)),
    "small-K32": (32, 800, [40] * 260, dict(kernel=SMALL, fused=1)),
    "small-K7-odd": (7, 400, [25] * 270, dict(kernel=SMALL, fused=1)),
    "reg-K1": (1, 200, [15] * 40, dict(kernel=REG, fused=1)),
    "reg-K7": (7, 300, [30] * 40, dict(kernel=REG, fused=1)),
    "reg-K33": (33, 600, [40] * 300, dict(kernel=REG, fused=1)),
    "reg-K64": (64, 1000, [60] * 50, dict(kernel=REG, fused=1)),
    "reg-K100": (100, 1500, [70] * 60, dict(kernel=REG, fused=1)),
    "reg-K128": (128, 2000, [128] * 30, dict(kernel=REG, fused=1)),
    "tiered-150": (64, 2000, [150] + [40] * 50, dict(kernel=TIER, fused=1, split=False)),
    "split-300-900": (64, 3000, [900, 300, 200] + [40] * 40, dict(kernel=TIER, fused=1, split=True)),
    "beyond-1024": (100, 4000, [1500, 400] + [50] * 30, dict(kernel=TIER, fused=1)),
    "wide-K129": (129, 700, [50] * 40, dict(kernel=WIDE, fused=0)),
    "wide-K200": (200, 900, [60] * 30, dict(kernel=WIDE, fused=0)),
    "wide-K512": (512, 600, [40] * 20, dict(kernel=WIDE, fused=0)),
    "general-K513": (513, 600, [40] * 20, dict(kernel=GEN, fused=0)),
    "general-K1000": (1000, 400, [30] * 12, dict(kernel=GEN, fused=0)),
    # K V above the dense kernel's grid (1024 x 256) with K not dividing it: the k += kstep wrap runs
    "dense-wrap-K100": (100, 7000, [60] * 40, dict(kernel=REG, fused=1)),
    "dense-wrap-K7": (7, 50000, [60] * 40, dict(kernel=REG, fused=1)),
}


@pytest.mark.parametrize("name", list(PATHS))
def test_every_e_step_path(L, name):
    K, V, lengths, path = PATHS[name]
    seed = sum(map(ord, name))
    m = _model(K, V, _lam(K, V, seed))
    docs = _docs(lengths, V, seed + 1)
    _check(L, m, docs, _g0(K, len(lengths), seed + 2), path=path)
    m.close()


def test_wave_per_document_when_asked_for(L):
    """TRLDA_DOCS_SMALL: the wave-per-document body at 40 documents, and the register kernel's
    result for the same inputs to rounding"""
    K, V, B = 16, 600, 40
    m = _model(K, V, _lam(K, V, 5))
    docs = _docs([35] * B, V, 6)
    g0 = _g0(K, B, 7)
    from trlda_amd import _ffi
    _ffi.check(L.trlda_model_set_doc_kernel(m._handle, 3))               # TRLDA_DOCS_SMALL
    t, b_small, _ = _check(L, m, docs, g0, path=dict(kernel=SMALL, fused=1))
    _ffi.check(L.trlda_model_set_doc_kernel(m._handle, 0))
    _t, b_reg, _ = _check(L, m, docs, g0, path=dict(kernel=REG, fused=1))
    assert abs(b_small - b_reg) <= 1e-13 * elbo_host.scale(t)
    m.close()


def test_two_kernel_preamble(L):
    """set_split_preamble(1): exp_elog_beta_kernel writes psi_sum, not the document launch"""
    K, V, B = 100, 1500, 60
    m = _model(K, V, _lam(K, V, 11))
    docs = _docs([70] * B, V, 12)
    g0 = _g0(K, B, 13)
    from trlda_amd import _ffi
    _t, b_fused, _ = _check(L, m, docs, g0, path=dict(fused=1))
    _ffi.check(L.trlda_model_set_split_preamble(m._handle, 1))
    t, b_split, _ = _check(L, m, docs, g0, path=dict(fused=0))
    _ffi.check(L.trlda_model_set_split_preamble(m._handle, 0))
    assert abs(b_fused - b_split) <= 1e-12 * elbo_host.scale(t)
    m.close()


@pytest.mark.parametrize("K,V,lengths,factor", [(64, 1000, [60] * 50, 20.0), (200, 900, [60] * 30, 1.0),
                                                (22, 100, [30] * 15, 2.0)])
def test_end_to_end_against_the_oracle(L, oracle, K, V, lengths, factor):
    """the oracle's E-step from the same gamma0, then its bound: equal iteration counts, the bound
    to 1e-9 relative"""
    m = _model(K, V, _lam(K, V, K))
    docs = _docs(lengths, V, K + 1)
    g0 = _g0(K, len(lengths), K + 2)
    batch = m.upload(docs)
    got, gamma, _ = _bound(L, m, batch, g0, factor)
    _g, _s, iters = m.update_variables(batch, latents=g0, max_iter=100, return_iterations=True)
    lam = m.lambdas
    go, so, ito = oracle.estep(lam, .1, docs.indptr, docs.ids, docs.cnts, g0, 100, 1e-3)
    assert np.array_equal(iters, ito)
    want = oracle.lower_bound(lam, .1, .3, docs.indptr, docs.ids, docs.cnts, go, so, factor)
    assert abs(got - want) < 1e-9 * abs(want), (got, want)
    batch.close()
    m.close()


# -- model states: each hands the bound a different origin of psi_sum --------------------------------
def _state_update(m, batch, K, V):
    """right after update_parameters on the same DeviceBatch: the row sums carried from the M-step"""
    import trlda_amd
    trlda_amd.seed(31)
    m.update_parameters(batch, max_iter_tr=2, max_iter_inference=20)


def _state_prefetched(m, batch, K, V):
    """an io_next call on another batch that announced this one: its preamble is prepared"""
    import torch
    from trlda_amd import _ffi
    L = _ffi.lib()
    other = m.upload(_docs([50] * 30, V, 77))
    g0 = torch.tensor(_g0(K, 30, 78).T.copy(), device="cuda:0")
    g = torch.empty_like(g0)
    s = torch.empty((V, K), dtype=torch.float64, device="cuda:0")
    _ffi.check(L.trlda_model_estep_io_next(m._handle, other.handle, batch.handle, g0.data_ptr(),
                                           g.data_ptr(), s.data_ptr(), 20, 1e-3, None))
    _ffi.check(L.trlda_model_synchronize(m._handle))
    other.close()


def _state_merged(m, batch, K, V):
    """set_merged_launch(2): the statistics ride on the document launch"""
    from trlda_amd import _ffi
    _ffi.check(_ffi.lib().trlda_model_set_merged_launch(m._handle, 2))


class _Stream(object):
    """inside an open EStepStream (deferred statistics on, two lanes) after a few steps"""

    def __call__(self, m, batch, K, V):
        import torch
        from trlda_amd.stream import EStepStream
        self.s = EStepStream(m)
        self.keep = []
        bs = [m.upload(_docs([50] * 40, V, 90 + i)) for i in range(4)]
        for i, b in enumerate(bs):
            g0 = torch.tensor(_g0(K, 40, 95 + i).T.copy(), device="cuda:0")
            g = torch.empty_like(g0)
            s = torch.empty((V, K), dtype=torch.float64, device="cuda:0")
            self.s.step(b, bs[i + 1:i + 3], g0, g, s, max_iter=20)
            self.keep += [g0, g, s]
        self.keep += bs

    def close(self):
        self.s.close()
        for x in self.keep:
            if hasattr(x, "close"):
                x.close()


STATES = ["update", "prefetched", "merged", "stream"]


def _in_state(state, K, V, lam, batch_docs):
    m = _model(K, V, lam)
    batch = m.upload(batch_docs)
    st = {"update": _state_update, "prefetched": _state_prefetched, "merged": _state_merged,
          "stream": _Stream()}[state]
    st(m, batch, K, V)
    return m, batch, st


def _fresh(m):
    f = _model(m.num_topics, m.num_words, m.lambdas, eta=m.eta)
    f.alpha = _alpha_vec(m)
    return f


def _same(a, b, state):
    if state == "update":
        assert np.array_equal(a == 0, b == 0)
        nz = b != 0
        assert np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz])) < 1e-12, state
    else:
        assert np.array_equal(a, b), (state, float(np.max(np.abs(a - b))))


@pytest.mark.parametrize("state", STATES)
def test_model_states(L, state):
    """In each state: the bound equals a fresh model's with the same lambda and alpha (1e-12
    relative) and the restatement's; do_e_step returns a fresh model's gamma and sstats bitwise;
    predictive_log_likelihood matches heldout_host.  Each of the three calls is the first call in
    its own copy of the state.  After an update the row sums are the ones the M-step carried, added
    up in another order than a fresh model's: there gamma and sstats agree to 1e-12, not bitwise."""
    from trlda_amd import _ffi
    from trlda_amd.utils import split_documents
    K, V, B = 64, 2000, 100
    lam = _lam(K, V, 41)
    docs = _docs([60] * B, V, 42)
    g0 = _g0(K, B, 43)
    # the bound
    m, batch, st = _in_state(state, K, V, lam, docs)
    got, gamma, path = _bound(L, m, batch, g0, 3.0)
    if state == "merged":
        assert path["merged"], path
    lam_now = m.lambdas
    f = _fresh(m)
    want, g_f, _ = _bound(L, f, f.upload(docs), g0, 3.0)
    _same(gamma, g_f, state)
    assert abs(got - want) <= 1e-12 * abs(want), (state, got, want, path)
    _gu, su = f.update_variables(docs, latents=g0, max_iter=100)
    t = elbo_host.terms(lam_now, _alpha_vec(f), f.eta, docs.indptr, docs.ids, docs.cnts, gamma, su)
    assert abs(got - elbo_host.bound(t, 3.0)) <= TOL * elbo_host.scale(t, 3.0)
    if hasattr(st, "close"):
        st.close()
    batch.close()
    m.close()
    # do_e_step
    m, batch, st = _in_state(state, K, V, lam, docs)
    g1, s1 = m.do_e_step(batch, latents=g0, max_iter=100)
    lam_now = m.lambdas
    f2 = _fresh(m)
    g2, s2 = f2.do_e_step(docs, latents=g0, max_iter=100)
    _same(g1, g2, state)
    _same(s1, s2, state)
    if hasattr(st, "close"):
        st.close()
    batch.close()
    m.close()
    # predictive_log_likelihood on the same documents' observed part
    import trlda_amd
    trlda_amd.seed(44)
    obs, held = split_documents(docs, 0.25)
    m, ob, st = _in_state(state, K, V, lam, obs)
    hb = m.upload(held)
    gp = np.array(_g0(K, B, 45), order="F")
    loglik = np.full(B, np.nan)
    tokens = np.full(B, np.nan)
    _ffi.check(L.trlda_model_predictive(m._handle, ob.handle, hb.handle, gp, 100, 1e-3, loglik, tokens))
    lam_now = m.lambdas
    hc = hb.csr
    w_ll, w_tok = heldout_host.score(hc.indptr, hc.ids, hc.cnts, gp, lam_now)
    assert np.array_equal(tokens, w_tok)
    assert np.max(np.abs(loglik - w_ll) / np.maximum(np.abs(w_ll), 1e-300)) < 1e-12, state
    if hasattr(st, "close"):
        st.close()
    ob.close()
    hb.close()
    m.close()
    f.close()
    f2.close()


def test_after_a_big_table_update(L, monkeypatch):
    """K = 384, V = 20000 (K V >= 2^22), after a trust-region update on the same batch.  Inside the
    update the M-step leaves exp(psi(lambda)) of the batch's words behind for the next iteration's
    E-step (fused_big: the wide kernel applies the topic factors, topic_factors_kernel writes
    psi_sum).  The LAST M-step of the call leaves nothing of the kind (emit_u is off there), so the
    bound's E-step cannot take that path: it runs exp_elog_beta_kernel on the carried row sums,
    asserted here, and its result equals a fresh model's (1e-12) and the restatement's."""
    import trlda_amd
    monkeypatch.setenv("TRLDA_BIG_EMIT", "1")
    K, V, B = 384, 20000, 64
    lam = _lam(K, V, 51)
    docs = _docs([60] * B, V, 52)
    g0 = _g0(K, B, 53)
    m = _model(K, V, lam, D=200000)
    batch = m.upload(docs)
    trlda_amd.seed(54)
    m.update_parameters(batch, max_iter_tr=3, max_iter_inference=20)
    assert L.trlda_model_last_preamble_fused(m._handle) == 1
    got, gamma, path = _bound(L, m, batch, g0, 2.0, max_iter=50)
    assert path["fused"] == 0 and path["kernel"] == WIDE, path
    lam_now = m.lambdas
    f = _fresh(m)
    fb = f.upload(docs)
    want, g_f, p_f = _bound(L, f, fb, g0, 2.0, max_iter=50)
    assert p_f == path, p_f
    _same(gamma, g_f, "update")
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    _g, s = f.update_variables(fb, latents=g0, max_iter=50)
    t = elbo_host.terms(lam_now, _alpha_vec(f), f.eta, docs.indptr, docs.ids, docs.cnts, gamma, s)
    assert abs(got - elbo_host.bound(t, 2.0)) <= TOL * elbo_host.scale(t, 2.0)
    for x in (batch, fb, m, f):
        x.close()


# -- edges ---------------------------------------------------------------------------------------------
def test_single_document(L):
    for K in (10, 100, 300):
        m = _model(K, 500, _lam(K, 500, K + 60))
        _check(L, m, _docs([40], 500, 61), _g0(K, 1, 62))
        m.close()


def test_empty_documents_zero_counts_and_repeated_ids(L):
    from trlda_amd.documents import CSRDocuments
    K, V = 20, 300
    rng = np.random.RandomState(63)
    lengths = np.array([0, 30, 0, 12, 50, 0, 1, 40, 0])
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ids = rng.randint(0, 8, size=indptr[-1]).astype(np.int32)           # few distinct words: repeats
    ids[-5:] = V - 1
    cnts = rng.randint(0, 4, size=indptr[-1]).astype(np.int32)           # zeros among them
    cnts[indptr[6]] = 0                                                  # a document of one zero entry
    docs = CSRDocuments(indptr, ids, cnts)
    for KK in (K, 200):
        m = _model(KK, V, _lam(KK, V, 64))
        _check(L, m, docs, _g0(KK, len(lengths), 65))
        m.close()


def test_non_uniform_alpha_wide_lambda_and_eta(L):
    K, V, B = 24, 400, 30
    alpha = np.linspace(.01, 3., K)
    docs = _docs(np.random.RandomState(66).randint(1, 80, size=B), V, 67)
    for eta in (1e-3, 10.):
        m = _model(K, V, _lam(K, V, 68, lo=1e-3, hi=1e4), alpha=alpha, eta=eta)
        assert np.array_equal(_alpha_vec(m), alpha)
        _check(L, m, docs, _g0(K, B, 69))
        m.close()


def test_same_seed_twice_and_permuted_documents(L):
    import trlda_amd
    from trlda_amd.documents import CSRDocuments
    K, V, B = 50, 1200, 80
    m = _model(K, V, _lam(K, V, 70))
    docs = _docs(np.random.RandomState(71).randint(5, 120, size=B), V, 72)
    trlda_amd.seed(73)
    a = m.lower_bound(docs, num_documents=5000)
    trlda_amd.seed(73)
    b = m.lower_bound(docs, num_documents=5000)
    assert a == b
    g0 = _g0(K, B, 74)
    t, b1, _ = _check(L, m, docs, g0)
    perm = np.random.RandomState(75).permutation(B)
    ip, ids, cn = [0], [], []
    for d in perm:
        s, e = docs.indptr[d], docs.indptr[d + 1]
        ids.append(docs.ids[s:e])
        cn.append(docs.cnts[s:e])
        ip.append(ip[-1] + e - s)
    pd = CSRDocuments(np.array(ip, np.int32), np.concatenate(ids), np.concatenate(cn))
    _t, b2, _ = _check(L, m, pd, np.asfortranarray(g0[:, perm]))
    assert abs(b1 - b2) <= 1e-13 * elbo_host.scale(t), (b1, b2)
    m.close()
