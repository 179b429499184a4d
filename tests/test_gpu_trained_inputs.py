"""The sampling and scoring entry points on what a trained model looks like (tests/trained_cases.py):
lambda = eta + sparse counts, most entries at eta <= 0.01 and a few at 1e3 .. 1e5, and a per-topic alpha
over three decades.  tests/test_trained_inputs_host.py proves on the restatements alone that these
inputs can fail a wrong kernel.

The table the samplers read, e = exp(psi(lambda) - psi(rowsum)), against a 50-digit golden table
(tests/golden/f16_trained_table.npz) in its three unvisited regimes -- tiny (~1e-49), subnormal
(~1e-316, through exp_nonpos's final ldexp) and exactly 0 (its clamp at -800) -- and every entry point
against its restatement under the bars its own file holds, with alpha swapped between two topics a
wrongly indexed kernel would confuse wherever alpha is read.

What it found: exp_elog_beta_kernel's subnormal entries were off by 4 - 5 units of 2^-1074 (1.5e-7
relative at 1e-316) where the bound allows one: csrc/psi.h formed s * ldexp(p, n), s = lambda + 10, so
the half unit of the ldexp's rounding onto the subnormal grid was multiplied by ten.  exp_nonpos now
multiplies s into p before the ldexp (the same bits wherever the result is normal).  The observed
maxima are in the docstrings of test_the_table and test_gibbs_chains.
"""
import ctypes as C

import numpy as np
import pytest

import cvb0_host
import gibbs_host
import gibbs_update_host as gu
import heldout_host
import l2r_host
import marginal_host
import sample_host
import trained_cases as tc
import wordtopics_host
from helpers import golden

pytestmark = pytest.mark.gpu

HISTOGRAM = "Something went wrong while sampling from histogram."


@pytest.fixture(scope="module")
def hip(hip_lib):
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return hip_lib


@pytest.fixture(scope="module")
def table_golden():
    return golden("f16_trained_table")


def _model(c, lam, alpha, cls=None):
    """An OnlineLDA (or `cls`) holding `lam` without the constructor's K V 100 draws."""
    from trlda_amd.models import OnlineLDA
    cls = cls or OnlineLDA
    m = cls.__new__(cls)
    if cls is OnlineLDA:
        m._num_documents = 1000
        m._update_count = 0
        m._ada_tau = 1000.
        m._ada_rho = 1. / m._ada_tau
        m._ada_sq_norm = 1.
    m._setup(c.V, c.K, alpha, c.eta, None, _lambda=np.asfortranarray(lam))
    return m


def _table(m):
    from trlda_amd import _ffi
    e = np.empty((m.num_topics, m.num_words), order="F")
    _ffi.check(_ffi.lib().trlda_debug_gibbs_table(m._handle, e))
    return e


def _key():
    from trlda_amd import _ffi
    key = C.c_uint64(0)
    _ffi.check(_ffi.lib().trlda_rng_draw_key(C.byref(key)))
    return key.value


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _table_name(c):
    return tc.case_id(c) + ("" if c.V == tc.V else "-V%d" % c.V)


# --------------------------------------------------------------------------------------------
# 1. the table
# --------------------------------------------------------------------------------------------
def check_table(e, c, lam, words, g):
    """The device's table at the columns `words` against the golden table.  Per entry

        |e - want| <= want (2e-15 max(1, |psi(lambda)|) + 5e-15 max(1, |psi(rowsum)|) + V 2^-53) + 2^-1074

    -- the bars tests/test_gpu_utils.py (test_device_digamma_table) holds for exp psi (2e-15 per unit
    of |psi|) and for psi (5e-15), the rounding of the row sum's V additions, and one more rounding
    onto the subnormal grid.  Entries the golden table has as 0 are 0, none is NaN or negative, and a
    golden entry above 4 * 2^-1074 is not 0.  Returns the worst error / bound."""
    name = _table_name(c)
    cols = g[name + "/cols"]
    at = np.searchsorted(cols, words)
    assert np.array_equal(cols[at], words)
    assert np.array_equal(g[name + "/lam"][:, at], lam[:, words])            # the same model, bitwise
    want = g[name + "/e"][:, at]
    psi_lam = np.abs(g[name + "/psi_lam"][:, at])
    psi_rs = np.abs(g[name + "/psi_rs"])[:, None]
    got = e[:, words]
    assert not np.isnan(got).any() and (got >= 0).all()
    assert np.all(got[want == 0] == 0)
    assert np.all(got[want > 4 * 2. ** -1074] > 0)
    bound = want * (2e-15 * np.maximum(1, psi_lam) + 5e-15 * np.maximum(1, psi_rs) + c.V * 2. ** -53) + 2. ** -1074
    ratio = np.abs(got - want) / bound
    worst = float(ratio.max())
    print("%s: %d x %d entries, worst error / bound %.3f (smallest non-zero %.3g, zeros %d)" %
          (name, got.shape[0], got.shape[1], worst, want[want > 0].min(), int((want == 0).sum())))
    assert worst <= 1.0, (name, worst, np.unravel_index(np.argmax(ratio), ratio.shape))
    return worst


@pytest.mark.parametrize("c", tc.table_cases(), ids=_table_name)
def test_the_table(hip, table_golden, c):
    """update_variables(inference_method='gibbs') (the preamble's block partials), and the table the
    update loops leave behind (trlda_model_online_update_gibbs with max_iter_tr = 0 and one epoch of
    trlda_model_batch_update_gibbs: their E-step reads the model's lambda as it is), against the
    golden table under check_table's bound.  Worst error / bound observed on the MI355X, the three
    tables alike: control 0.050, tiny 0.058, subnormal 0.047, zero 0.049 (its non-zero entries; every
    golden 0 is 0), V = 2000 0.031.  Before psi.h's exp_nonpos took its factor inside the ldexp the
    subnormal regime stood at 4.0 (K = 3) and 5.0 (K = 65, 200, 1000)."""
    import trlda_amd
    from trlda_amd.models import BatchLDA
    lam, alpha, _, _ = tc.build(c)
    docs = tc.table_docs(c)
    words = tc.words_of(docs)
    if c.eta != 1e-3:
        assert {c.V - 1, c.V - 2} <= set(words)
    trlda_amd.seed(7)
    m = _model(c, lam, alpha)
    try:
        m.update_variables(docs, inference_method="gibbs", num_samples=1, burn_in=0)
        check_table(_table(m), c, lam, words, table_golden)
        m.update_parameters(docs, max_iter_tr=0, inference_method="gibbs", num_samples=1, burn_in=0)
        check_table(_table(m), c, lam, words, table_golden)
    finally:
        m.close()
    b = _model(c, lam, alpha, cls=BatchLDA)
    try:
        b.update_parameters(docs, max_epochs=1, inference_method="gibbs", num_samples=1, burn_in=0)
        check_table(_table(b), c, lam, words, table_golden)
    finally:
        b.close()


# --------------------------------------------------------------------------------------------
# 2. Gibbs chains
# --------------------------------------------------------------------------------------------
def check_chain(m, alpha, docs, theta0, ns, bi, key, stats=None):
    """test_gpu_gibbs._check_chain with the alpha given: counts bitwise, theta to rounding."""
    from test_gpu_gibbs import _device_gibbs
    theta, sstats, e = _device_gibbs(m, docs, theta0, ns, bi, key)
    indptr, ids, cnts = tc.csr(docs)
    th_h, cnt_h, _ = gibbs_host.gibbs(e, alpha, indptr, ids, cnts, theta0, ns, bi, key, stats=stats)
    assert np.array_equal(sstats, cnt_h * (1.0 / ns))
    assert np.array_equal(np.rint(sstats * ns), cnt_h)
    assert np.allclose(theta, th_h, rtol=1e-12, atol=1e-300)
    return sstats


@pytest.mark.parametrize("c", tc.cases("gibbs"), ids=tc.case_id)
def test_gibbs_chains(hip, c):
    """_device_gibbs against gibbs_host.gibbs on the device's own table, with theta0 given and None,
    and with alpha swapped inside a lane and across lanes: device and restatement still agree, and
    the statistics are not those of the unswapped alpha.  At K = 3, eta = 1.4e-3 also the chain of
    trained_cases.FALLBACK_KEY over the documents with the unseen words, whose one-token document has
    a subnormal total of ~2e8 units: the restatement, on the device's table, counts a draw that ends in
    'last topic with p > 0' there.  Counted on the MI355X's tables: of the 31 752 draws of the sixteen
    cases' unswapped chains 4 526 pass an all-zero lane between a live lane and the chosen one and none
    picks a weight that is not > 0; the fall-back chain's 3 120 draws hold 1 'last topic with p > 0'
    (no lane with x_l > r), agreeing with the device bit for bit like the rest."""
    lam, alpha, docs, unseen = tc.build(c)
    th0 = tc.theta0(c.K, len(docs), c.seed)
    key = tc.key_of(c)
    stats = {}
    m = _model(c, lam, alpha)
    try:
        base = check_chain(m, alpha, docs, th0, tc.NS, tc.BI, key, stats)
        check_chain(m, alpha, docs, None, tc.NS, tc.BI, key + 1, stats)
        if c.K == tc.FALLBACK_K and c.eta == tc.FALLBACK_ETA:
            one = {}
            check_chain(m, alpha, unseen, th0, tc.FALLBACK_NS, tc.FALLBACK_BI, tc.FALLBACK_KEY, one)
            print("%s, the fall-back chain: %r" % (tc.case_id(c), one))
            assert one.get("last_overall", 0) >= 1
    finally:
        m.close()
    print("%s: %r" % (tc.case_id(c), stats))
    assert stats.get("zero_weight_pick", 0) == 0
    if c.eta == 1e-3 and c.K > 64:
        assert stats.get("zero_lane_below", 0) >= 1
    assert len(c.pairs) == len(tc.pair_patterns("gibbs", c.K))
    for pair in c.pairs:
        a2 = tc.swapped(alpha, pair)
        m = _model(c, lam, a2)
        try:
            other = check_chain(m, a2, docs, th0, tc.NS, tc.BI, key)
        finally:
            m.close()
        assert not np.array_equal(other, base), pair


def test_gibbs_failure_leaves_no_trace(hip):
    """An unseen word at eta = 1e-3: every topic's table entry is 0, the token's histogram has total 0
    and the call raises the reference's message; the caller's statistics are not written, and the
    model's next call on a good batch matches the restatement (no stale flag, no stale counts)."""
    from trlda_amd import _ffi
    c = next(x for x in tc.cases("gibbs") if x.K == 65 and x.eta == 1e-3)
    lam, alpha, docs, unseen = tc.build(c)
    th0 = tc.theta0(c.K, len(docs), c.seed)
    m = _model(c, lam, alpha)
    try:
        for latents in (None, th0):
            with pytest.raises(RuntimeError, match=HISTOGRAM):
                m.update_variables(unseen, latents=latents, inference_method="gibbs")
        batch = m.upload(unseen)
        try:
            theta = np.array(th0, order="F")
            sstats = np.full((c.K, c.V), -7., order="F")
            rc = hip.trlda_model_gibbs_host(m._handle, batch.handle, theta, 1, sstats, 1, 2)
            assert rc == _ffi.ERR_VALUE and hip.trlda_last_error().decode() == HISTOGRAM
            assert np.all(sstats == -7.) and np.array_equal(theta, th0)
        finally:
            batch.close()
        check_chain(m, alpha, docs, th0, tc.NS, tc.BI, tc.key_of(c))
        check_chain(m, alpha, docs, None, 2, 0, tc.key_of(c) + 5)
    finally:
        m.close()


# --------------------------------------------------------------------------------------------
# 3. the Gibbs update loops
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in tc.cases("gibbs") if c.K > 64], ids=tc.case_id)
def test_gibbs_update_loops(hip, oracle, c):
    """tests/test_gpu_gibbs_update.py's comparison (lambda to 1e-12, the statistics bitwise where they
    are kept) with the trained lambda, its eta and the per-topic alpha, at one K per KPL >= 2: online
    with max_iter_tr 0, 1 (adaptive: a given rho) and 3, batch with 1 and 2 epochs."""
    import trlda
    from test_gpu_gibbs_update import _close, _keys, _sstats
    from trlda_amd.models import BatchLDA
    lam0, alpha, docs, _ = tc.build(c)
    D = 1000
    for T in (0, 1, 3):
        seed = 1000 + c.K + T
        m = _model(c, lam0, alpha)
        try:
            keys = _keys(seed, max(T, 1))
            trlda.seed(seed)
            rho = m.update_parameters(docs, max_iter_tr=T, inference_method="gibbs", num_samples=tc.NS,
                                      burn_in=tc.BI, adaptive=(T == 1), rho=(0.4 if T == 1 else -1.))
            want_rho = 0.4 if T == 1 else gu.online_rho(0, .7, 100.)
            assert rho == want_rho
            lam, sstats, _, _, _ = gu.online(lam0, alpha, c.eta, docs, D, want_rho, T, True, tc.NS, tc.BI,
                                             keys, oracle.digamma, last_table=_table(m))
            assert _close(m.lambdas, lam), (T, _rel(np.asarray(m.lambdas), lam))
            if T == 1:
                assert np.array_equal(_sstats(m), sstats)
        finally:
            m.close()
    for epochs in (1, 2):
        seed = 2000 + c.K + epochs
        m = _model(c, lam0, alpha, cls=BatchLDA)
        try:
            keys = _keys(seed, epochs)
            trlda.seed(seed)
            m.update_parameters(docs, max_epochs=epochs, inference_method="gibbs", num_samples=tc.NS,
                                burn_in=tc.BI)
            lam, _, _, _, _ = gu.batch(lam0, alpha, c.eta, docs, epochs, tc.NS, tc.BI, keys, oracle.digamma,
                                       last_table=_table(m))
            assert _close(m.lambdas, lam), (epochs, _rel(np.asarray(m.lambdas), lam))
        finally:
            m.close()


def test_gibbs_update_adaptive_rate_and_eta(hip, oracle):
    """test_gpu_gibbs_update.test_adaptive_rate_and_eta from the trained lambda (K = 65, eta = 0.01, the
    per-topic alpha): three online Gibbs updates with adaptive=True, update_eta=True match the
    restatement's rho sequence and eta to 1e-12, and lambda to 1e-12."""
    import trlda
    from test_gpu_gibbs_update import _close, _keys
    c = next(x for x in tc.cases("gibbs") if x.K == 65 and x.eta == 0.01)
    lam0, alpha, docs, _ = tc.build(c)
    T, D = 2, 1000
    batches = [docs, tc.l2r_docs(docs), docs[::-1]]
    m = _model(c, lam0, alpha)
    try:
        keys = _keys(77, len(batches) * T)
        trlda.seed(77)
        rhos, etas = [], []
        for b in batches:
            rhos.append(m.update_parameters(b, max_iter_tr=T, inference_method="gibbs", adaptive=True,
                                            update_eta=True))
            etas.append(m.eta)
        lam_dev = np.array(m.lambdas)
    finally:
        m.close()
    ada = gu.Adaptive((c.K, c.V))
    lam, eta = lam0, c.eta
    for i, b in enumerate(batches):
        rho = ada.rho
        assert abs(rhos[i] - rho) <= 1e-12 * rho, (i, rhos[i], rho)
        new, sstats, _, _, _ = gu.online(lam, alpha, eta, b, D, rho, T, True, 1, 2, keys[i * T:(i + 1) * T],
                                         oracle.digamma)
        eta_new = gu.eta_step(new, eta, rho, oracle.digamma)
        ada.step(eta + float(D) / len(b) * sstats, lam)
        lam, eta = new, eta_new
        assert abs(etas[i] - eta) <= 1e-12 * eta, (i, etas[i], eta)
    assert len(set(rhos)) == len(batches)
    assert _close(lam_dev, lam)


# --------------------------------------------------------------------------------------------
# 4. CVB0
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", tc.cases("cvb0"), ids=tc.case_id)
def test_cvb0(hip, c):
    """tests/test_gpu_cvb0.py's comparison -- iterations, theta and statistics bit for bit against
    cvb0_host.cvb0 on the device's table -- without and with latents, and with alpha swapped."""
    from test_gpu_cvb0 import no_near_tie
    lam, alpha, docs, _ = tc.build(c)
    indptr, ids, cnts = tc.csr(docs)
    lat = tc.theta0(c.K, len(docs), c.seed)
    runs = [(tc.CVB0_ITER, tc.CVB0_THRESHOLD, None), (100, 0.001, None), (tc.CVB0_ITER, tc.CVB0_THRESHOLD, lat)]

    def run(a):
        m = _model(c, lam, a)
        out = []
        try:
            for max_iter, threshold, latents in runs:
                theta, sstats, iters = m.update_variables(docs, latents=latents, inference_method="cvb0",
                                                          max_iter=max_iter, threshold=threshold,
                                                          return_iterations=True)
                th, ss, it, deltas = cvb0_host.cvb0(_table(m), a, indptr, ids, cnts, latents, max_iter, threshold)
                assert no_near_tie(deltas, it, max_iter, threshold), deltas
                assert np.array_equal(iters, it), (iters, it)
                assert np.array_equal(theta, th) and np.array_equal(sstats, ss)
                out.append(theta)
        finally:
            m.close()
        return out

    base = run(alpha)
    assert len(c.pairs) == len(tc.pair_patterns("cvb0", c.K))
    for pair in c.pairs:
        other = run(tc.swapped(alpha, pair))
        assert not np.array_equal(other[0], base[0]), pair


# --------------------------------------------------------------------------------------------
# 5. LDA.sample
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", tc.cases("sample"), ids=tc.case_id)
def test_sample(hip, c):
    """tests/test_gpu_sample.py's comparisons with the trained lambda: a Dirichlet(lambda_k) with
    lambda = 1e-3 gives many beta exactly 0 and prefix sums with long flat runs.  Tokens bitwise given
    the device's theta and table, theta and the table to that file's _close, and every drawn word has
    a beta > 0 in the restatement's table."""
    from test_gpu_sample import _close, _device_sample
    lam, alpha, _, _ = tc.build(c)
    B, length = 40, 30
    key = 0x2545F4914F6CDD1D ^ tc.key_of(c)
    m = _model(c, lam, alpha)
    try:
        indptr, ids, theta, table = _device_sample(m, B, length, key)
    finally:
        m.close()
    assert np.array_equal(indptr, sample_host.lengths(B, length, key))
    assert (ids >= 0).all() and (ids < c.V).all()
    w, z = sample_host.tokens(indptr, theta, table, key)
    assert np.array_equal(ids, w)
    want = sample_host.beta_table(lam, key)
    assert _close(table, want)
    assert _close(theta, sample_host.theta(alpha, B, key))
    beta = np.diff(np.concatenate((np.zeros((c.K, 1)), want), axis=1), axis=1)
    assert len(w) > B and np.all(beta[z, w] > 0)
    print("%s: %d tokens; beta exactly 0 in %.1f%% of the restatement's table" %
          (tc.case_id(c), len(w), 100. * (beta == 0).mean()))


# --------------------------------------------------------------------------------------------
# 6. left_to_right
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", tc.cases("l2r"), ids=tc.case_id)
def test_left_to_right(hip, c):
    """tests/test_gpu_l2r.py's parity (1e-12 relative, token counts exact) under the same key, both
    `resample` values and both combinations, and with alpha swapped.  The long document is cut to that
    file's 131 tokens (trained_cases.l2r_docs: the restatement redraws the whole prefix per position).
    Observed maximum: 1.6e-15."""
    import trlda_amd
    from test_gpu_l2r import PARITY_RTOL
    lam, alpha, docs, _ = tc.build(c)
    docs = tc.l2r_docs(docs)
    indptr, ids, cnts = tc.csr(docs)
    R = tc.L2R_PARTICLES
    tokens_want = np.array([float(sum(n for _, n in d)) for d in docs])
    assert tokens_want[3] == tc.L2R_LONG

    def run(a, resamples):
        m = _model(c, lam, a)
        batch = m.upload(docs)
        out, worst = [], 0.
        try:
            for resample in resamples:
                trlda_amd.seed(100 + c.K)
                key = _key()
                want, want_tokens = l2r_host.left_to_right(indptr, ids, cnts, lam, a, key, R, resample)
                for combine in ("particle", "position"):
                    trlda_amd.seed(100 + c.K)
                    ll, tokens = m.left_to_right(batch, num_particles=R, resample=resample, combine=combine,
                                                 return_tokens=True)
                    assert np.array_equal(tokens, want_tokens) and np.array_equal(tokens, tokens_want)
                    full = tokens > 0
                    assert np.all(ll[~full] == 0.0) and np.all(np.isfinite(ll)) and np.all(ll[full] < 0)
                    err = _rel(ll[full], want[combine][full])
                    worst = max(worst, err)
                    assert err < PARITY_RTOL, (resample, combine, err)
                    out.append(ll)
        finally:
            batch.close()
            m.close()
        return out, worst

    base, worst = run(alpha, (True, False))
    print("%s: max rel err loglik %.3e" % (tc.case_id(c), worst))
    assert len(c.pairs) == len(tc.pair_patterns("l2r", c.K))
    for pair in c.pairs:
        other, _ = run(tc.swapped(alpha, pair), (False,))
        assert _rel(other[0], base[2]) > 1e-9, pair


# --------------------------------------------------------------------------------------------
# 7. document_log_likelihood
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", tc.cases("marginal"), ids=tc.case_id)
def test_document_log_likelihood(hip, c):
    """tests/test_gpu_marginal.py's parity under the same key for both proposals (loglik 1e-12, ess
    1e-9 relative; documents without tokens 1e-12 absolute), and with alpha swapped.  Observed maxima:
    loglik 2.0e-13, ess 7.3e-13."""
    import trlda_amd
    from trlda_amd import _ffi
    from test_gpu_marginal import PARITY_RTOL
    lam, alpha, docs, _ = tc.build(c)
    indptr, ids, cnts = tc.csr(docs)
    B, S = len(docs), tc.MARGINAL_SAMPLES
    tok = np.array([sum(n for _, n in d) > 0 for d in docs])

    def run(a):
        m = _model(c, lam, a)
        batch = m.upload(docs)
        out = {}
        try:
            for proposal in ("vi", "prior"):
                trlda_amd.seed(100 + c.K)
                g0 = None
                if proposal == "vi":
                    g0 = np.empty((c.K, B), order="F")
                    _ffi.lib().trlda_sample_gamma_init(c.K, B, g0)
                key = _key()
                trlda_amd.seed(100 + c.K)
                ll, ess = m.document_log_likelihood(batch, num_samples=S, proposal=proposal, return_ess=True)
                gamma = m.update_variables(batch, latents=g0)[0] if proposal == "vi" else None
                want_ll, want_ess = marginal_host.document_loglik(indptr, ids, cnts, lam, a, key, S, gamma=gamma)
                assert np.all(np.isfinite(ll)) and ll.shape == (B,)
                assert np.all(np.abs(ll[~tok]) < 1e-12) and np.all(np.abs(want_ll[~tok]) < 1e-12)
                e_ll, e_ess = _rel(ll[tok], want_ll[tok]), _rel(ess, want_ess)
                print("%s %s: max rel err loglik %.3e ess %.3e" % (tc.case_id(c), proposal, e_ll, e_ess))
                assert e_ll < 1e-12 and e_ess < PARITY_RTOL, (proposal, e_ll, e_ess)
                assert np.all(ess >= 1.0) and np.all(ess <= S)
                out[proposal] = ll
        finally:
            batch.close()
            m.close()
        return out

    base = run(alpha)
    assert len(c.pairs) == len(tc.pair_patterns("marginal", c.K))
    for pair in c.pairs:
        other = run(tc.swapped(alpha, pair))
        for proposal in base:
            assert _rel(other[proposal][tok], base[proposal][tok]) > 1e-9, (pair, proposal)


# --------------------------------------------------------------------------------------------
# 8. predictive_log_likelihood
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", tc.cases("heldout"), ids=tc.case_id)
def test_predictive_log_likelihood(hip, c):
    """tests/test_gpu_heldout.py's comparison (tokens exact, loglik to its _close) from the gamma the
    call returns; the held-out documents hold the unseen words, whose beta is eta / rowsum in every
    topic.  With alpha swapped (read by the E-step behind it) the same, and another value."""
    from test_gpu_heldout import _close, _device_predictive
    lam, alpha, docs, unseen = tc.build(c)
    h_indptr, h_ids, h_cnts = tc.csr(unseen)
    g0 = np.asfortranarray(np.random.RandomState(c.K).gamma(1., 1., (c.K, len(docs))) + .1)

    def run(a):
        m = _model(c, lam, a)
        try:
            gamma, loglik, tokens = _device_predictive(m, docs, unseen, g0)
            g_ref, _ = m.update_variables(docs, latents=g0, max_iter=20, threshold=1e-3)
        finally:
            m.close()
        assert np.array_equal(gamma, np.asarray(g_ref))
        want_ll, want_tok = heldout_host.score(h_indptr, h_ids, h_cnts, gamma, lam)
        assert np.array_equal(tokens, want_tok)
        assert _close(loglik, want_ll), _rel(loglik, want_ll)
        assert loglik[1] == 0 and tokens[1] == 0
        return loglik

    base = run(alpha)
    assert len(c.pairs) == len(tc.pair_patterns("heldout", c.K))
    for pair in c.pairs:
        assert _rel(run(tc.swapped(alpha, pair)), base) > 1e-9, pair


# --------------------------------------------------------------------------------------------
# 9. word_topics
# --------------------------------------------------------------------------------------------
def wordtopics_floor(indptr, ids, gamma, lam):
    """Per entry what the subnormal grid does to a probability: s_pk = exp(psi(gamma_dk) - psi(rs_k))
    exp(psi(lambda_kw)) is a product rounded onto multiples of 2^-1074 once it is below 2^-1022 -- half
    a unit on the device, half a unit in the restatement, and a unit each where their factors differ
    in the last place and the product falls on either side of a grid point -- so phi = s / sum_j s_pj
    carries up to 4 * 2^-1074 / sum_j s_pj of ABSOLUTE error beside the file's 1e-9 relative."""
    from scipy.special import psi
    doc = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    with np.errstate(under="ignore"):
        fac = np.exp(psi(gamma) - psi(lam.sum(axis=1))[:, None])
        s = fac[:, doc].T * np.exp(psi(lam[:, ids])).T
    return 4 * 2. ** -1074 / s.sum(axis=1)


@pytest.mark.parametrize("c", tc.cases("wordtopics"), ids=tc.case_id)
def test_word_topics(hip, c):
    """tests/test_gpu_wordtopics.py's parity from the gamma the call returns, with the per-topic alpha:
    probs to 1e-9 relative plus wordtopics_floor's absolute term (the file's bar is wrong on paper for
    a probability that is a handful of subnormal units over a normal sum: see there), topics exactly
    in every row without a near tie.  A row is free of near ties when each of its top_n ranked
    probabilities is above the next by more than GAP_FLOOR relative and twice the floor, or both are
    exactly 0 (equal values go by the smaller topic id, in the restatement as on the device); a row
    that is not keeps the bar on its probabilities, compared in rank order.  At eta = 0.3 and 0.01 no
    row has a near tie, at every eta every row's first topic is clear.  Observed: no row of any case has
    a near tie; the largest relative error beyond the floor is 1.4e-13 (K = 3).  With alpha swapped (read
    by the E-step behind it) the same, and other leading probabilities."""
    from test_gpu_wordtopics import GAP_FLOOR
    lam, alpha, docs, _ = tc.build(c)
    indptr, ids, cnts = tc.csr(docs)
    g0 = np.asfortranarray(np.random.RandomState(c.K).gamma(1., 1., (c.K, len(docs))) + .1)
    top_n = min(3, c.K)

    def run(a):
        m = _model(c, lam, a)
        try:
            ip, topics, probs, gamma = m.word_topics(docs, top_n=top_n, latents=g0, max_iter=20,
                                                     return_gamma=True)
        finally:
            m.close()
        assert np.array_equal(ip, indptr) and topics.shape == probs.shape == (len(ids), top_n)
        with np.errstate(under="ignore", invalid="ignore"):
            phi, want_t, want_p, _ = wordtopics_host.word_topics(indptr, ids, gamma, lam, top_n)
        floor = wordtopics_floor(indptr, ids, gamma, lam)[:, None]
        ranked = -np.sort(-phi, axis=1)[:, :top_n + 1]
        upper, lower = ranked[:, :-1], ranked[:, 1:]
        clear = (upper - lower > GAP_FLOOR * upper + 2 * floor) | ((upper == 0) & (lower == 0))
        rows = clear.all(axis=1)
        assert clear[:, 0].all()
        if c.eta >= 0.01:
            assert rows.all()
        assert np.array_equal(topics[rows], want_t[rows])
        assert np.array_equal(topics[:, 0], want_t[:, 0])
        excess = np.abs(probs - want_p) - floor
        err = float(np.max(excess / np.maximum(want_p, 1e-300)))
        assert np.all(excess <= 1e-9 * want_p), err
        return probs, err, rows

    base, err, rows = run(alpha)
    print("%s: max rel err of probs beyond the floor %.2e; rows without a near tie %d of %d" %
          (tc.case_id(c), err, int(rows.sum()), len(rows)))
    assert len(c.pairs) == len(tc.pair_patterns("wordtopics", c.K))
    for pair in c.pairs:
        other, _, _ = run(tc.swapped(alpha, pair))
        assert _rel(other[:, 0], base[:, 0]) > 1e-9, pair
