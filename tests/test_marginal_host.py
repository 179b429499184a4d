"""The documents' marginal likelihood on the CPU: the NumPy restatement of csrc/marginal_kernels.h
(tests/marginal_host.py) against the exact value by enumeration, the enumerator against a closed
form, the restatement's building blocks, and what LDA.document_log_likelihood refuses before it
touches a device."""
import math

import numpy as np
import pytest

import marginal_host as mh

K, V = 3, 4
LAM = np.array([[5., 1., 2., .5], [1., 4., 1., 3.], [2., 2., 6., 1.]])
ALPHA = np.array([0.5, 0.2, 1.0])
DOC = [(0, 2), (1, 1), (2, 2), (3, 1)]          # the model and document of test_gpu_gibbs.py, test_exact_posterior
WORDS = [0, 0, 1, 2, 2, 3]
T_BOUND = 9.0                                   # that test's bound: above t_19's two-sided 1e-6 / 15 quantile (8.51)


def _csr(docs):
    indptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int32)
    ids = np.array([w for d in docs for w, _ in d], dtype=np.int32)
    cnts = np.array([c for d in docs for _, c in d], dtype=np.int32)
    return indptr, ids, cnts


def ratios(proposal, oracle, S=1000, n=20):
    beta = LAM / LAM.sum(axis=1)[:, None]
    exact = mh.exact_log_marginal(beta, ALPHA, WORDS)
    indptr, ids, cnts = _csr([DOC])
    gamma = None
    if proposal == "vi":                         # the fixed-lambda E-step's gamma, from gamma0 = 1
        gamma, _, _ = oracle.estep(LAM, ALPHA, indptr, ids, cnts, np.ones((K, 1)), 100, 1e-3)
    est = [mh.document_loglik(indptr, ids, cnts, LAM, ALPHA, 0x9E3779B97F4A7C15 * (j + 1) % 2 ** 63, S,
                              gamma=gamma)[0][0] for j in range(n)]
    return np.exp(np.array(est) - exact)


@pytest.mark.parametrize("proposal", ["vi", "prior"])
def test_restatement_is_unbiased_for_the_enumerated_marginal(oracle, proposal):
    """20 independently keyed estimates R_j = exp(est_j - exact), S = 1000 samples each, of the
    6-token document: their mean is within t SE of 1, SE the spread over the 20 (a t distribution
    with 19 degrees of freedom), t = 9.0 -- the bound test_exact_posterior derives for 15
    quantities at 1e-6; here there are 2, one per proposal.  Observed |mean - 1| / SE: 'prior' 1.18
    (mean 0.9983, SE 1.44e-3), 'vi' 2.76 (mean 0.9220, SE 2.83e-2).

    Why 'vi' is the wider one here: gamma = (2.01, 0.21, 5.48) against alpha = (0.5, 0.2, 1.0).  Near
    theta_k = 0 the weight grows like theta_k^(alpha_k - gamma_k) while the likelihood of so short a
    document stays positive there (the other topics explain its words), so E_q[w^2] ~ integral of
    theta_k^(2 alpha_k - gamma_k - 1) diverges where gamma_k >= 2 alpha_k (topics 0 and 2): the
    estimate is unbiased with a heavy right tail, and finite runs sit below 1.  Long documents with
    separated topics push that tail's mass towards nothing; ess is what tells."""
    R = ratios(proposal, oracle)
    se = R.std(ddof=1) / math.sqrt(len(R))
    print("%s: mean %.6f SE %.3e |mean - 1| / SE %.3f" % (proposal, R.mean(), se, abs(R.mean() - 1) / se))
    assert se > 0 and abs(R.mean() - 1.0) <= T_BOUND * se


def test_enumerator_one_token_closed_form():
    """N = 1: p(w) = sum_k (alpha_k / sum alpha) beta_kw."""
    rng = np.random.RandomState(3)
    for k in (1, 2, 5):
        beta = rng.dirichlet(np.ones(7), size=k)
        alpha = rng.gamma(1., 1., k) + .05
        for w in (0, 3, 6):
            want = math.log(float((alpha / alpha.sum()) @ beta[:, w]))
            assert abs(mh.exact_log_marginal(beta, alpha, [w]) - want) < 1e-13
    assert mh.exact_log_marginal(np.ones((2, 2)) / 2, np.ones(2), []) == 0.0


def test_enumerator_one_topic_is_the_product():
    """K = 1: theta = 1, p(w) = prod_i beta_{0, w_i}."""
    beta = np.array([[.1, .2, .3, .4]])
    words = [0, 3, 3, 1, 2]
    want = sum(math.log(beta[0, w]) for w in words)
    assert abs(mh.exact_log_marginal(beta, np.array([.7]), words) - want) < 1e-13


def test_wave_sum_tree():
    """wave_sum_dpp's tree: exact on integers, and the stated grouping on values that expose it."""
    rng = np.random.RandomState(0)
    v = rng.randint(-1000, 1000, size=(5, 64)).astype(np.float64)
    assert np.array_equal(mh.wave_sum_dpp(v), v.sum(axis=1))
    x = rng.standard_normal(64) * 10.0 ** rng.randint(-8, 8, 64)
    def row(r):                                  # lane 15 of a row after shifts by 1, 2, 4, 8
        p = [r[i] + r[i - 1] for i in range(1, 16, 2)]                 # (x1+x0), (x3+x2), ..
        q = [p[i] + p[i - 1] for i in range(1, 8, 2)]
        h = [q[i] + q[i - 1] for i in range(1, 4, 2)]
        return h[1] + h[0]
    r = [row(x[16 * i:16 * i + 16]) for i in range(4)]
    assert mh.wave_sum_dpp(x) == (r[3] + r[2]) + (r[1] + r[0])
    assert mh.lane_sum(np.arange(130.0)[None, :])[0] == 130 * 129 / 2
    assert mh.block_sum(np.arange(3000.0), 2) == 3000 * 2999 / 2


def test_waves_per_document():
    assert [mh.waves(k) for k in (1, 512, 513, 2552, 2553, 4096, 6814)] == [8, 8, 8, 8, 7, 4, 2]
    for k in (513, 2552, 2553, 6814):
        assert mh.RED_DOUBLES + mh.waves(k) * k <= mh.LDS_DOUBLES


def test_combine_is_a_logsumexp_and_ess():
    rng = np.random.RandomState(1)
    lw = rng.standard_normal(300) * 5 - 700.0
    lw[7] = -np.inf
    ll, ess = mh.combine(lw, 8)
    w = np.exp(lw - lw.max())
    assert abs(ll - (lw.max() + math.log(w.sum()) - math.log(300))) < 1e-12
    assert abs(ess - w.sum() ** 2 / (w ** 2).sum()) < 1e-10
    assert mh.combine(np.full(5, -np.inf), 8) == (-math.inf, 0.0)
    assert mh.combine(np.full(40, -3.25), 8) == (-3.25, 40.0)
    assert mh.combine(np.array([-2.0]), 8) == (-2.0, 1.0)             # S < W: waves without a sample


def test_zero_counts_and_empty_documents():
    docs = [[], [(1, 0), (2, 3)], [(2, 3)]]
    indptr, ids, cnts = _csr(docs)
    ll, ess = mh.document_loglik(indptr, ids, cnts, LAM, ALPHA, 5, 64)
    assert ll[0] == 0.0 and ess[0] == 64.0
    # (document 1 and 2 sit at different indices d, so their draws differ: compare 1 with itself
    # without its zero-count entry)
    ll2, _ = mh.document_loglik(*_csr([[], [(2, 3)]]), LAM, ALPHA, 5, 64)
    assert ll[1] == ll2[1]


def test_symbol_and_method_exist(hip_lib):
    from trlda_amd import _ffi
    from trlda_amd.models import LDA
    assert "trlda_model_document_loglik" in _ffi.EXPORTED_SYMBOLS
    assert hasattr(hip_lib, "trlda_model_document_loglik")
    assert callable(LDA.document_log_likelihood)
    blob = open(_ffi.LIB_PATH, "rb").read()
    assert b"marginal_docs_kernel" in blob


def test_arguments_are_refused_before_any_device_work():
    from trlda_amd.models import OnlineLDA
    m = OnlineLDA.__new__(OnlineLDA)             # no constructor: nothing here may reach the library
    m._K, m._V, m._handle = 3, 4, None
    for bad in ("map", "", None, 3):
        with pytest.raises(TypeError, match="proposal"):
            m.document_log_likelihood([DOC], proposal=bad)
    with pytest.raises(TypeError, match="latents"):
        m.document_log_likelihood([DOC], proposal="Prior", latents=np.ones((3, 1)))
    with pytest.raises(RuntimeError, match="num_samples"):
        m.document_log_likelihood([DOC], num_samples=0)
    with pytest.raises(RuntimeError, match="2\\^32"):
        m.document_log_likelihood([DOC], num_samples=2 ** 32 // 3 + 1)
    with pytest.raises(TypeError):
        m.document_log_likelihood([DOC], num_samples=2.5)


def test_kernels_do_not_spill_vector_registers(hip_lib):
    """Eight waves per document leave each 256 registers; at sixteen (128) every variant spilled 56
    to 128 of them into scratch around the draws."""
    import os
    from helpers import kernel_resources
    from trlda_amd import _ffi
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    res = {k: v for k, v in kernel_resources(_ffi.LIB_PATH).items() if "marginal_docs_kernel" in k}
    assert len(res) == 9, sorted(res)
    for name, f in res.items():
        assert f["vgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_count"] <= 256, (name, f)
