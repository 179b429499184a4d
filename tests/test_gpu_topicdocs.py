"""Topic summaries of a DocumentIndex on the GPU (csrc/topicdocs_kernels.h): theta^, the
ranking per topic, the mean and the centred scatter against the restatement (tests/topicdocs_host.py)
of the device's own rows; exact ties, independence of the partition and of how the index was filled,
the Python forms, the model's state, the buffers and the errors.

Every array is small: at most 300 indexed documents (1100 once, at K = 8, to cross the growth copy)
and 513 topics.  Observed on the MI355X, as shares of the bounds below: theta^ of a
cosine index at most 6.5 of the 8 * 2^-53 allowed (K = 63) and bitwise the ordered restatement
everywhere; the mean at most 4.5 % of its bound (K = 17, N = 31); the scatter at most 3.1 % of its bound
(K = 17, N = 3; 0.4 % at N = 300), with the automatic and with a forced chunk alike."""
import os
import subprocess
import sys

import numpy as np
import pytest

import topicdocs_host as th

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GAP_FLOOR = 1e-9
MEASURES = ["hellinger", "cosine"]
N_MAX = 300
KS = [1, 3, 15, 16, 17, 63, 65, 130, 513]          # the Kp tail, the MFMA edge, the tile edge, three tiles
NS = [1, 2, 3, 5, 31, 33, 65]                      # the MFMA depth, the staging depth, ragged chunks
SHAPES = [(K, N_MAX) for K in KS] + [(17, N) for N in NS]

# theta^ of a cosine index against r / r.sum() of NumPy, in units of U = 2^-53, the largest relative
# error of one rounding.  Each side rounds its quotient once: 2 U.  The two sums differ in order only.
# The device's passes a term through ceil(K / 64) - 1 additions of its lane and six levels of a tree,
# NumPy's through an eight-way unrolled loop and three levels (pairwise blocks above 128 terms); on
# positive terms each is within (number of additions a term passes) U of the exact sum in the worst
# case, but the roundings have either sign and mostly cancel: on the inputs used here the device's
# order stays within 2.3 U and NumPy's within 4.1 U of the longdouble sum (both measured with NumPy
# alone, tests/topicdocs_host.py being the device's order), and they rarely err in opposite
# directions by their maxima at once.  2 U + d_dev + d_np <= 8 U is therefore what is asked, as for
# ROW_BOUND["cosine"] of test_gpu_docindex.py; it is not a worst-case bound.  The sharp statement is
# the one next to it: theta^ is bitwise the restatement that adds in the device's order.
# (A hellinger theta^ is one multiply: bitwise rows() ** 2.)
THETA_BOUND = 8 * U


def mean_bound(theta):
    """|m_dev - m_longdouble| per topic: any order of N additions errs by (N - 1) u sum |terms|, the
    division adds u / 2, and the allowance of 16 covers the longdouble side: (N + 16) 2 u sum / N."""
    N = theta.shape[0]
    return (N + 16) * 2 * U * np.abs(theta).sum(axis=0) / N


def scatter_bound(A, N):
    """|S_dev - S_restated| with both centred on the device's mean: any order of n additions errs
    by (n - 1) u sum |terms|, and each term carries about 3 u from its two subtractions and the
    product: (N + 16) 4 u A_ij, A_ij = sum_d |theta_di - m_i| |theta_dj - m_j|."""
    return (N + 16) * 4 * U * A.astype(np.float64)


@pytest.fixture(scope="module")
def hip():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


def _model(K, V=8, lam=None, alpha=.1, eta=.3):
    """An OnlineLDA holding `lam` without the constructor's K V 100 draws."""
    from trlda_amd.models import OnlineLDA
    if lam is None:
        lam = np.random.RandomState(77).gamma(2.0, 1.0, size=(K, V)) + 0.05
    m = OnlineLDA.__new__(OnlineLDA)
    m._num_documents = 1000
    m._update_count = 0
    m._ada_tau = 1000.
    m._ada_rho = 1. / m._ada_tau
    m._ada_sq_norm = 1.
    m._setup(V, K, alpha, eta, None, _lambda=np.asfortranarray(lam))
    return m


def _gammas(K, n, seed):
    """n gamma columns: sparse-ish topic weights of very different totals."""
    rng = np.random.RandomState(seed)
    g = rng.gamma(0.3, 1.0, size=(K, n)) + 0.01
    return np.asfortranarray(g * rng.uniform(0.5, 40.0, size=n))


def _case(K, N):
    return _gammas(K, N_MAX, 4000 + K)[:, :N]


def _state():
    from trlda_amd import _ffi
    s = np.zeros(33, dtype=np.uint32)
    _ffi.lib().trlda_rng_get_state(s)
    return s


def _tops(N):
    return sorted({1, min(10, N), min(100, N)})


def _chunk(N):
    """Rows per chunk that cut N into at least five chunks (N chunks below 5) with a ragged last."""
    return max(1, (N - 1) // 5)


# 1. theta^ and the ranking ---------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K,N", SHAPES)
def test_theta_and_ranking(hip, K, N, measure):
    g = _case(K, N)
    m = _model(K)
    ix = m.document_index(measure)
    ix.add_gamma(g)
    rows = ix.rows()
    restated = th.theta_hat(rows, measure)
    top = min(N, 100)
    want_ids, want_theta, gap = th.top_documents(restated, top)
    if K == 1:
        # (the one topic holds every document whole: r = 1 and theta^ = 1 exactly under both measures,
        # so the ranking is by id alone and there is no gap to ask for)
        assert np.all(rows == 1.0) and np.all(restated == 1.0)
    elif measure == "cosine":
        # (hellinger needs no gap: its theta^ is reproduced bit for bit)
        assert gap.min() > GAP_FLOOR, gap.min()
    ids, theta = ix.topic_documents(top, return_theta=True)
    assert ids.dtype == np.int64 and theta.dtype == np.float64 and ids.shape == theta.shape == (K, top)
    assert np.array_equal(ids, want_ids)
    plain = rows / rows.sum(axis=1)[:, None] if measure == "cosine" else rows ** 2
    picked = plain.T[np.arange(K)[:, None], ids]
    err = float(np.max(np.abs(theta - picked) / picked))
    print("K = %d N = %d %s: theta^ max rel err %.2f u, bitwise the restatement: %s, smallest gap %.2e"
          % (K, N, measure, err / U, np.array_equal(theta, want_theta), gap.min()))
    if measure == "hellinger":
        assert np.array_equal(theta, picked)
    else:
        assert err <= THETA_BOUND, err / U
    assert np.array_equal(theta, want_theta)                 # the restatement adds in the device's order
    if N <= 100:                                             # every theta^ comes back
        back = np.empty((N, K))
        back[ids, np.arange(K)[:, None]] = theta
        assert np.array_equal(np.sort(ids, axis=1), np.tile(np.arange(N), (K, 1)))
        if measure == "hellinger":
            assert np.array_equal(back, rows ** 2)
        else:
            assert np.max(np.abs(back - plain) / plain) <= THETA_BOUND
    # the same bits for a shorter list, slabs of 16 rows, and without theta
    for rows_per_slab in (0, 16):
        ix.set_slab_rows(rows_per_slab)
        for top_n in _tops(N):
            ids_n, theta_n = ix.topic_documents(top_n, return_theta=True)
            assert np.array_equal(ids_n, ids[:, :top_n]) and np.array_equal(theta_n, theta[:, :top_n])
            assert np.array_equal(ix.topic_documents(top_n), ids_n)
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_exact_ties_rank_by_id(hip, measure):
    """The same gamma column at ids 3, 40 and 299, slabs of 16, 64 and 2048 rows: the three lie in
    different slabs of the first two."""
    K = 20
    g = _case(K, N_MAX).copy(order="F")
    g[:, 40] = g[:, 3]
    g[:, 299] = g[:, 3]
    m = _model(K)
    ix = m.document_index(measure)
    ix.add_gamma(g)
    restated = th.theta_hat(ix.rows(), measure)
    assert np.array_equal(restated[3], restated[40]) and np.array_equal(restated[3], restated[299])
    want_ids, want_theta, _ = th.top_documents(restated, 100)
    seen = 0
    for rows_per_slab in (16, 64, 0):
        ix.set_slab_rows(rows_per_slab)
        ids, theta = ix.topic_documents(100, return_theta=True)
        assert np.array_equal(ids, want_ids) and np.array_equal(theta, want_theta)
        for k in range(K):
            at = list(ids[k]).index(3) if 3 in ids[k] else None
            if at is not None and at + 2 < 100:
                assert list(ids[k, at:at + 3]) == [3, 40, 299] and theta[k, at] == theta[k, at + 2]
                seen += 1
    assert seen >= 3
    m.close()


def test_results_do_not_depend_on_how_the_index_was_filled(hip):
    """1100 documents at K = 8 in ragged adds of 1, 7 and 64 rows without reserve -- the table starts
    at 1024 rows and is copied into 2048 -- against one add into reserved room."""
    K, N = 8, 1100
    g = _gammas(K, N, 12)
    m = _model(K)
    for measure in MEASURES:
        whole = m.document_index(measure)
        whole.reserve(N)
        whole.add_gamma(g)
        parts = m.document_index(measure)
        at, step = 0, 0
        while at < N:
            n = min((1, 7, 64)[step % 3], N - at)
            assert parts.add_gamma(g[:, at:at + n]) == at
            at, step = at + n, step + 1
        assert len(parts) == N and np.array_equal(parts.rows(), whole.rows())
        for top_n in (1, 10, 100):
            a, b = whole.topic_documents(top_n, True), parts.topic_documents(top_n, True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        want_ids, want_theta, _ = th.top_documents(th.theta_hat(whole.rows(), measure), 100)
        assert np.array_equal(a[0], want_ids) and np.array_equal(a[1], want_theta)
        (ma, sa), (mb, sb) = whole._moments(), parts._moments()
        assert np.array_equal(ma, mb) and np.array_equal(sa, sb)
    m.close()


# 2. the mean and the scatter -------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K,N", SHAPES)
def test_moments(hip, K, N, measure):
    g = _case(K, N)
    m = _model(K)
    ix = m.document_index(measure)
    ix.add_gamma(g)
    theta = th.theta_hat(ix.rows(), measure)
    mean, S = ix._moments()
    assert mean.shape == (K,) and S.shape == (K, K) and mean.dtype == S.dtype == np.float64
    m_err = np.abs(mean.astype(np.longdouble) - th.mean(theta)).astype(np.float64)
    m_bound = mean_bound(theta)
    assert np.all(m_err <= m_bound), float(np.max(m_err / m_bound))
    # centred on the device's own mean: the mean's error is tested once, above
    want, A = th.scatter(theta, mean)
    bound = scatter_bound(A, N)
    shares = []
    for rows in (0, _chunk(N)):
        ix.set_moment_chunk(rows)
        mean_c, S_c = ix._moments()
        assert np.array_equal(mean_c, mean)
        err = np.abs(S_c.astype(np.longdouble) - want).astype(np.float64)
        assert np.all(err <= bound), (rows, float(np.max(err / np.maximum(bound, 1e-300))))
        shares.append(float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.array_equal(S_c, S_c.T) and np.all(np.diag(S_c) >= 0)
        # sum_j (theta^_j - m_j) = 0 for every document: the rows of S sum to (nearly) nothing
        assert np.all(np.abs(S_c.sum(axis=1)) <= 1e-13 * np.abs(S_c).sum(axis=1))
        if N == 1:
            assert np.array_equal(S_c, np.zeros((K, K)))
        again = ix._moments()
        assert np.array_equal(again[0], mean_c) and np.array_equal(again[1], S_c)
    print("K = %d N = %d %s: mean err / bound %.2e, scatter err / bound %.2e (automatic chunk) %.2e (chunks of %d)"
          % (K, N, measure, float(np.max(m_err / m_bound)), shares[0], shares[1], _chunk(N)))
    ix.set_moment_chunk(0)
    # the Python forms: the restatement's closing arithmetic on the device's S
    assert np.array_equal(ix.topic_correlations(), th.correlation(S), equal_nan=True)
    if N == 1:
        assert np.all(np.isnan(ix.topic_correlations()))
        with pytest.raises(ValueError):
            ix.topic_covariance()
    else:
        cov, mean_p = ix.topic_covariance(return_mean=True)
        assert np.array_equal(cov, th.covariance(S, N, 1)) and np.array_equal(mean_p, mean)
        assert np.array_equal(ix.topic_covariance(), cov)
        if K > 1 and N > 2:
            corr = ix.topic_correlations()
            assert np.all(np.diag(corr) == 1.0) and np.all(np.abs(corr) <= 1.0)
            loose = np.corrcoef(theta, rowvar=False)
            assert np.max(np.abs(corr - loose)) <= 1e-9
    assert np.array_equal(ix.topic_covariance(ddof=0), th.covariance(S, N, 0))
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_zero_variance_gives_nan(hip, measure):
    """The same gamma column twice: the mean is the column's theta^ exactly, every variance 0."""
    K = 17
    g = _case(K, 1)
    m = _model(K)
    ix = m.document_index(measure)
    ix.add_gamma(g)
    ix.add_gamma(g)
    mean, S = ix._moments()
    assert len(ix) == 2 and np.array_equal(mean, th.theta_hat(ix.rows(), measure)[0])
    assert np.array_equal(S, np.zeros((K, K)))
    corr = ix.topic_correlations()
    assert corr.shape == (K, K) and np.all(np.isnan(corr))
    assert np.array_equal(ix.topic_covariance(), np.zeros((K, K)))
    # a third, different document: every variance positive, nothing is NaN, the diagonal is 1
    ix.add_gamma(_case(K, 2)[:, 1])
    corr = ix.topic_correlations()
    assert np.all(np.isfinite(corr)) and np.all(np.diag(corr) == 1.0)
    assert np.array_equal(corr, ix.topic_correlations(), equal_nan=True)
    m.close()


# 3. the model's state, the buffers, the errors ---------------------------------------------------------
def test_state_is_left_alone(hip):
    import trlda_amd
    K, N = 16, 40
    m = _model(K, alpha=.2, eta=.05)
    ix = m.document_index("cosine")
    ix.add_gamma(_case(K, N))
    rows = ix.rows()
    before = (np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count)
    trlda_amd.seed(9)
    state = _state()
    ix.topic_documents(10, return_theta=True)
    ix.topic_covariance(return_mean=True)
    ix.topic_correlations()
    ix.set_moment_chunk(8)
    ix.topic_correlations()
    assert np.array_equal(state, _state())
    assert len(ix) == N and np.array_equal(ix.rows(), rows)
    assert np.array_equal(np.asarray(m.lambdas), before[0]) and np.array_equal(np.asarray(m.alpha), before[1])
    assert m.eta == before[2] and m.update_count == before[3]
    m.close()


def test_no_buffer_is_kept_by_the_calls(hip):
    """A fresh process (the count is the process's): the calls leave the live count as it was, and
    after close() the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "topicdocs_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout


def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K, N = 8, 12
    m = _model(K)
    ix = m.document_index("cosine")
    trlda_amd.seed(3)
    before = _state()
    ids = np.full((K, 101), -7, dtype=np.int64)
    theta = np.full((K, 101), -7.)
    mean = np.full(K, -7.)
    S = np.full((K, K), -7.)

    def refused(top_n):
        assert hip.trlda_docindex_topic_documents(ix._handle, top_n, ids.ctypes.data, theta.ctypes.data) == _ffi.ERR_ARG
        assert hip.trlda_docindex_topic_documents(ix._handle, top_n, ids.ctypes.data, None) == _ffi.ERR_ARG

    # an empty index
    refused(1)
    assert hip.trlda_docindex_topic_moments(ix._handle, mean.ctypes.data, S.ctypes.data) == _ffi.ERR_ARG
    with pytest.raises(RuntimeError, match="top_n"):
        ix.topic_documents(1)
    with pytest.raises(ValueError):
        ix.topic_covariance(ddof=0)
    with pytest.raises(_ffi.TrldaError, match="empty"):
        ix.topic_correlations()
    ix.add_gamma(_case(K, N))
    for top_n in (0, -1, 101, N + 1):
        refused(top_n)
        with pytest.raises(RuntimeError, match="top_n"):
            ix.topic_documents(top_n)
    with pytest.raises(TypeError):
        ix.topic_documents(2.5)
    with pytest.raises(ValueError):
        ix.topic_covariance(ddof=N)
    # NULL outputs, a negative chunk
    assert hip.trlda_docindex_topic_documents(ix._handle, 1, None, theta.ctypes.data) == _ffi.ERR_ARG
    assert hip.trlda_docindex_topic_moments(ix._handle, None, S.ctypes.data) == _ffi.ERR_ARG
    assert hip.trlda_docindex_topic_moments(ix._handle, mean.ctypes.data, None) == _ffi.ERR_ARG
    with pytest.raises(_ffi.TrldaError):
        ix.set_moment_chunk(-1)
    # nothing was drawn or written
    assert len(ix) == N and np.array_equal(before, _state())
    assert np.all(ids == -7) and np.all(theta == -7.) and np.all(mean == -7.) and np.all(S == -7.)
    # the index still works after the refusals
    got = ix.topic_documents(N)
    assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(N), (K, 1)))
    ix.close()
    for call in (lambda: ix.topic_documents(1), ix.topic_correlations, lambda: ix.topic_covariance(ddof=0),
                 lambda: ix.set_moment_chunk(0)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    m.close()
