"""CPU checks of the topic summaries of a document index: the restatement (tests/topicdocs_host.py)
against NumPy's own lexsort, cov and corrcoef, and what the library and ``DocumentIndex`` answer
before any GPU work."""
import numpy as np
import pytest

import docindex_host as dh
import topicdocs_host as th


LD_STEP = np.longdouble(0.125)


def _theta(N, K, seed):
    g = np.random.RandomState(seed).gamma(0.3, 1.0, size=(K, N)) + 0.01
    return (g / g.sum(axis=0)).T


def test_theta_hat_from_rows():
    g = np.random.RandomState(3).gamma(0.3, 1.0, size=(130, 9)) + 0.01
    theta = (g / g.sum(axis=0)).T
    hel = th.theta_hat(dh.rows(g, "hellinger"), "hellinger")
    assert np.array_equal(hel, np.sqrt(theta) ** 2) and np.max(np.abs(hel - theta) / theta) <= 2 ** -51
    r = dh.rows(g, "cosine")
    cos = th.theta_hat(r, "cosine")
    assert np.max(np.abs(cos - theta) / theta) <= 2 ** -49
    # the ordered sum is a sum: within a few u of NumPy's, and exact where every order is
    assert np.max(np.abs(th.row_sums(r) - r.sum(axis=1)) / r.sum(axis=1)) <= 2 ** -50
    ints = np.arange(1.0, 131.0)[None, :] * np.array([[1.0], [3.0]])
    assert np.array_equal(th.row_sums(ints), [8515.0, 25545.0])
    assert np.array_equal(th.row_sums(np.array([[0.25]])), [0.25])
    with pytest.raises(ValueError):
        th.theta_hat(r, "manhattan")


def test_ranking_is_the_lexsort():
    theta = _theta(40, 5, 11)
    theta[7] = theta[3]                                   # equal values: the smaller id first
    theta[20, 2] = theta[5, 2]
    ids = np.arange(40)
    order = th.rank(theta)
    for k in range(5):
        assert np.array_equal(order[k], np.lexsort((ids, -theta[:, k])))
        assert list(order[k]).index(7) == list(order[k]).index(3) + 1
    assert list(order[2]).index(20) == list(order[2]).index(5) + 1
    top, val, gap = th.top_documents(theta, 3)
    assert top.shape == val.shape == (5, 3) and top.dtype == np.int64 and val.dtype == np.float64
    assert np.array_equal(top, order[:, :3]) and np.array_equal(val, theta.T[np.arange(5)[:, None], top])
    assert np.all(np.diff(val, axis=1) <= 0)
    assert np.all(th.top_documents(theta, 40)[2] == 0)    # the tie is among all 40
    # the report: relative, and the first value left out counts
    ranked = np.array([[0.5, 0.25, 0.125, 0.125],
                       [0.5, 0.5, 0.25, 0.125],
                       [1.0, 0.5, 0.375, 0.25]])
    assert np.array_equal(th.gaps(ranked, 1), [0.5, 0.0, 0.5])
    assert np.array_equal(th.gaps(ranked, 2), [0.5, 0.0, 0.25])
    assert np.array_equal(th.gaps(ranked, 3), [0.0, 0.0, 0.25])
    assert np.array_equal(th.gaps(ranked, 4), th.gaps(ranked, 3))
    assert np.all(np.isinf(th.gaps(ranked[:, :1], 1)))


@pytest.mark.parametrize("N,K", [(2, 3), (33, 17), (300, 65)])
def test_moments_against_numpy(N, K):
    theta = _theta(N, K, 100 * N + K)
    m = th.mean(theta)
    S, A = th.scatter(theta)
    assert m.dtype == S.dtype == A.dtype == np.longdouble and S.shape == A.shape == (K, K)
    assert np.max(np.abs(m.astype(np.float64) - theta.mean(axis=0))) <= 1e-15
    for ddof in (0, 1):
        cov = th.covariance(S, N, ddof).astype(np.float64)
        want = np.cov(theta, rowvar=False, ddof=ddof).reshape(K, K)
        assert np.max(np.abs(cov - want)) <= 1e-12 * np.max(np.abs(want))
    corr = th.correlation(S).astype(np.float64)
    assert np.max(np.abs(corr - np.corrcoef(theta, rowvar=False))) <= 1e-12
    assert np.all(np.diag(corr) == 1.0) and np.all(np.abs(corr) <= 1.0)
    assert np.array_equal(S, S.T) and np.all(np.diag(S) >= 0) and np.all(A >= np.abs(S))
    # sum_j (theta_j - m_j) = 0 for every document: the rows of S sum to (nearly) nothing
    assert np.all(np.abs(S.sum(axis=1)) <= 1e-13 * np.abs(S).sum(axis=1))
    # about another centre: S' = S + N (m - c)(m - c)^T
    c = m + LD_STEP
    S2, _ = th.scatter(theta, c)
    assert np.max(np.abs(S2 - (S + N * np.outer(m - c, m - c)))) <= 1e-15


def test_zero_variance_gives_nan():
    theta = _theta(12, 4, 5)
    theta[:, 2] = 0.25                                    # a topic every document holds equally
    S, _ = th.scatter(theta)
    assert S[2, 2] == 0 and np.all(S[2] == 0)
    for corr in (th.correlation(S), th.correlation(S.astype(np.float64))):
        assert np.all(np.isnan(corr[2])) and np.all(np.isnan(corr[:, 2]))
        rest = np.delete(np.delete(corr, 2, axis=0), 2, axis=1)
        assert np.all(np.isfinite(rest)) and np.all(np.diag(rest) == 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.corrcoef(theta, rowvar=False)
    assert np.array_equal(np.isnan(want), np.isnan(th.correlation(S)))
    # a single document: an exact zero scatter, nothing but NaN
    one, _ = th.scatter(theta[:1])
    assert np.all(one == 0) and np.all(np.isnan(th.correlation(one)))


def test_closing_arithmetic_of_the_index_is_the_restatement():
    from trlda_amd.index import _correlation
    theta = _theta(50, 6, 8)
    theta[:, 4] = 0.125
    S = th.scatter(theta)[0].astype(np.float64)
    assert np.array_equal(_correlation(S), th.correlation(S), equal_nan=True)
    assert np.array_equal(S / float(50 - 1), th.covariance(S, 50, 1))
    # a value a hair outside [-1, 1] is clamped
    S = np.array([[1.0, 1.0 + 2 ** -52], [1.0 + 2 ** -52, 1.0]])
    assert np.array_equal(_correlation(S), np.ones((2, 2)))
    S[0, 1] = S[1, 0] = -S[0, 1]
    assert np.array_equal(_correlation(S), [[1.0, -1.0], [-1.0, 1.0]])


# -- the library ----------------------------------------------------------------------------------
def test_topicdocs_entry_points_are_exported(hip_lib):
    from trlda_amd import _ffi
    names = ["trlda_docindex_" + n for n in ("topic_documents", "topic_moments", "set_moment_chunk")]
    for name in names:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    # (no index: the argument check answers before any device is touched)
    ids, theta = np.full(4, -7, dtype=np.int64), np.full(4, -7.0)
    assert hip_lib.trlda_docindex_topic_documents(None, 1, ids.ctypes.data, theta.ctypes.data) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_topic_documents(None, 1, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_topic_moments(None, theta.ctypes.data, theta.ctypes.data) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_topic_moments(None, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_set_moment_chunk(None, 0) == _ffi.ERR_ARG
    assert np.all(ids == -7) and np.all(theta == -7.0)


class _Shell(object):
    """A DocumentIndex without a device side: `n` documents, no handle."""

    def __new__(cls, n):
        from trlda_amd.index import DocumentIndex

        class Shell(DocumentIndex):
            def __len__(self):
                return n
        x = DocumentIndex.__new__(Shell)
        x._handle, x._K, x._measure = None, 3, 0
        return x


def test_python_argument_errors_come_before_any_gpu_work():
    x = _Shell(5)
    for ddof in (5, 6, 5.5, 100):
        with pytest.raises(ValueError):
            x.topic_covariance(ddof=ddof)
        with pytest.raises(ValueError):
            x.topic_covariance(ddof, return_mean=True)
    with pytest.raises(ValueError):
        _Shell(1).topic_covariance()                      # ddof = 1 of one document
    with pytest.raises(ValueError):
        _Shell(0).topic_covariance(ddof=0)
    for bad in (2.5, "3", None, [1]):
        with pytest.raises(TypeError):
            x.topic_documents(top_n=bad)
    for bad in (0, 6, -1, 101):
        with pytest.raises(RuntimeError, match="top_n"):
            x.topic_documents(bad)
    with pytest.raises(RuntimeError, match="top_n"):
        _Shell(300).topic_documents(101)
    with pytest.raises(TypeError):
        x.set_moment_chunk(1.5)
    # what passes the checks reaches the index, which is closed
    for call in (lambda: x.topic_documents(3), lambda: x.topic_documents(5, return_theta=True), x.topic_covariance,
                 lambda: x.topic_covariance(ddof=0), x.topic_correlations, lambda: x.set_moment_chunk(0)):
        with pytest.raises(RuntimeError, match="closed"):
            call()


def test_topicdocs_kernels_do_not_spill(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    mine = {k: v for k, v in res.items() if "topicdocs_" in k}
    # scale, select, mean, mean_sum, scatter, finish
    assert len(mine) == 6, sorted(mine)
    for part in ("scale", "select", "mean_kernel", "mean_sum", "scatter", "finish"):
        assert sum("topicdocs_" + part in k for k in mine) == 1, (part, sorted(mine))
    for name, f in mine.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_spill_count"] == 0, (name, f)
        assert f["sgpr_spill_count"] == 0, (name, f)
        assert f["vgpr_count"] <= 256, (name, f)
        assert f["group_segment_fixed_size"] <= 64 * 1024, (name, f)
    # the pins of the kernels this feature leans on hold: it adds no kernel of theirs
    assert sum("docindex_" in k for k in res) == 4 and sum("topicdist_" in k for k in res) == 7
