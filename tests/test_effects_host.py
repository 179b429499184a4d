"""CPU checks of topic prevalence against document metadata: the restatement (tests/effects_host.py)
against NumPy's own lstsq, average, var and histogram (and SciPy's linregress where it imports), the
closing arithmetic of ``DocumentIndex.topic_effects`` and ``group_prevalence``, the binning of
``topic_trends``, and what the library and ``DocumentIndex`` answer before any GPU work."""
import numpy as np
import pytest

import effects_host as eh

LD = np.longdouble


def _theta(N, K, seed):
    g = np.random.RandomState(seed).gamma(0.3, 1.0, size=(K, N)) + 0.01
    return (g / g.sum(axis=0)).T


def _weights(N, seed):
    w = np.random.RandomState(seed).uniform(0.5, 30.0, size=N)
    w[::7] = 0.0
    return w


# -- the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_restated_regression_against_lstsq(weighted):
    N, K, P = 120, 7, 4
    theta = _theta(N, K, 3)
    X = np.random.RandomState(4).normal(size=(N, P))
    w = _weights(N, 5) if weighted else None
    Z = eh.design(X)
    G, AG, C, AC = eh.products(theta, Z, w)
    assert G.dtype == C.dtype == LD and G.shape == (P + 1, P + 1) and C.shape == (P + 1, K)
    assert np.max(np.abs(G - G.T)) <= 1e-15 * np.max(np.abs(G)) and np.all(AG >= np.abs(G)) and np.all(AC >= np.abs(C))
    coef = np.linalg.solve(G.astype(np.float64), C.astype(np.float64))
    want, want_rss = eh.lstsq(theta, Z, w)
    assert np.max(np.abs(coef - want)) <= 1e-12
    rss, E = eh.residuals(theta, Z, coef, w)
    assert np.max(np.abs(rss.astype(np.float64) - want_rss) / want_rss) <= 1e-10
    assert np.all(E > 0) and np.all(E <= 1e-12 * rss.astype(np.float64) + 1e-18)
    # sum_k theta = 1: the intercept row sums to 1 over the topics, every other row to 0
    assert abs(coef[0].sum() - 1.0) <= 1e-12 and np.max(np.abs(coef[1:].sum(axis=1))) <= 1e-12


def test_one_covariate_against_linregress():
    from trlda_amd.index import _effects_closing
    N, K = 80, 3
    theta = _theta(N, K, 9)
    x = np.random.RandomState(10).normal(size=N)
    Z = eh.design(x)
    G, _, C, _ = eh.products(theta, Z)
    G, C = G.astype(np.float64), C.astype(np.float64)
    coef = np.linalg.solve(G, C)
    rss = eh.residuals(theta, Z, coef)[0].astype(np.float64)
    tss = eh.residuals(theta, np.ones((N, 1)), (C[0] / G[0, 0])[None, :])[0].astype(np.float64)
    out = _effects_closing(G, C, rss, tss, N, True)
    for k in range(K):
        # the closed forms of simple regression
        sxx = np.sum((x - x.mean()) ** 2)
        slope = np.sum((x - x.mean()) * (theta[:, k] - theta[:, k].mean())) / sxx
        assert abs(out["coef"][1, k] - slope) <= 1e-13
        assert abs(out["stderr"][1, k] - np.sqrt(out["rss"][k] / (N - 2) / sxx)) <= 1e-13
        assert abs(out["r2"][k] - np.corrcoef(x, theta[:, k])[0, 1] ** 2) <= 1e-12
    try:
        from scipy import stats
    except ImportError:
        return
    for k in range(K):
        ref = stats.linregress(x, theta[:, k])
        assert abs(out["coef"][1, k] - ref.slope) <= 1e-13 and abs(out["coef"][0, k] - ref.intercept) <= 1e-13
        assert abs(out["stderr"][1, k] - ref.stderr) <= 1e-13
        assert abs(out["stderr"][0, k] - ref.intercept_stderr) <= 1e-13
        assert abs(out["r2"][k] - ref.rvalue ** 2) <= 1e-12
        assert abs(out["tvalues"][1, k] - ref.slope / ref.stderr) <= 1e-9 * abs(out["tvalues"][1, k])


@pytest.mark.parametrize("weighted", [False, True])
def test_restated_groups_against_numpy(weighted):
    from trlda_amd.index import _group_variance, _positive_counts
    N, K, G = 700, 5, 4
    theta = _theta(N, K, 21)
    labels = np.random.RandomState(22).randint(-1, G - 1, size=N)        # group G - 1 is empty
    labels[:600][labels[:600] == 0] = 1                                  # ... and group 1 passes one chunk
    w = _weights(N, 23) if weighted else None
    mean, counts, var = eh.group_prevalence(theta, labels, G, w)
    assert counts.dtype == np.int64 and counts[G - 1] == 0 and counts[1] > eh.CHUNK
    assert np.array_equal(counts, np.bincount(labels[labels >= 0], minlength=G))
    for g in range(G - 1):
        ids = labels == g
        assert np.max(np.abs(mean[:, g] - np.average(theta[ids], axis=0, weights=None if w is None else w[ids]))) <= 1e-15
        if w is None:
            assert np.max(np.abs(var[:, g] / np.var(theta[ids], axis=0, ddof=1) - 1)) <= 1e-12
        else:
            n = np.count_nonzero(w[ids] > 0)
            m = np.average(theta[ids], axis=0, weights=w[ids])
            want = np.average((theta[ids] - m) ** 2, axis=0, weights=w[ids]) * n / (n - 1)
            assert np.max(np.abs(var[:, g] / want - 1)) <= 1e-12
    assert np.all(np.isnan(mean[:, G - 1])) and np.all(np.isnan(var[:, G - 1]))
    # the longdouble form and its bounds contain the ordered one
    exact, A, _, _, W, n = eh.group_exact(theta, labels, G, w)
    assert np.all(np.abs(mean - exact.astype(np.float64))[:, :G - 1] <= eh.group_mean_bound(A, n)[:, :G - 1])
    _, _, SS, B, _, _ = eh.group_exact(theta, labels, G, w, centre=np.nan_to_num(mean))
    S, Wd = eh.group_pass(theta, labels, G, w)
    dev_ss = eh.group_pass(theta, labels, G, w, S / np.where(Wd > 0, Wd, 1.0))[0]
    assert np.all(np.abs(dev_ss - SS.astype(np.float64)) <= eh.group_ss_bound(B, n))
    # the index's closing arithmetic is the restatement's
    lab = labels.astype(np.int32)
    mine = _group_variance(np.asfortranarray(dev_ss), Wd, _positive_counts(lab, w, G), 1, w is not None)
    assert mine.flags.f_contiguous and np.array_equal(mine, var, equal_nan=True)
    # one member: a variance needs two (ddof = 1), and ddof = 0 gives an exact zero
    one = np.full(N, -1)
    one[5] = 0
    m1, c1, v1 = eh.group_prevalence(theta, one, 1, None)
    assert np.array_equal(m1[:, 0], theta[5]) and c1[0] == 1 and np.all(np.isnan(v1))
    assert np.all(eh.group_prevalence(theta, one, 1, None, ddof=0)[2] == 0.0)


# -- the closing arithmetic ------------------------------------------------------------------------------
def test_closing_of_a_one_hot_design_gives_the_group_means():
    from trlda_amd.index import _effects_closing
    N, K, G = 90, 6, 4
    theta = _theta(N, K, 31)
    labels = np.arange(N) % G
    w = _weights(N, 32)
    Z = (labels[:, None] == np.arange(G)[None, :]).astype(np.float64)
    for weights in (None, w):
        Gm, _, C, _ = eh.products(theta, Z, weights)
        Gm, C = Gm.astype(np.float64), C.astype(np.float64)
        coef = C / np.diag(Gm)[:, None]
        rss = eh.residuals(theta, Z, coef, weights)[0].astype(np.float64)
        nobs = N if weights is None else int(np.count_nonzero(weights > 0))
        out = _effects_closing(Gm, C, rss, None, nobs, False)
        assert "tss" not in out and "r2" not in out
        mean, counts, var = eh.group_prevalence(theta, labels, G, weights, ddof=0)
        assert np.max(np.abs(out["coef"].T - mean)) <= 1e-15
        # rss: the within-group sums of squares
        _, _, SS, _, W, _ = eh.group_exact(theta, labels, G, weights)
        assert np.max(np.abs(out["rss"] - SS.sum(axis=1).astype(np.float64))) <= 1e-15
        assert out["dof"] == nobs - G and out["nobs"] == nobs
        assert np.max(np.abs(np.diag(out["cov_unscaled"]) - 1.0 / np.diag(Gm))) <= 1e-15
        assert np.array_equal(out["sigma2"], out["rss"] / (nobs - G))


def test_closing_of_an_intercept_only_design():
    from trlda_amd.index import _effects_closing
    N, K = 50, 4
    theta = _theta(N, K, 41)
    Z = np.ones((N, 1))
    G, _, C, _ = eh.products(theta, Z)
    G, C = G.astype(np.float64), C.astype(np.float64)
    mean = C / G[0, 0]
    rss = eh.residuals(theta, Z, mean)[0].astype(np.float64)
    out = _effects_closing(G, C, rss, rss, N, True)
    assert np.max(np.abs(out["coef"][0] - theta.mean(axis=0))) <= 1e-16
    centred = theta - theta.mean(axis=0)
    assert np.max(np.abs(out["rss"] - np.diag(centred.T.dot(centred)))) <= 1e-15
    assert np.all(out["r2"] == 0.0) and np.array_equal(out["tss"], rss)
    assert np.max(np.abs(out["stderr"][0] - np.sqrt(np.var(theta, axis=0, ddof=1) / N))) <= 1e-15


def test_rank_deficiency_and_degrees_of_freedom():
    from trlda_amd.index import _effects_closing, _effects_solve
    N, K = 40, 3
    theta = _theta(N, K, 51)
    X = np.random.RandomState(52).normal(size=(N, 3))
    for Z in (eh.design(np.hstack([X, X[:, :1]])),            # a duplicated column
              eh.design(np.hstack([X, X[:, :1] * 3.0])),      # ... up to its scale
              np.hstack([X, np.zeros((N, 1))])):              # a column of zeros
        G, _, C, _ = eh.products(theta, Z)
        with pytest.raises(ValueError, match="rank deficient"):
            _effects_solve(G.astype(np.float64), C.astype(np.float64))
        with pytest.raises(ValueError, match="rank deficient"):
            _effects_closing(G.astype(np.float64), C.astype(np.float64), np.ones(K), np.ones(K), N, True)
    # N < P'
    Z = eh.design(np.random.RandomState(53).normal(size=(4, 6)))
    G, _, C, _ = eh.products(theta[:4], Z)
    with pytest.raises(ValueError, match="rank deficient"):
        _effects_closing(G.astype(np.float64), C.astype(np.float64), np.zeros(K), np.ones(K), 4, True)
    # N = P': an exact fit, no degrees of freedom
    Z = eh.design(np.random.RandomState(54).normal(size=(4, 3)))
    G, _, C, _ = eh.products(theta[:4], Z)
    out = _effects_closing(G.astype(np.float64), C.astype(np.float64), np.zeros(K), np.ones(K), 4, True)
    assert out["dof"] == 0 and np.all(np.isfinite(out["coef"]))
    assert np.all(np.isnan(out["stderr"])) and np.all(np.isnan(out["tvalues"])) and np.all(np.isnan(out["sigma2"]))
    assert np.max(np.abs(Z.dot(out["coef"]) - theta[:4])) <= 1e-12
    # a badly scaled but full-rank design passes: the equilibration takes the scale out
    scale = np.array([1.0, 2.0 ** -20, 1.0, 2.0 ** 20])
    Z = eh.design(X) * scale
    G, _, C, _ = eh.products(theta, Z)
    coef, cov = _effects_solve(G.astype(np.float64), C.astype(np.float64))
    want = eh.lstsq(theta, eh.design(X))[0] / scale[:, None]             # (lstsq itself wants the scale out)
    assert np.max(np.abs(coef - want) / np.max(np.abs(want), axis=1, keepdims=True)) <= 1e-10
    assert np.array_equal(cov, cov.T)


# -- the binning -----------------------------------------------------------------------------------------
def test_time_labels_against_histogram():
    from trlda_amd.index import _time_labels
    rng = np.random.RandomState(61)
    t = rng.uniform(1990.0, 2020.0, size=500)
    t[:5] = [np.nan, np.inf, -np.inf, t[5:].min(), t[5:].max()]
    t[5:].sort()
    for bins in (1, 7, 10):
        edges, lab = _time_labels(t, bins)
        finite = t[np.isfinite(t)]
        want, want_edges = np.histogram(finite, bins)
        assert lab.dtype == np.int32 and np.array_equal(edges, want_edges)
        assert np.array_equal(np.bincount(lab[lab >= 0], minlength=bins), want)
        assert np.array_equal(lab[:3], [-1, -1, -1]) and lab[3] == 0 and lab[4] == bins - 1
    given = np.array([1995.0, 2000.0, 2000.5, 2010.0])
    t[10:13] = [1995.0, 2000.0, 2010.0]                                  # on the edges: the last one closed
    edges, lab = _time_labels(t, given)
    assert np.array_equal(edges, given)
    assert np.array_equal(np.bincount(lab[lab >= 0], minlength=3), np.histogram(t[np.isfinite(t)], given)[0])
    assert np.array_equal(lab[10:13], [0, 1, 2])
    assert np.all(lab[np.isfinite(t) & ((t < 1995.0) | (t > 2010.0))] == -1) and np.all(lab[:3] == -1)
    assert np.count_nonzero(lab == -1) > 3
    # integers pass as times; one distinct value is one bin around it, as np.histogram has it
    edges, lab = _time_labels([3, 3, 3], 2)
    assert np.array_equal(edges, np.histogram([3, 3, 3], 2)[1]) and np.array_equal(lab, [1, 1, 1])
    with pytest.raises(ValueError):
        _time_labels([np.nan, np.inf], 3)
    with pytest.raises(ValueError):
        _time_labels(t, 0)
    with pytest.raises(ValueError):
        _time_labels(t, [3.0, 2.0, 4.0])
    with pytest.raises(ValueError):
        _time_labels(t, [1.0, np.nan])
    with pytest.raises(RuntimeError):
        _time_labels(t, [1.0])
    with pytest.raises(RuntimeError):
        _time_labels(t.reshape(2, -1), 3)
    with pytest.raises(TypeError):
        _time_labels(t, 2.5)
    with pytest.raises(TypeError):
        _time_labels(["a", "b"], 2)


# -- the library -----------------------------------------------------------------------------------------
def test_effects_entry_points_are_exported(hip_lib):
    from trlda_amd import _ffi
    names = ["trlda_docindex_" + n for n in ("group_moments", "regress_products", "regress_residuals")]
    for name in names:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    # (no index: the argument check answers before any device is touched)
    f, i = np.full(8, -7.0), np.full(8, -7, dtype=np.int64)
    lab = np.zeros(4, dtype=np.int32)
    p = f.ctypes.data
    assert hip_lib.trlda_docindex_group_moments(None, lab.ctypes.data, 1, None, p, p, i.ctypes.data, p) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_group_moments(None, None, 1, None, None, None, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_regress_products(None, p, 1, None, p, p) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_regress_products(None, None, 1, None, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_regress_residuals(None, p, 1, None, p, p) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_regress_residuals(None, None, 1, None, None, None) == _ffi.ERR_ARG
    assert np.all(f == -7.0) and np.all(i == -7)


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
    lab = np.array([0, 1, -1, 1, 0])
    X = np.arange(10.0).reshape(5, 2) ** 2
    # group_prevalence
    for bad in (lab.astype(np.float64), "01011", None, [0.5] * 5):
        with pytest.raises(TypeError):
            x.group_prevalence(bad)
    for bad in (lab[:4], lab.reshape(5, 1), np.zeros(6, dtype=int)):
        with pytest.raises(RuntimeError, match="labels"):
            x.group_prevalence(bad)
    with pytest.raises(RuntimeError, match="empty"):
        _Shell(0).group_prevalence(np.zeros(0, dtype=int))
    for groups in (0, -1, 4096):
        with pytest.raises(RuntimeError, match="num_groups"):
            x.group_prevalence(lab, num_groups=groups)
    with pytest.raises(RuntimeError, match="num_groups"):
        x.group_prevalence(np.array([0, 1, 2, 3, 4095]))
    with pytest.raises(TypeError):
        x.group_prevalence(lab, num_groups=2.5)
    for bad in (np.array([0, 1, -2, 1, 0]), np.array([0, 1, 2, 1, 0])):
        with pytest.raises(ValueError, match="labels"):
            x.group_prevalence(bad, num_groups=2)
    for call in (lambda w: x.group_prevalence(lab, weights=w), lambda w: x.topic_effects(X, weights=w),
                 lambda w: x.topic_trends(np.arange(5.0), 2, weights=w)):
        for bad in ([1.0, 2.0, np.nan, 1.0, 1.0], [1.0, -1.0, 1.0, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0, 1.0], np.zeros(5)):
            with pytest.raises(ValueError, match="weights"):
                call(bad)
        for bad in (np.ones(4), np.ones((5, 1))):
            with pytest.raises(RuntimeError, match="weights"):
                call(bad)
        with pytest.raises(TypeError):
            call("heavy")
    # topic_trends
    with pytest.raises(RuntimeError):
        x.topic_trends(np.arange(4.0), 2)
    with pytest.raises(ValueError):
        x.topic_trends(np.full(5, np.nan), 2)
    with pytest.raises(RuntimeError, match="num_groups"):
        x.topic_trends(np.arange(5.0), 4096)
    # topic_effects
    for bad in (None, "abc", [["a", "b"]] * 5):
        with pytest.raises(TypeError):
            x.topic_effects(bad)
    for bad in (X[:4], X.reshape(5, 2, 1), np.zeros((5, 256)), np.float64(3.0)):
        with pytest.raises(RuntimeError):
            x.topic_effects(bad)
    with pytest.raises(RuntimeError):
        x.topic_effects(np.zeros((5, 0)), intercept=False)
    with pytest.raises(RuntimeError, match="empty"):
        _Shell(0).topic_effects(np.zeros((0, 2)))
    for bad in (np.nan, np.inf):
        Y = X.copy()
        Y[2, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            x.topic_effects(Y)
    with pytest.raises(ValueError, match="rank deficient"):
        x.topic_effects(np.arange(25.0).reshape(5, 5))                    # N < P'
    with pytest.raises(ValueError, match="rank deficient"):
        x.topic_effects(X, weights=[1.0, 1.0, 0.0, 0.0, 0.0])              # ... of the rows that count
    # what passes the checks reaches the index, which is closed
    for call in (lambda: x.group_prevalence(lab), lambda: x.group_prevalence(lab, np.ones(5), 7, True, 0),
                 lambda: x.topic_trends(np.arange(5.0), 2), lambda: x.topic_trends([1, 2, np.nan, 4, 9], [0.0, 3.0, 5.0]),
                 lambda: x.topic_effects(X), lambda: x.topic_effects(X[:, 0], intercept=False),
                 lambda: x.topic_effects(np.zeros((5, 0))), lambda: x.topic_effects(X, weights=np.arange(5.0))):
        with pytest.raises(RuntimeError, match="closed"):
            call()


def test_effects_kernels_do_not_spill(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    mine = {k: v for k, v in res.items() if "effects_" in k}
    # group<false>, group<true>, group_finish, products, products_finish, residual, residual_finish
    assert len(mine) == 7, sorted(mine)
    for part, count in (("group_kernel", 2), ("group_finish", 1), ("products_kernel", 1), ("products_finish", 1),
                        ("residual_kernel", 1), ("residual_finish", 1)):
        assert sum("effects_" + part in k for k in mine) == count, (part, sorted(mine))
    for name, f in mine.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_spill_count"] == 0, (name, f)
        assert f["sgpr_spill_count"] == 0, (name, f)
        assert f["vgpr_count"] <= 256, (name, f)
        assert f["group_segment_fixed_size"] <= 64 * 1024, (name, f)
    # the pins of the kernels this feature leans on hold: it adds no kernel of theirs
    assert sum("topicdocs_" in k for k in res) == 6 and not any("cluster_" in k for k in mine)
