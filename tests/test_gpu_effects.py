"""Topic prevalence against document metadata on the GPU (csrc/effects_kernels.h):
``DocumentIndex.group_prevalence``, ``topic_trends`` and ``topic_effects`` of both measures against the
restatement (tests/effects_host.py) of the device's own rows: the group passes bit for bit and within
their bounds of the longdouble sums, their independence of the other groups, the numbering, the slab and
the way the index was filled; the Gram matrix and the cross products within the scatter's bound, an
exact case in which every sum is exact whatever order the matrix core adds in, the closing arithmetic,
the residuals within a first-order rounding bound, the coefficients against lstsq; the model's state,
the buffers and the errors.

Every array is small: at most 300 indexed documents (1100 once, at K = 8, to cross the growth copy),
513 topics and 256 design columns.  The observed shares of the bounds are printed by each test and
recorded in DESIGN.md 3.34."""
import os
import subprocess
import sys

import numpy as np
import pytest

import effects_host as eh
import topicdocs_host as th

pytestmark = pytest.mark.gpu

U = eh.U
LD = np.longdouble
MEASURES = ["hellinger", "cosine"]
N_MAX = 300
COND_MAX = 1e4
GROUP_SHAPES = [(K, N_MAX) for K in (1, 3, 16, 17, 63, 65, 130, 513)] + [(17, N) for N in (1, 2, 3, 5, 31, 33, 65)]
PRODUCT_SHAPES = ([(P, 17, N_MAX) for P in (1, 2, 3, 5, 16, 17, 63, 64, 65, 129, 256)] +
                  [(5, K, N_MAX) for K in (1, 3, 16, 63, 65, 130)] +
                  [(2, 17, 3), (3, 17, 5), (5, 17, 31), (16, 17, 33), (17, 17, 65)])
CLOSING_SHAPES = [(1, 17, N_MAX), (2, 17, 3), (5, 1, N_MAX), (5, 65, N_MAX), (17, 17, 65), (65, 17, N_MAX),
                  (129, 130, N_MAX)]


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


def _filled(m, measure, g, step=None):
    ix = m.document_index(measure)
    step = g.shape[1] if step is None else step
    for c0 in range(0, g.shape[1], step):
        ix.add_gamma(np.asfortranarray(g[:, c0:c0 + step]))
    return ix


def _state():
    from trlda_amd import _ffi
    s = np.zeros(33, dtype=np.uint32)
    _ffi.lib().trlda_rng_get_state(s)
    return s


def _weights(N, seed=5, zeros=True):
    w = np.random.RandomState(seed).uniform(0.5, 30.0, size=N)
    if zeros:
        w[3::11] = 0.0
    return w


def _labels(N, big):
    """Five groups over scattered ids: group 0 of min(big, N // 2) members, group 1 empty, group 2 of one
    member (from N = 3), group 3 the rest but for the documents left out (-1, about one in six)."""
    order = np.random.RandomState(9 * N + big).permutation(N)
    lab = np.full(N, 3, dtype=np.int64)
    b = min(big, N // 2)
    lab[order[:b]] = 0
    rest = order[b:]
    if len(rest) > 1:
        lab[rest[0]] = 2
    lab[rest[2::6]] = -1
    return lab


def _bigs(N):
    return (255, 256, 257) if N == N_MAX else (N // 2,)


def _group_raw(hip, ix, labels, G, w=None, want_ss=True):
    """(mean K x G, wsum G, counts G, ss K x G) straight from the library."""
    from trlda_amd import _ffi
    K = ix._K
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    mean, ss = np.empty((K, G), order="F"), np.empty((K, G), order="F")
    wsum, counts = np.empty(G), np.empty(G, dtype=np.int64)
    _ffi.check(hip.trlda_docindex_group_moments(ix._handle, lab.ctypes.data, G, None if w is None else w.ctypes.data,
                                                mean.ctypes.data, wsum.ctypes.data, counts.ctypes.data,
                                                ss.ctypes.data if want_ss else None))
    return mean, wsum, counts, ss


def _products_raw(hip, ix, Z, w=None):
    from trlda_amd import _ffi
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    P = Z.shape[1]
    gram, cross = np.empty((P, P)), np.empty((P, ix._K))
    _ffi.check(hip.trlda_docindex_regress_products(ix._handle, Z.ctypes.data, P, None if w is None else w.ctypes.data,
                                                   gram.ctypes.data, cross.ctypes.data))
    return gram, cross


def _residuals_raw(hip, ix, Z, coef, w=None):
    from trlda_amd import _ffi
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    rows = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).T)
    rss = np.empty(ix._K)
    _ffi.check(hip.trlda_docindex_regress_residuals(ix._handle, Z.ctypes.data, Z.shape[1],
                                                    None if w is None else w.ctypes.data, rows.ctypes.data,
                                                    rss.ctypes.data))
    return rss


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _chunk(N):
    """Rows per chunk that cut N into at least five chunks (N chunks below 5) with a ragged last."""
    return max(1, (N - 1) // 5)


# 1. the group passes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K,N", GROUP_SHAPES)
def test_group_passes(hip, K, N, measure):
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    theta = eh.theta_hat(ix.rows(), measure)
    G = 5
    shares = [0.0, 0.0]
    for big in _bigs(N):
        labels = _labels(N, big)
        for w in (None, _weights(N)):
            mean, counts, var = ix.group_prevalence(labels, weights=w, num_groups=G, return_variance=True)
            assert mean.shape == var.shape == (K, G) and mean.flags.f_contiguous and var.flags.f_contiguous
            assert mean.dtype == var.dtype == np.float64 and counts.dtype == np.int64 and counts.shape == (G,)
            want = eh.group_prevalence(theta, labels, G, w)
            assert np.array_equal(counts, want[1]) and counts[1] == 0
            assert np.array_equal(mean, want[0], equal_nan=True)
            assert np.array_equal(var, want[2], equal_nan=True)
            assert np.all(np.isnan(mean[:, 1])) and np.all(np.isnan(var[:, 1]))
            assert _same(ix.group_prevalence(labels, weights=w, num_groups=G), (mean, counts))
            # against longdouble
            raw_mean, wsum, raw_counts, ss = _group_raw(hip, ix, labels, G, w)
            assert np.array_equal(raw_mean, mean, equal_nan=True) and np.array_equal(raw_counts, counts)
            exact, A, _, _, W, n = eh.group_exact(theta, labels, G, w)
            live = W > 0
            assert np.array_equal(np.isnan(mean[0]), ~live)
            assert np.all(np.abs(wsum.astype(LD) - W) <= (n + 16) * U * W.astype(np.float64))
            err, bound = np.abs(mean.astype(LD) - exact).astype(np.float64)[:, live], eh.group_mean_bound(A, n)[:, live]
            assert np.all(err <= bound), float(np.max(err / bound))
            shares[0] = max(shares[0], float(np.max(err / bound)))
            # the sums of squares about the device's own mean: the mean's error is tested once, above
            _, _, SS, B, _, _ = eh.group_exact(theta, labels, G, w, centre=np.nan_to_num(mean))
            err, bound = np.abs(ss.astype(LD) - SS).astype(np.float64)[:, live], eh.group_ss_bound(B, n)[:, live]
            assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))
            shares[1] = max(shares[1], float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(ss[:, live] >= 0)
            if N >= 3:
                assert counts[2] == 1 and (w is not None or np.all(ss[:, 2] == 0.0))
                one = int(np.flatnonzero(labels == 2)[0])
                if w is None or w[one] > 0:
                    assert np.array_equal(mean[:, 2], theta[one] if w is None else (w[one] * theta[one]) / w[one])
    print("K = %d N = %d %s: mean err / bound %.2e, SS err / bound %.2e" % (K, N, measure, shares[0], shares[1]))
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_a_group_depends_on_its_members_alone(hip, measure):
    K, N, G = 17, N_MAX, 5
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    labels = _labels(N, 257)
    for w in (None, _weights(N)):
        base = ix.group_prevalence(labels, weights=w, num_groups=G, return_variance=True)
        # the groups renumbered: the columns move with them
        perm = np.array([3, 0, 4, 1, 2])
        moved = np.where(labels >= 0, perm[np.maximum(labels, 0)], -1)
        got = ix.group_prevalence(moved, weights=w, num_groups=G, return_variance=True)
        assert _same([a[..., perm] for a in got], base)
        # more groups than labels
        got = ix.group_prevalence(labels, weights=w, num_groups=G + 9, return_variance=True)
        assert _same([a[..., :G] for a in got], base) and np.all(got[1][G:] == 0) and np.all(np.isnan(got[0][:, G:]))
        assert _same(ix.group_prevalence(labels, weights=w, return_variance=True), [a[..., :4] for a in base])
        # the other groups left out
        for g in (0, 3):
            got = ix.group_prevalence(np.where(labels == g, 0, -1), weights=w, return_variance=True)
            assert _same([a[..., 0] for a in got], [a[..., g] for a in base])
        ix.set_slab_rows(16)
        assert _same(ix.group_prevalence(labels, weights=w, num_groups=G, return_variance=True), base)
        ix.set_slab_rows(0)
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_results_do_not_depend_on_how_the_index_was_filled(hip, measure):
    """1100 documents at K = 8, added 1, 7 and 64 at a time: the table grows past its first 1024 rows."""
    K, N, G = 8, 1100, 4
    g = _gammas(K, N, 88)
    rng = np.random.RandomState(3)
    labels = rng.randint(-1, G, size=N)
    labels[:900] = np.where(labels[:900] > 0, 0, labels[:900])           # group 0: three chunks
    w = _weights(N)
    X = rng.normal(size=(N, 4))
    m = _model(K)
    results = []
    for step in (1, 7, 64):
        ix = _filled(m, measure, g, step)
        assert len(ix) == N
        got = list(ix.group_prevalence(labels, weights=w, return_variance=True))
        got += list(ix.group_prevalence(labels, return_variance=True))
        out = ix.topic_effects(X, weights=w)
        got += [out[k] for k in ("gram", "coef", "rss", "tss", "stderr", "r2")]
        got += list(_products_raw(hip, ix, eh.design(X)))
        results.append(got)
        ix.close()
    assert np.bincount(labels[labels >= 0])[0] > 2 * eh.CHUNK
    assert _same(results[1], results[0]) and _same(results[2], results[0])
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_trends_are_the_groups_of_the_time_labels(hip, measure):
    from trlda_amd.index import _time_labels
    K, N = 16, 120
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    t = np.random.RandomState(12).uniform(1990.0, 2020.0, size=N)
    t[[4, 50]] = [np.nan, np.inf]
    w = _weights(N)
    for bins in (6, np.array([1995.0, 2000.0, 2001.0, 2015.0])):
        edges, lab = _time_labels(t, bins)
        for weights in (None, w):
            got = ix.topic_trends(t, bins, weights=weights, return_variance=True)
            assert np.array_equal(got[0], edges) and got[1].shape == (K, len(edges) - 1)
            assert _same(got[1:], ix.group_prevalence(lab, weights=weights, num_groups=len(edges) - 1,
                                                      return_variance=True))
            assert _same(ix.topic_trends(t, bins, weights=weights), got[:3])
        assert np.array_equal(got[2], np.histogram(t[np.isfinite(t)], edges)[0])
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_one_group_is_the_covariance(hip, measure):
    """Without weights and with every document in one group the mean and the variance are those of
    topic_covariance, each side within its own bound of the longdouble figure."""
    K, N = 17, N_MAX
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    theta = eh.theta_hat(ix.rows(), measure)
    mean, counts, var = ix.group_prevalence(np.zeros(N, dtype=int), return_variance=True)
    cov, cmean = ix.topic_covariance(return_mean=True)
    _, A, SS, B, _, n = eh.group_exact(theta, np.zeros(N, dtype=int), 1)
    mb = eh.group_mean_bound(A, n)[:, 0] + (N + 16) * 2 * U * np.abs(theta).sum(axis=0) / N
    assert counts[0] == N and np.all(np.abs(mean[:, 0] - cmean) <= mb), np.max(np.abs(mean[:, 0] - cmean) / mb)
    # the two sums of squares are about the two device means: S(c) = S(m) + N (m - c)^2
    _, Ad = th.scatter(theta, cmean)
    vb = (eh.group_ss_bound(B, n)[:, 0] + (N + 16) * 4 * U * np.diag(Ad).astype(np.float64) + 2 * N * mb * mb) / (N - 1)
    vb = vb + 4 * U * np.diag(cov)
    assert np.all(np.abs(var[:, 0] - np.diag(cov)) <= vb), np.max(np.abs(var[:, 0] - np.diag(cov)) / vb)
    print("%s: one group against topic_covariance: mean %.2e, variance %.2e of the summed bounds"
          % (measure, np.max(np.abs(mean[:, 0] - cmean) / mb), np.max(np.abs(var[:, 0] - np.diag(cov)) / vb)))
    m.close()


# 2. the products ---------------------------------------------------------------------------------------
def _covariates(N, P, seed=None):
    return np.random.RandomState(700 + P if seed is None else seed).normal(size=(N, P - 1))


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("P,K,N", PRODUCT_SHAPES)
def test_products(hip, P, K, N, measure):
    g = _case(K, N)
    m = _model(K)
    ix = _filled(m, measure, g)
    theta = eh.theta_hat(ix.rows(), measure)
    Z = eh.design(_covariates(N, P))
    other = _filled(m, measure, g, 64)
    shares = []
    for w in (None, _weights(N, zeros=False)):
        want_G, AG, want_C, AC = eh.products(theta, Z, w)
        cond = np.linalg.cond(eh.equilibrated(want_G.astype(np.float64))[0])
        assert cond <= COND_MAX, cond
        bG, bC = eh.products_bound(AG, N), eh.products_bound(AC, N)
        gram, cross = _products_raw(hip, ix, Z, w)
        assert gram.shape == (P, P) and cross.shape == (P, K)
        assert np.array_equal(gram, gram.T)
        again = _products_raw(hip, ix, Z, w)
        assert np.array_equal(again[0], gram) and np.array_equal(again[1], cross)
        assert _same(_products_raw(hip, other, Z, w), (gram, cross))
        ix.set_slab_rows(16)
        assert _same(_products_raw(hip, ix, Z, w), (gram, cross))
        ix.set_slab_rows(0)
        for rows in (0, _chunk(N)):
            ix.set_moment_chunk(rows)
            gc, cc = _products_raw(hip, ix, Z, w)
            eG = np.abs(gc.astype(LD) - want_G).astype(np.float64)
            eC = np.abs(cc.astype(LD) - want_C).astype(np.float64)
            assert np.all(eG <= bG), (rows, float(np.max(eG / bG)))
            assert np.all(eC <= bC), (rows, float(np.max(eC / bC)))
            assert np.array_equal(gc, gc.T)
            shares.append(max(float(np.max(eG / bG)), float(np.max(eC / bC))))
        ix.set_moment_chunk(0)
        if w is None:
            assert gram[0, 0] == float(N)                    # the intercept's square: N ones
    print("P' = %d K = %d N = %d %s: err / bound %.2e (automatic chunk) %.2e (chunks of %d); weighted %.2e %.2e; "
          "cond %.0f" % (P, K, N, measure, shares[0], shares[1], _chunk(N), shares[2], shares[3], cond))
    m.close()


def _squares(K):
    """a (K integers >= 1) with sum a^2 = 4^m: theta = a^2 / 4^m is the square of the dyadic a / 2^m."""
    m = 1
    while 4 ** m < K:
        m += 1
    rest = 4 ** m - K                                       # raising a 1 to a adds a^2 - 1
    steps = [a * a - 1 for a in range(2, 2 ** m + 1)]
    best = {0: []}
    for total in range(1, rest + 1):
        for s in steps:
            if s <= total and total - s in best and len(best[total - s]) < K:
                best[total] = best[total - s] + [s]
                break
    a = np.ones(K, dtype=np.int64)
    for i, s in enumerate(best[rest]):                      # (every K used here has such a sum)
        a[i] = int(round(np.sqrt(s + 1)))
    return a, m


@pytest.mark.parametrize("P,K", [(3, 5), (65, 65), (17, 130), (256, 17)])
def test_an_exact_case(hip, P, K):
    """gamma columns are rotations of a pattern such as (9, 1, 4, 1, 1), whose theta are squares of dyadics;
    X holds integers in [-2, 2] and the weights integers in [0, 3]: every product and every partial sum is
    an integer multiple of a power of two well below 2^53 times it, so every sum is exact in fp64 whatever
    order it is added in, and the device's figures equal integer arithmetic.  This pins the tile, chunk
    and padding edges."""
    N = N_MAX
    a, mexp = _squares(K)
    scale = 4 ** mexp
    assert int((a * a).sum()) == scale and a.min() >= 1
    rng = np.random.RandomState(100 + K)
    asq = np.stack([np.roll(a * a, int(s)) for s in rng.randint(0, K, size=N)])      # N x K integers
    m = _model(K)
    ix = _filled(m, "hellinger", np.asfortranarray(asq.T.astype(np.float64)))
    theta = asq / float(scale)
    assert np.array_equal(ix.rows() ** 2, theta)
    Zi = np.hstack([np.ones((N, 1), dtype=np.int64), rng.randint(-2, 3, size=(N, P - 1))])
    wi = rng.randint(0, 4, size=N)
    Z = Zi.astype(np.float64)
    for w in (None, wi.astype(np.float64)):
        wz = Zi if w is None else wi[:, None] * Zi
        for rows in (0, _chunk(N), 64):
            ix.set_moment_chunk(rows)
            gram, cross = _products_raw(hip, ix, Z, w)
            assert np.array_equal(gram, (wz.T.dot(Zi)).astype(np.float64))
            assert np.array_equal(cross, wz.T.dot(asq) / float(scale))
        ix.set_moment_chunk(0)
        # coefficients in eighths: fit, the residual, its square and the sums are exact
        bi = rng.randint(-4, 5, size=(P, K))
        bi[:, 0] = 0                                         # (a topic whose fit is nothing)
        r = 8 * asq - scale * Zi.dot(bi)                     # (8 4^m) (theta - fit), integers
        want = ((1 if w is None else wi[:, None]) * r * r).sum(axis=0)
        assert want.max() < 2 ** 53
        rss = _residuals_raw(hip, ix, Z, bi / 8.0, w)
        assert np.array_equal(rss, want / float(64 * scale * scale))
        assert np.array_equal(_residuals_raw(hip, ix, Z, bi / 8.0, w), rss)
    m.close()


# 3. the closing arithmetic and the residuals -----------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("P,K,N", CLOSING_SHAPES)
def test_effects(hip, P, K, N, measure):
    from trlda_amd.index import _effects_closing
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    theta = eh.theta_hat(ix.rows(), measure)
    X = _covariates(N, P)
    Z = eh.design(X)
    notes = []
    for w in (None, _weights(N, zeros=N > 2 * P)):
        out = ix.topic_effects(X, weights=w)
        nobs = N if w is None else int(np.count_nonzero(w > 0))
        assert out["nobs"] == nobs and out["dof"] == nobs - P
        assert out["coef"].shape == out["stderr"].shape == out["tvalues"].shape == (P, K)
        assert out["rss"].shape == out["tss"].shape == out["r2"].shape == out["sigma2"].shape == (K,)
        assert out["gram"].shape == out["cov_unscaled"].shape == (P, P)
        # the closing arithmetic: bitwise that of the device's own sums
        gram, cross = _products_raw(hip, ix, Z, w)
        assert np.array_equal(out["gram"], gram)
        want = _effects_closing(gram, cross, out["rss"], out["tss"], nobs, True)
        for key in ("coef", "stderr", "tvalues", "r2", "sigma2", "cov_unscaled"):
            assert np.array_equal(out[key], want[key], equal_nan=True), key
        assert np.array_equal(out["rss"], _residuals_raw(hip, ix, Z, out["coef"], w))
        if out["dof"] <= 0:
            assert np.all(np.isnan(out["stderr"])) and np.all(np.isnan(out["tvalues"]))
        else:
            assert np.all(np.isfinite(out["stderr"]))
        # the residuals: explicit, within the first-order bound (effects_host.rss_bound)
        rss, E = eh.residuals(theta, Z, out["coef"], w)
        err = np.abs(out["rss"].astype(LD) - rss).astype(np.float64)
        assert np.all(err <= E), float(np.max(err / np.maximum(E, 1e-300)))
        means = (cross[0] / gram[0, 0])[None, :]
        tss, Et = eh.residuals(theta, np.ones((N, 1)), means, w)
        terr = np.abs(out["tss"].astype(LD) - tss).astype(np.float64)
        assert np.all(terr <= Et), float(np.max(terr / np.maximum(Et, 1e-300)))
        assert np.all(out["rss"] >= 0) and np.all(out["rss"] <= out["tss"] * (1 + 1e-12) + E)
        # the coefficients: against float64 lstsq, in the equilibrated coordinates
        want_G, AG, want_C, AC = eh.products(theta, Z, w)
        A, d = eh.equilibrated(want_G.astype(np.float64))
        cond = np.linalg.cond(A)
        assert cond <= COND_MAX, cond
        tol = eh.coef_bound(want_G.astype(np.float64), eh.products_bound(AG, N), eh.products_bound(AC, N),
                            out["coef"], COND_MAX)
        ref = eh.lstsq(theta, Z, w)[0]
        cerr = np.linalg.norm((out["coef"] - ref) / d[:, None], axis=0)
        assert np.all(cerr <= tol), float(np.max(cerr / tol))
        # sum_k theta^_dk = 1 + eps_d: the rows of coef sum to (1, 0, ..., 0) + the regression of eps on Z,
        # which in the equilibrated coordinates is at most sqrt(P W) max |eps| / lambda_min
        eps = float(np.max(np.abs(theta.astype(LD).sum(axis=1) - 1)))
        lam_max = float(np.linalg.eigvalsh(A)[-1])
        stol = tol.sum() + COND_MAX / lam_max * np.sqrt(P * want_G[0, 0].astype(np.float64)) * (eps + 4 * U)
        target = np.zeros(P)
        target[0] = 1.0
        serr = np.linalg.norm((out["coef"].sum(axis=1) - target) / d)
        assert serr <= stol, serr / stol
        notes.append("rss %.2e tss %.2e coef %.2e sums %.2e cond %.0f"
                     % (float(np.max(err / np.maximum(E, 1e-300))), float(np.max(terr / np.maximum(Et, 1e-300))),
                        float(np.max(cerr / tol)), serr / stol, cond))
    print("P' = %d K = %d N = %d %s: shares of the bounds: %s; weighted %s" % (P, K, N, measure, notes[0], notes[1]))
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_one_hot_groups_are_the_group_means(hip, measure):
    K, N, G = 17, N_MAX, 4
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    theta = eh.theta_hat(ix.rows(), measure)
    labels = np.random.RandomState(8).randint(0, G, size=N)
    Z = (labels[:, None] == np.arange(G)[None, :]).astype(np.float64)
    for w in (None, _weights(N)):
        out = ix.topic_effects(Z, weights=w, intercept=False)
        assert "tss" not in out and "r2" not in out
        mean, counts = ix.group_prevalence(labels, weights=w)
        # coef_gk = C_gk / G_gg (the equilibrated Gram matrix is the identity): each side within its bound
        want_G, AG, want_C, AC = eh.products(theta, Z, w)
        Gd = np.diag(want_G).astype(np.float64)[:, None]
        _, A, _, _, _, n = eh.group_exact(theta, labels, G, w)
        bound = (eh.products_bound(AC, N) + eh.products_bound(np.diag(AG), N)[:, None] * np.abs(mean.T)) / Gd
        bound = bound + eh.group_mean_bound(A, n).T + 8 * U * np.abs(mean.T)
        err = np.abs(out["coef"] - mean.T)
        assert np.all(err <= bound), float(np.max(err / bound))
        # rss: the within-group sums of squares about those means
        ss = _group_raw(hip, ix, labels, G, w)[3]
        rss, E = eh.residuals(theta, Z, out["coef"], w)
        assert np.all(np.abs(out["rss"].astype(LD) - rss) <= E)
        assert np.all(np.abs(out["rss"] - ss.sum(axis=1)) <= 1e-12 * out["rss"])
    m.close()


# 4. the model's state, the buffers, the errors -----------------------------------------------------------
def test_state_is_left_alone(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K, N = 16, 40
    m = _model(K, alpha=.2, eta=.05)
    ix = _filled(m, "cosine", _case(K, N))
    rows = ix.rows()
    # an E-step first, so that the model's statistics are not trivial
    rng = np.random.RandomState(31)
    docs = [[(int(w), int(rng.randint(1, 5))) for w in rng.choice(8, size=rng.randint(2, 7), replace=False)]
            for _ in range(9)]
    latents = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 9)) + 0.1)
    gamma0, sstats = m.update_variables(docs, latents=latents.copy(order="F"), max_iter=20)
    held = np.empty((K, 8), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, held))
    assert np.array_equal(held, sstats) and np.any(held > 0)
    before = (np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count)
    labels = np.arange(N) % 3 - 1
    X = rng.normal(size=(N, 2))
    w = _weights(N)
    kept = (labels.copy(), X.copy(), w.copy())
    trlda_amd.seed(9)
    state = _state()
    ix.group_prevalence(labels, weights=w, return_variance=True)
    ix.topic_trends(X[:, 0], 4)
    ix.topic_effects(X, weights=w)
    ix.set_moment_chunk(8)
    ix.topic_effects(X, intercept=False)
    ix.set_moment_chunk(0)
    assert np.array_equal(state, _state())
    assert np.array_equal(labels, kept[0]) and np.array_equal(X, kept[1]) and np.array_equal(w, kept[2])
    assert len(ix) == N and np.array_equal(ix.rows(), rows)
    assert np.array_equal(np.asarray(m.lambdas), before[0]) and np.array_equal(np.asarray(m.alpha), before[1])
    assert m.eta == before[2] and m.update_count == before[3]
    after_stats = np.empty((K, 8), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, after_stats))
    assert np.array_equal(after_stats, held)                      # the model's statistics: no E-step ran
    # the same E-step after the calls: the same bits
    gamma1, sstats1 = m.update_variables(docs, latents=latents.copy(order="F"), max_iter=20)
    assert np.array_equal(gamma1, gamma0) and np.array_equal(sstats1, sstats)
    m.close()


def test_no_buffer_is_kept_by_the_calls(hip):
    """A fresh process (the count is the process's): the calls, the refused ones included, leave the
    live count as it was, and after close() the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "effects_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout


def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K, N, G, P = 8, 12, 3, 2
    m = _model(K)
    ix = m.document_index("cosine")
    trlda_amd.seed(3)
    before = _state()
    f = np.full(K * 4096, -7.0)
    cnt = np.full(4096, -7, dtype=np.int64)
    lab = (np.arange(N) % G).astype(np.int32)
    Z = np.ascontiguousarray(eh.design(np.arange(N, dtype=np.float64)))
    w = np.ones(N)
    b = np.zeros((K, P))
    p, null = f.ctypes.data, None

    def groups(labels, groups_, weights, mean=p, wsum=p, counts=cnt.ctypes.data, index=ix):
        return hip.trlda_docindex_group_moments(index._handle, labels, groups_, weights, mean, wsum, counts, p)

    def products(z, cols, weights, gram=p, cross=p):
        return hip.trlda_docindex_regress_products(ix._handle, z, cols, weights, gram, cross)

    def residuals(z, cols, weights, coef, rss=p):
        return hip.trlda_docindex_regress_residuals(ix._handle, z, cols, weights, coef, rss)

    # an empty index
    assert groups(lab.ctypes.data, G, null) == _ffi.ERR_ARG
    assert products(Z.ctypes.data, P, null) == _ffi.ERR_ARG
    assert residuals(Z.ctypes.data, P, null, b.ctypes.data) == _ffi.ERR_ARG
    with pytest.raises(RuntimeError, match="empty"):
        ix.group_prevalence(np.zeros(0, dtype=int))
    with pytest.raises(RuntimeError, match="empty"):
        ix.topic_effects(np.zeros((0, 1)))
    ix.add_gamma(_case(K, N))
    # NULL arguments, G and P out of range
    assert groups(null, G, null) == _ffi.ERR_ARG
    assert groups(lab.ctypes.data, G, null, mean=null) == _ffi.ERR_ARG
    assert groups(lab.ctypes.data, G, null, wsum=null) == _ffi.ERR_ARG
    assert groups(lab.ctypes.data, G, null, counts=null) == _ffi.ERR_ARG
    for bad in (0, -1, 4096):
        assert groups(lab.ctypes.data, bad, null) == _ffi.ERR_ARG
    assert products(null, P, null) == _ffi.ERR_ARG
    assert products(Z.ctypes.data, P, null, gram=null) == _ffi.ERR_ARG
    assert products(Z.ctypes.data, P, null, cross=null) == _ffi.ERR_ARG
    assert residuals(null, P, null, b.ctypes.data) == _ffi.ERR_ARG
    assert residuals(Z.ctypes.data, P, null, null) == _ffi.ERR_ARG
    assert residuals(Z.ctypes.data, P, null, b.ctypes.data, rss=null) == _ffi.ERR_ARG
    for bad in (0, -3, 257):
        assert products(Z.ctypes.data, bad, null) == _ffi.ERR_ARG
        assert residuals(Z.ctypes.data, bad, null, b.ctypes.data) == _ffi.ERR_ARG
    # values: labels, weights, the design, the coefficients
    for value in (-2, G):
        bad = lab.copy()
        bad[5] = value
        assert groups(bad.ctypes.data, G, null) == _ffi.ERR_VALUE
    for value in (-1.0, np.nan, np.inf):
        bad = w.copy()
        bad[7] = value
        assert groups(lab.ctypes.data, G, bad.ctypes.data) == _ffi.ERR_VALUE
        assert products(Z.ctypes.data, P, bad.ctypes.data) == _ffi.ERR_VALUE
        assert residuals(Z.ctypes.data, P, bad.ctypes.data, b.ctypes.data) == _ffi.ERR_VALUE
    for value in (np.nan, -np.inf):
        bad = Z.copy()
        bad[3, 1] = value
        assert products(bad.ctypes.data, P, null) == _ffi.ERR_VALUE
        assert residuals(bad.ctypes.data, P, null, b.ctypes.data) == _ffi.ERR_VALUE
        bad = b.copy()
        bad[2, 0] = value
        assert residuals(Z.ctypes.data, P, null, bad.ctypes.data) == _ffi.ERR_VALUE
    # the Python forms
    with pytest.raises(TypeError):
        ix.group_prevalence(lab.astype(np.float64))
    with pytest.raises(RuntimeError):
        ix.group_prevalence(lab[:-1])
    with pytest.raises(ValueError):
        ix.group_prevalence(lab, num_groups=2)
    with pytest.raises(ValueError):
        ix.group_prevalence(lab, weights=np.zeros(N))
    with pytest.raises(RuntimeError):
        ix.topic_effects(np.zeros((N + 1, 1)))
    with pytest.raises(ValueError, match="finite"):
        ix.topic_effects(np.full((N, 1), np.nan))
    with pytest.raises(ValueError, match="rank deficient"):
        ix.topic_effects(np.ones((N, 1)))                     # the intercept twice
    with pytest.raises(ValueError, match="rank deficient"):
        ix.topic_effects(np.zeros((N, 12)))                   # N < P'
    with pytest.raises(ValueError):
        ix.topic_trends(np.full(N, np.nan))
    # nothing was drawn or written
    assert len(ix) == N and np.array_equal(before, _state())
    assert np.all(f == -7.0) and np.all(cnt == -7)
    # the index still works after the refusals
    mean, counts = ix.group_prevalence(lab)
    assert np.array_equal(counts, [4, 4, 4]) and np.all(np.abs(mean.sum(axis=0) - 1) <= 1e-14)
    ix.close()
    for call in (lambda: ix.group_prevalence(lab), lambda: ix.topic_trends(np.arange(N)),
                 lambda: ix.topic_effects(np.arange(N, dtype=np.float64))):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    m.close()
