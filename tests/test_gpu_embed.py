"""The map of a DocumentIndex on the GPU (csrc/tsne_kernels.h): nearest_neighbors,
affinities, embedding_gradient and embed against the restatement (tests/embed_host.py) on the device's
own rows and values -- the neighbours' ids and similarities, the calibrated rows and their two limits,
every component of the gradient and the KL within the derived bounds, a five-step trajectory within 100
times the float64-vs-longdouble distance of the restatement, the planted groups end to end; the bitwise
invariances (slab width, row block, the way the index was filled, the tile knob, two calls); the model's
state, the buffers and the errors.

Every array is small: at most 1100 indexed documents and 65 topics.

Observed on the MI355X: similarities at most 1.2e-15 from the longdouble ones (bound 1.6e-14 at K = 65);
near ties only where the rows lie on a curve (K = 2: 183 and 391 rows over all shapes, their ids held
to their own similarities instead) and 1 row each at K = 3 and 17, cosine; calibrated p at most 5.4 % of
its bound, the entropy condition 11.5 %; the gradient at most 9.1 % of its bound (N = 3, exaggeration
12; 0.4 % at N = 1100), KL 1.3 %; the trajectories 0.5 % (N = 300, E = 8.1e-16) and 0.7 % (N = 65,
E = 9.7e-16) of the bar of 100 E."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import docindex_host as dh
import embed_host as eh
from test_gpu_docindex import GAP_FLOOR, _model, _state, sim_bound

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = eh.U
MEASURES = ["hellinger", "cosine"]
SIZES = [2, 3, 17, 64, 65, 300, 1100]


@pytest.fixture(scope="module")
def hip():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


def _live():
    from trlda_amd import _ffi
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return live.value


def _gammas(K, N, seed=0):
    """The groups-of-three corpus where K has room for it, sparse-ish random columns below."""
    if K >= 6:
        return eh.planted(N, 100 * K + N + seed, K)[0]
    rng = np.random.RandomState(100 * K + N + seed)
    return np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, N)) + 0.01)


def _filled(m, measure, g):
    ix = m.document_index(measure)
    ix.add_gamma(g)
    return ix


def _same(p, q):
    return len(p) == len(q) and all(v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes()
                                    for v, w in zip(p, q))


# 1. neighbours ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", [2, 3, 17, 65])
def test_neighbours_are_the_restatements(hip, K, measure):
    """Ids and similarities on the device's own rows.  A row whose ids differ from the restatement's
    must hold a near tie (a non-zero gap below GAP_FLOOR among its first top_n + 2): the report."""
    m = _model(K)
    near, worst = 0, 0.0
    for N in SIZES:
        ix = _filled(m, measure, _gammas(K, N))
        if N == 300:
            ix.set_slab_rows(64)
        ranked = eh.ranking(ix.rows())
        for top_n in sorted({1, min(N - 1, 10), min(N - 1, 99)}):
            want_ids, want_s, gap = eh.knn(None, top_n, ranked)
            ids, s = ix.nearest_neighbors(top_n, return_similarity=True, block_rows=128 if N == 300 else 0)
            assert ids.dtype == np.int64 and s.dtype == np.float64 and ids.shape == s.shape == (N, top_n)
            assert not np.any(ids == np.arange(N)[:, None])
            tied = gap <= GAP_FLOOR
            near += int(tied.sum())
            assert np.array_equal(ids[~tied], want_ids[~tied]), (N, top_n)
            err = float(np.max(np.abs(s.astype(LD) - want_s)))
            worst = max(worst, err)
            assert err <= sim_bound(K), (N, top_n, err)
            # (near ties included: every id stands beside its own similarity)
            own = np.take_along_axis(ranked[0], ids, axis=1)
            assert float(np.max(np.abs(s.astype(LD) - own))) <= sim_bound(K), (N, top_n)
            ids2, dist = ix.nearest_neighbors(top_n)
            assert np.array_equal(ids2, ids) and np.array_equal(dist, dh.distance(s, measure))
        ix.close()
    print("K = %d %s: max |s - longdouble| %.2e (bound %.2e), %d rows with a near tie"
          % (K, measure, worst, sim_bound(K), near))
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_duplicates_find_each_other(hip, measure):
    """12 identical documents among 40, top_n = 5: the duplicates of the seven largest ids do not find
    their own id among the first six (the fallback drops the last entry instead)."""
    K, N = 5, 40
    g = _gammas(K, N).copy(order="F")
    twins = np.arange(3, 39, 3)
    assert len(twins) == 12
    g[:, twins] = g[:, [3]]
    m = _model(K)
    ix = _filled(m, measure, g)
    ids, s = ix.nearest_neighbors(5, return_similarity=True)
    want_ids, want_s, _ = eh.knn(ix.rows(), 5)
    assert np.array_equal(ids, want_ids)
    for t in twins:
        assert list(ids[t]) == [u for u in twins if u != t][:5] and np.all(s[t] == s[t][0])
    # the tie limit of the calibration: 11 others at d = 0 exactly, perplexity 5
    cids, p, beta = ix.affinities(5.0, return_conditional=True)
    for t in twins:
        assert beta[t] == np.inf and np.array_equal(p[t], np.where(np.isin(cids[t], twins), 1.0 / 11, 0.0))
        assert np.sum(p[t] > 0) == 11
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_neighbours_do_not_depend_on_the_partition(hip, measure):
    K, N = 17, 300
    g = _gammas(K, N)
    m = _model(K)
    whole = _filled(m, measure, g)
    base = whole.nearest_neighbors(40, return_similarity=True)
    cond = whole.affinities(10.0, return_conditional=True)
    parts = m.document_index(measure)
    for a, b in ((0, 7), (7, 8), (8, 300)):
        parts.add_gamma(g[:, a:b])
    for ix in (whole, parts):
        for slab in (0, 64, 128):
            ix.set_slab_rows(slab)
            for block in (0, 1, 64, 100, 299):
                if block == 1 and slab:
                    continue
                assert _same(ix.nearest_neighbors(40, return_similarity=True, block_rows=block), base)
            assert _same(ix.affinities(10.0, return_conditional=True, block_rows=100), cond)
    m.close()


# 2. calibration --------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("perplexity", [1.0, 5.0, 10.0, 33.0])
def test_calibration(hip, perplexity, measure):
    K = 17
    m = _model(K)
    worst_p, worst_h = 0.0, 0.0
    for N in SIZES:
        ix = _filled(m, measure, _gammas(K, N, 1))
        k = min(N - 1, int(3 * perplexity))
        ids, p, beta = ix.affinities(perplexity, return_conditional=True)
        ids2, s = ix.nearest_neighbors(k, return_similarity=True)
        assert ids.shape == p.shape == (N, k) and beta.shape == (N,) and np.array_equal(ids, ids2)
        d = eh.offsets(eh.distances(s))
        target = np.log(LD(perplexity))
        for i in range(N):
            if np.log(k) <= np.log(perplexity):                           # the uniform limit
                assert beta[i] == 0 and np.array_equal(p[i], np.full(k, 1.0 / k))
                continue
            tied = d[i] == 0
            if tied.sum() >= perplexity:                                  # the tie limit (perplexity 1: m = 1)
                assert beta[i] == np.inf and np.array_equal(p[i], np.where(tied, 1.0 / tied.sum(), 0.0))
                continue
            assert 0 < beta[i] < np.inf
            di = d[i].astype(LD)
            H, w, S, _ = eh.entropy(LD(beta[i]), di)
            want = w / S
            big = want > 1e-290
            rel = np.abs(p[i][big].astype(LD) - want[big]) / want[big]
            bound = eh.p_bound(k, beta[i], d[i].max())
            worst_p = max(worst_p, float(rel.max() / bound))
            assert np.all(rel <= bound) and np.all(p[i][~big] <= 1e-289)
            slack = abs(float(eh.entropy_slope(LD(beta[i]), di))) * beta[i] * 2.0 ** -49
            hb = slack + eh.entropy_bound(k, beta[i], di)
            worst_h = max(worst_h, abs(float(H - target)) / hb)
            assert abs(float(H - target)) <= hb, (N, i)
        ix.close()
    print("perplexity %g %s: p at most %.3f of its bound, H at most %.3f of its bound"
          % (perplexity, measure, worst_p, worst_h))
    m.close()


def test_affinities_are_symmetric_and_sum_to_one(hip):
    K, N = 17, 300
    m = _model(K)
    ix = _filled(m, "hellinger", _gammas(K, N))
    indptr, ids, p = ix.affinities(10.0)
    cids, cp, _ = ix.affinities(10.0, return_conditional=True)
    P = eh.dense(indptr, ids, p)
    assert np.array_equal(P, P.T) and abs(P.sum() - 1.0) <= (2 * 30 + 64) * U
    assert np.array_equal(P, eh.symmetrise(cids, cp))
    for i in range(N):
        assert np.all(np.diff(ids[indptr[i]:indptr[i + 1]]) > 0)
    m.close()


# 3. gradient and KL ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,measure", [(2, 2, "hellinger"), (3, 3, "cosine"), (17, 17, "hellinger"),
                                         (64, 65, "cosine"), (65, 2, "hellinger"), (300, 17, "cosine"),
                                         (300, 3, "hellinger"), (1100, 65, "hellinger")])
def test_gradient_and_kl(hip, N, K, measure):
    m = _model(K)
    ix = _filled(m, measure, _gammas(K, N, 2))
    if N == 300:
        ix.set_slab_rows(64)
        ix.set_tsne_tile(64)
    aff = ix.affinities(10.0)
    P = eh.dense(*aff)
    rng = np.random.RandomState(N + K)
    for scale in (1e-4, 1.0, 30.0):
        Y = rng.normal(0.0, scale, size=(N, 2))
        for ex in (1.0, 12.0):
            grad, kl = ix.embedding_gradient(Y, aff, ex)
            want, want_kl, parts = eh.gradient(Y, P, ex, LD, parts=True)
            bound = eh.gradient_bound(N, parts, ex)
            err = np.abs(grad.astype(LD) - want).astype(np.float64)
            share = float(np.max(err / np.maximum(bound, 1e-300)))
            kb = eh.kl_bound(N, parts)
            print("N = %d K = %d scale %g ex %g: gradient at most %.3f of its bound, KL %.3f of its bound"
                  % (N, K, scale, ex, share, abs(float(kl - want_kl)) / kb))
            assert np.all(err <= bound)
            assert abs(float(kl - want_kl)) <= kb
        # twice, and across the tile knob: the same bits
        base = ix.embedding_gradient(Y, aff, 12.0)
        for tile in (64, 128, 1024, 0):
            ix.set_tsne_tile(tile)
            again = ix.embedding_gradient(Y, aff, 12.0)
            assert base[0].tobytes() == again[0].tobytes() and base[1] == again[1], tile
    # an all-equal map: no repulsion and no attraction, exactly
    grad, kl = ix.embedding_gradient(np.full((N, 2), 0.37), aff, 12.0)
    assert np.all(grad == 0.0)
    m.close()


# 4. trajectory ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", eh.TRAJECTORY_SIZES)
def test_trajectory(hip, N):
    """Five iterations across the end of the exaggeration and the momentum switch, from an explicit
    start.  E is the float64-vs-longdouble distance of the two restatements on the device's own
    affinities, relative to the extent of the map; the device must lie within 100 E of the longdouble
    trajectory, and its KL of every iteration within the KL bound plus what 100 E moves the KL by
    (sum |dKL/dY| times the bar).  Observed: 0.5 % of the bar at N = 300, 0.7 % at N = 65."""
    gamma, Y0 = eh.trajectory_case(N)
    m = _model(gamma.shape[0])
    ix = _filled(m, "hellinger", gamma)
    if N == 300:
        ix.set_slab_rows(64)
        ix.set_tsne_tile(64)
    aff = ix.affinities(eh.TRAJECTORY_PERPLEXITY)
    P = eh.dense(*aff)
    Y64, _, same64, _ = eh.loop(Y0, P, trace=True, **eh.TRAJECTORY)
    Yl, kll, samel, iterates = eh.loop(Y0, P, dtype=LD, trace=True, **eh.TRAJECTORY)
    for a, b in zip(same64, samel):
        assert np.array_equal(a, b)                                       # the gain decisions agree
    extent = float(np.max(np.abs(Yl)))
    E = float(np.max(np.abs(Y64 - Yl))) / extent
    Y, info = ix.embed(init=Y0, affinities=aff, return_info=True, **eh.TRAJECTORY)
    got = float(np.max(np.abs(Y.astype(LD) - Yl))) / extent
    print("N = %d: E = %.2e, the device %.2e of the extent: %.3f of the bar" % (N, E, got, got / (100 * E)))
    assert E > 0 and got <= 100 * E
    assert info["iterations"] == 5 and info["learning_rate"] == eh.learning_rate(N)
    for t in range(5):
        _, _, parts = eh.gradient(iterates[t], P, 1.0, LD, parts=True)
        g1 = eh.gradient(iterates[t], P, 1.0, LD)[0]
        carried = float(np.abs(g1).sum()) * 100 * E * float(np.max(np.abs(iterates[t])))
        assert abs(float(info["kl"][t] - kll[t])) <= eh.kl_bound(N, parts) + carried, t
    again = ix.embed(init=Y0, affinities=aff, **eh.TRAJECTORY)
    assert again.tobytes() == Y.tobytes()
    m.close()


# 5. end to end ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
def test_planted_groups_come_apart(hip, measure):
    N = 150
    gamma, group = eh.planted(N, 40 + N)
    m = _model(6)
    ix = _filled(m, measure, gamma)
    start = ix._pca_start(N)
    want = eh.pca_start(eh.theta_of(ix.rows(), measure))
    assert abs(start[:, 0].std() / 1e-4 - 1.0) < 1e-9 and np.max(np.abs(start - want)) < 1e-9 * 1e-4
    Y, info = ix.embed(perplexity=10.0, num_iterations=500, init="pca", return_info=True)
    purity, between, within = eh.separation(Y, group)
    print("%s: purity %.3f, centroids %.1f apart, members within %.1f, KL %.4f -> %.4f"
          % (measure, purity, between, within, info["kl"][250], info["kl"][-1]))
    assert Y.shape == (N, 2) and purity == 1.0 and between > 2 * within
    assert info["kl"].shape == (500,) and info["kl"][-1] < info["kl"][250]
    assert np.max(np.abs(Y.mean(axis=0))) < 1e-9
    m.close()


def test_one_and_two_documents(hip):
    m = _model(3)
    ix = _filled(m, "hellinger", _gammas(3, 1))
    assert np.array_equal(ix.embed(), np.zeros((1, 2)))
    indptr, ids, p = ix.affinities()
    assert list(indptr) == [0, 0] and len(ids) == len(p) == 0
    with pytest.raises(RuntimeError, match="top_n"):
        ix.nearest_neighbors(1)
    ix.add_gamma(_gammas(3, 1, 5))
    indptr, ids, p = ix.affinities()
    assert list(indptr) == [0, 1, 2] and list(ids) == [1, 0] and list(p) == [0.5, 0.5]
    Y = ix.embed(num_iterations=20)
    assert Y.shape == (2, 2) and np.all(np.isfinite(Y))
    m.close()


# 6. state, buffers and errors ------------------------------------------------------------------------
def test_state_is_left_alone(hip):
    import trlda_amd
    K, N = 16, 40
    rng = np.random.RandomState(31)
    docs = [[(int(w), int(rng.randint(1, 5))) for w in rng.choice(8, size=rng.randint(2, 7), replace=False)]
            for _ in range(9)]
    lat = [np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 9)) + 0.1) for _ in range(2)]
    g = _gammas(K, N)

    def run(with_map):
        m = _model(K)
        ix = _filled(m, "hellinger", g)
        out = list(m.update_variables(docs, latents=lat[0].copy(order="F"), max_iter=20))
        if with_map:
            ix.nearest_neighbors(3)                                      # (the query workspaces grow once)
            trlda_amd.seed(9)
            state, live, rows = _state(), _live(), ix.rows()
            before = (np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count)
            ix.embed(perplexity=5.0, num_iterations=12, exaggeration_iterations=4)
            ix.embedding_gradient(np.zeros((N, 2)), ix.affinities(3.0))
            ix.nearest_neighbors(3)
            assert np.array_equal(state, _state()) and _live() == live
            assert len(ix) == N and np.array_equal(ix.rows(), rows)
            assert np.array_equal(np.asarray(m.lambdas), before[0]) and np.array_equal(np.asarray(m.alpha), before[1])
            assert m.eta == before[2] and m.update_count == before[3]
        out += list(m.update_variables(docs, latents=lat[1].copy(order="F"), max_iter=20))
        m.close()
        return [np.asarray(a) for a in out]

    assert _same(run(True), run(False))


def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    K, N = 8, 12
    m = _model(K)
    ix = m.document_index("cosine")
    trlda_amd.seed(3)
    before, live = _state(), _live()
    for refused in (lambda: ix.nearest_neighbors(1), lambda: ix.affinities(), lambda: ix.embed(),
                    lambda: ix.embedding_gradient(np.zeros((0, 2)), (np.zeros(1, dtype=np.int64), [], []))):
        with pytest.raises(RuntimeError, match="empty"):
            refused()
    ix.add_gamma(_gammas(K, N))
    aff = ix.affinities(3.0)
    other = m.document_index("cosine")
    other.add_gamma(_gammas(K, N + 1))
    stale = other.affinities(3.0)
    live = _live()
    Y0 = np.random.RandomState(1).normal(size=(N, 2))
    for perplexity in (0.5, 33.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="perplexity"):
            ix.affinities(perplexity)
        with pytest.raises(ValueError, match="perplexity"):
            ix.embed(perplexity=perplexity)
    for top_n in (0, N, 100):
        with pytest.raises(RuntimeError, match="top_n"):
            ix.nearest_neighbors(top_n)
    bad = Y0.copy()
    bad[3, 1] = np.nan
    for init in (Y0[:-1], Y0.T, Y0[:, :1], bad, "random"):
        with pytest.raises(ValueError):
            ix.embed(init=init, affinities=aff)
    with pytest.raises(ValueError):
        ix.embedding_gradient(bad, aff)
    indptr, ids, p = aff
    wrong_id, wrong_p, wrong_ptr = ids.copy(), p.copy(), indptr.copy()
    wrong_id[2], wrong_p[1], wrong_ptr[3] = N, -1e-3, wrong_ptr[2] - 1
    nan_p = p.copy()
    nan_p[0] = np.nan
    for broken in (stale, (indptr, ids), (indptr, wrong_id, p), (indptr, ids, wrong_p), (indptr, ids, nan_p),
                   (wrong_ptr, ids, p), (indptr, ids[:-1], p[:-1]), (indptr, ids.astype(np.float64), p)):
        with pytest.raises(ValueError):
            ix.embed(affinities=broken, init=Y0)
        with pytest.raises(ValueError):
            ix.embedding_gradient(Y0, broken)
    # the C entries refuse the same on their own
    from trlda_amd import _ffi
    out = np.full((N, 2), -7.0)
    kl = C.c_double(-7.0)
    ptr = lambda a: a.ctypes.data
    assert hip.trlda_docindex_tsne_gradient(ix._handle, ptr(indptr), ptr(wrong_id), ptr(p), ptr(Y0), 1.0, ptr(out),
                                            C.byref(kl)) == _ffi.ERR_VALUE
    assert hip.trlda_docindex_tsne_gradient(ix._handle, ptr(indptr), ptr(ids), ptr(p), ptr(bad), 1.0, ptr(out),
                                            C.byref(kl)) == _ffi.ERR_VALUE
    assert hip.trlda_docindex_tsne_run(ix._handle, ptr(indptr), ptr(ids), ptr(wrong_p), ptr(out), 3, 1, 12.0, 50.0,
                                       0.5, 0.8, ptr(out)) == _ffi.ERR_VALUE
    assert hip.trlda_docindex_nearest(ix._handle, N, 0, ptr(out), ptr(out)) == _ffi.ERR_ARG
    assert hip.trlda_docindex_affinities(ix._handle, 40.0, 0, ptr(out), ptr(out), ptr(out)) == _ffi.ERR_ARG
    assert hip.trlda_docindex_set_tsne_tile(ix._handle, 96) == _ffi.ERR_ARG
    assert np.all(out == -7.0) and kl.value == -7.0
    assert np.array_equal(before, _state()) and len(ix) == N and _live() == live
    m.close()


def test_device_buffers_are_returned():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "embed_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout
