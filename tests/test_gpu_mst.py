"""The minimum spanning tree of a DocumentIndex on the GPU and what is built on it (csrc/mst_kernels.h,
DESIGN.md 3.33): spanning_tree edge for edge and bit for bit against Kruskal on the device's own pair
distances (neighbors_within(radius=2.0): the same bits by construction) and core distances
(nearest_neighbors), in the edge order (w, lo, hi) -- no tolerance, ties and repeated rows included; its
sorted weights against the longdouble restatement (tests/mst_host.py) within the derived bound; the core
distances; the bitwise invariances -- slabs, how the index was filled, two calls; the sweep alone with
hand-made components; hdbscan, single_linkage and cut_linkage end to end on planted groups; the errors
and the buffers.

Every array is small: at most 300 indexed documents and 100 topics.

Observed on the MI355X: every tree equal to Kruskal's on all 36 shapes and three min_samples, up to 19 of
299 weights exactly tied; the sorted weights at most 10.1 % of the bound from the restatement's (K = 33,
N = 257 and 300, cosine)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import mst_host as mh

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def hip():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


def _model(K, V=8):
    """An OnlineLDA holding a lambda without the constructor's K V 100 draws."""
    from trlda_amd.models import OnlineLDA
    lam = np.random.RandomState(77).gamma(2.0, 1.0, size=(K, V)) + 0.05
    m = OnlineLDA.__new__(OnlineLDA)
    m._num_documents = 1000
    m._update_count = 0
    m._ada_tau = 1000.
    m._ada_rho = 1. / m._ada_tau
    m._ada_sq_norm = 1.
    m._setup(V, K, .1, .3, None, _lambda=np.asfortranarray(lam))
    return m


def _filled(m, measure, g):
    ix = m.document_index(measure)
    ix.add_gamma(g)
    return ix


def _made():
    from trlda_amd import _ffi
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return total.value


def _same(p, q):
    return len(p) == len(q) and all(v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes()
                                    for v, w in zip(p, q))


def _device_distances(ix):
    """The device's own d(i, j), N x N float64 (the diagonal 0): every pair lies within 2."""
    N = len(ix)
    return mh.dense_from_csr(*ix.neighbors_within(2.0), N)


def _device_weights(ix, D, min_samples):
    """(w N x N, core N) formed on the host from the device's distances and its nearest_neighbors."""
    N = len(ix)
    if min_samples == 1:
        return D, np.zeros(N)
    core = np.ascontiguousarray(ix.nearest_neighbors(min_samples - 1)[1][:, -1])
    return np.maximum(D, np.maximum(core[:, None], core[None, :])), core


def _check_trees(ix, K, measure, restated=True):
    """spanning_tree for every min_samples of the shared list: Kruskal's tree on the device's weights,
    bit for bit; the core distances; the restatement within its bound."""
    N = len(ix)
    D = _device_distances(ix)
    assert np.array_equal(D, D.T)                                # (s(i, j) and s(j, i) are the same bits)
    d_ref = mh.sh.pair_distances(ix.rows(), measure)[0] if restated else None
    for ms in mh.MIN_SAMPLES:
        if ms > N:
            with pytest.raises(RuntimeError):
                ix.spanning_tree(ms)
            continue
        wm, core_dev = _device_weights(ix, D, ms)
        ku, kv, kw = mh.kruskal(wm)
        u, v, w, core = ix.spanning_tree(ms, return_core=True)
        assert u.dtype == v.dtype == np.int64 and w.dtype == core.dtype == np.float64
        assert u.shape == v.shape == w.shape == (N - 1,) and core.shape == (N,)
        assert np.array_equal(u, ku) and np.array_equal(v, kv), (ms, int(np.sum((u != ku) | (v != kv))))
        assert w.tobytes() == np.ascontiguousarray(kw).tobytes()
        assert np.all(u < v) and _same(ix.spanning_tree(ms), (u, v, w))
        # the core distances: the (min_samples - 1)-th smallest off-diagonal entry of the row, bitwise
        assert core.tobytes() == core_dev.tobytes()
        assert core.tobytes() == np.ascontiguousarray(mh.core_distances(D, ms)).tobytes()
        ties = len(w) - len(np.unique(w))
        if not restated or N < 2:
            print("K = %d N = %d %s min_samples %d: %d of %d weights tied" % (K, N, measure, ms, ties, len(w)))
            continue
        # the sorted weights of ANY minimum spanning tree are unique: element by element, and the total
        rw = mh.kruskal(mh.mutual_reachability(d_ref, mh.core_distances(d_ref, ms)))[2]
        bound = mh.weight_bound(rw, K, measure)
        err = np.abs(w.astype(LD) - rw).astype(np.float64)
        gap = abs(float(LD(math.fsum(w)) - rw.sum()))
        print("K = %d N = %d %s min_samples %d: %d of %d weights tied, err / bound %.3f, total off by %.3g (bound %.3g)"
              % (K, N, measure, ms, ties, len(w), float(np.max(err / bound)), gap, float(bound.sum())))
        assert np.all(err <= bound), (ms, float(np.max(err / bound)))
        assert gap <= float(bound.sum()) + mh.U * float(rw.sum())


# 1. the exact tree, the core distances and the restatement ----------------------------------------------
@pytest.mark.parametrize("measure", mh.MEASURES)
@pytest.mark.parametrize("N", mh.NS)
@pytest.mark.parametrize("K", mh.KS)
def test_tree_is_kruskals_on_the_device_weights(hip, K, N, measure):
    m = _model(K)
    ix = _filled(m, measure, mh.gammas(K, N))
    _check_trees(ix, K, measure)
    m.close()


@pytest.mark.parametrize("measure", mh.MEASURES)
def test_tree_with_repeated_rows(hip, measure):
    """The same gamma three times more: four equal rows, whose distances are rounding or exactly 0 and
    whose core distances tie -- the edge order alone decides, and the tree is still Kruskal's."""
    K = 33
    g = mh.with_repeats(mh.gammas(K, 130))
    m = _model(K)
    ix = _filled(m, measure, g)
    rows = ix.rows()
    same = [65, 131, 132]
    assert all(np.array_equal(rows[1], rows[i]) for i in same)
    _check_trees(ix, K, measure)
    # the four are one cluster under any cut above rounding, and hdbscan does not divide by zero
    labels = ix.cut_linkage(ix.single_linkage(), distance=1e-6)
    assert len({int(labels[i]) for i in [1] + same}) == 1
    got, info = ix.hdbscan(min_cluster_size=3, min_samples=2, return_info=True)
    assert np.all(np.isfinite(info["stabilities"])) and np.all(np.isfinite(info["probabilities"]))
    assert len({int(got[i]) for i in [1] + same}) == 1
    m.close()


# 2. the invariances -------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", mh.MEASURES)
def test_tree_does_not_depend_on_slabs_filling_or_the_call(hip, measure):
    K, N = 33, 300
    g = mh.gammas(K, N)
    m = _model(K)
    ix = _filled(m, measure, g)
    base = {ms: ix.spanning_tree(ms, return_core=True) for ms in mh.MIN_SAMPLES}
    for ms in mh.MIN_SAMPLES:
        assert _same(ix.spanning_tree(ms, return_core=True), base[ms])            # two calls in a row
    # three slabs with a ragged last one; slabs that are no whole pass; one slab for everything
    for slab in (128, 48, 2048):
        ix.set_slab_rows(slab)
        for ms in mh.MIN_SAMPLES:
            assert _same(ix.spanning_tree(ms, return_core=True), base[ms]), (slab, ms)
    ix.set_slab_rows(0)
    parts = m.document_index(measure)
    for a, b in ((0, 7), (7, 150), (150, N)):
        parts.add_gamma(g[:, a:b])
    for ms in mh.MIN_SAMPLES:
        assert _same(parts.spanning_tree(ms, return_core=True), base[ms])
    assert np.array_equal(parts.hdbscan(), ix.hdbscan())
    m.close()


# 3. the sweep alone -------------------------------------------------------------------------------------
def _sweep(hip, ix, comp, core):
    from trlda_amd import _ffi
    N = len(ix)
    comp = np.ascontiguousarray(comp, dtype=np.int32)
    best_j, best_w = np.full(N, -7, dtype=np.int64), np.full(N, np.nan)
    _ffi.check(hip.trlda_docindex_mst_sweep(ix._handle, comp.ctypes.data, None if core is None else core.ctypes.data,
                                            best_j.ctypes.data, best_w.ctypes.data))
    return best_j, best_w


def _argmin_sweep(wm, comp):
    """Per row the first column of another component in the order (w, j); -1 / +inf without one."""
    N = wm.shape[0]
    best_j, best_w = np.full(N, -1, dtype=np.int64), np.full(N, np.inf)
    for i in range(N):
        cand = np.flatnonzero(comp != comp[i])
        if len(cand):
            j = cand[np.lexsort((cand, wm[i, cand]))[0]]
            best_j[i], best_w[i] = j, wm[i, j]
    return best_j, best_w


@pytest.mark.parametrize("measure", mh.MEASURES)
@pytest.mark.parametrize("K,N", [(33, 130), (100, 300)])
def test_sweep_with_hand_made_components(hip, K, N, measure):
    m = _model(K)
    ix = _filled(m, measure, mh.with_repeats(mh.gammas(K, N - 3)))
    D = _device_distances(ix)
    ids = np.arange(N)
    components = {
        "a 16 x 16 tile straddles the boundary": np.where(ids < 72, 5, 2),
        "one component": np.full(N, 3),
        "every document alone": ids[::-1].copy(),
        "interleaved": ids % 3,
    }
    for ms in (1, 5):
        wm, core = _device_weights(ix, D, ms)
        for name, comp in components.items():
            best_j, best_w = _sweep(hip, ix, comp, None if ms == 1 else core)
            want_j, want_w = _argmin_sweep(wm, comp)
            assert np.array_equal(best_j, want_j), (name, ms)
            assert best_w.tobytes() == want_w.tobytes(), (name, ms)
            if name == "one component":
                assert np.all(best_j == -1)
            else:
                assert np.all(best_j >= 0) and np.all(comp[best_j] != comp)
    m.close()


# 4. end to end on planted groups ------------------------------------------------------------------------
@pytest.mark.parametrize("measure", mh.MEASURES)
def test_hdbscan_and_linkage_on_planted_groups(hip, measure):
    from trlda_amd import index as ti
    K = 33
    g, truth = mh.planted_blobs(K)
    N = g.shape[1]
    assert N == 300
    m = _model(K)
    ix = _filled(m, measure, g)
    for kwargs in (dict(), dict(min_cluster_size=10, min_samples=3), dict(selection="leaf"),
                   dict(min_cluster_size=120, allow_single_cluster=True)):
        labels, info = ix.hdbscan(return_info=True, **kwargs)
        u, v, w = info["tree"]
        mcs = kwargs.get("min_cluster_size", 5)
        ms = min(kwargs.get("min_samples", mcs), 100)
        assert _same((u, v, w), ix.spanning_tree(ms))
        ref, ref_prob, ref_stab = mh.hdbscan(u, v, w, N, mcs, kwargs.get("selection", "eom"),
                                             kwargs.get("allow_single_cluster", False))
        assert labels.dtype == np.int32 and np.array_equal(labels, ref), kwargs
        assert np.array_equal(labels, ix.hdbscan(**kwargs))
        assert np.allclose(info["stabilities"], ref_stab.astype(np.float64), rtol=1e-12, atol=0)
        assert np.allclose(info["probabilities"], ref_prob.astype(np.float64), rtol=1e-14, atol=0)
        # info['tree'] feeds single_linkage's own result
        assert np.array_equal(ti._linkage(u, v, w, N), ix.single_linkage(ms))
    # the defaults find the three blobs, whole and apart; no uniform document carries a blob's label (in
    # 33 topics uniform draws from the simplex lie near its centre, so most of them form a loose
    # group of their own rather than noise)
    labels = ix.hdbscan()
    found = [np.unique(labels[truth == t]) for t in range(3)]
    assert all(len(f) == 1 and f[0] >= 0 for f in found) and len({int(f[0]) for f in found}) == 3
    assert not set(labels[truth < 0].tolist()) & {int(f[0]) for f in found}
    # single linkage on the blobs alone (the noise left out): three clusters are the three blobs
    blobs = _filled(m, measure, np.asfortranarray(g[:, truth >= 0]))
    Z = blobs.single_linkage()
    assert Z.shape == (len(blobs) - 1, 4) and Z.dtype == np.float64
    assert np.all(np.diff(Z[:, 2]) >= 0) and Z[-1, 3] == len(blobs) and np.all(Z[:, 0] < Z[:, 1])
    cut = blobs.cut_linkage(Z, num_clusters=3)
    kept = truth[truth >= 0]
    assert len(set(zip(cut.tolist(), kept.tolist()))) == 3
    assert np.array_equal(cut, blobs.cut_linkage(Z, distance=float(Z[-3, 2])))
    m.close()


# 5. the errors and the buffers --------------------------------------------------------------------------
def test_errors_come_before_anything_runs(hip):
    from trlda_amd import _ffi
    K, N = 33, 17
    m = _model(K)
    empty = m.document_index("hellinger")
    made = _made()
    for call in (empty.spanning_tree, empty.single_linkage, empty.hdbscan):
        with pytest.raises(RuntimeError):
            call()
    one = np.zeros(1, dtype=np.int32)
    out_j, out_w = np.zeros(1, dtype=np.int64), np.zeros(1)
    assert hip.trlda_docindex_mst_sweep(empty._handle, one.ctypes.data, None, out_j.ctypes.data,
                                        out_w.ctypes.data) == _ffi.ERR_ARG
    ix = _filled(m, "cosine", mh.gammas(K, N))
    made = _made()
    for bad in (0, -1, N + 1, 101):
        with pytest.raises(RuntimeError):
            ix.spanning_tree(bad)
        with pytest.raises(RuntimeError):
            ix.single_linkage(bad)
        with pytest.raises(RuntimeError):
            ix.hdbscan(min_samples=bad)
    with pytest.raises(ValueError):
        ix.hdbscan(selection="best")
    with pytest.raises(ValueError):
        ix.hdbscan(min_cluster_size=1)
    comp = np.zeros(N, dtype=np.int32)
    out_j, out_w = np.zeros(N, dtype=np.int64), np.zeros(N)
    args = (comp.ctypes.data, None, out_j.ctypes.data, out_w.ctypes.data)
    for hole in range(4):
        if hole != 1:                                               # (core may be NULL)
            broken = args[:hole] + (None,) + args[hole + 1:]
            assert hip.trlda_docindex_mst_sweep(ix._handle, *broken) == _ffi.ERR_ARG
    assert hip.trlda_docindex_mst_sweep(None, *args) == _ffi.ERR_ARG
    for value in (-1.0, np.nan, np.inf):
        core = np.full(N, 0.5)
        core[3] = value
        assert hip.trlda_docindex_mst_sweep(ix._handle, comp.ctypes.data, core.ctypes.data, out_j.ctypes.data,
                                            out_w.ctypes.data) == _ffi.ERR_VALUE
    assert _made() == made                                          # (nothing was allocated for any of them)
    Z = ix.single_linkage()
    for bad in (dict(), dict(num_clusters=2, distance=0.1)):
        with pytest.raises(ValueError):
            ix.cut_linkage(Z, **bad)
    # min_samples=None is min_cluster_size, capped by the tree's limit: 17 documents here
    assert np.array_equal(ix.hdbscan(min_cluster_size=40), ix.hdbscan(min_cluster_size=40, min_samples=N))
    ix.close()
    with pytest.raises(RuntimeError):
        ix.spanning_tree()
    m.close()


def test_no_buffer_is_kept_by_the_calls(hip):
    """A fresh process (the count is the process's): the calls, the refused ones included, leave the
    live count as it was, and after close() the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mst_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout
