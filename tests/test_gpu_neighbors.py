"""The radius join of a DocumentIndex on the GPU (csrc/neighbors_kernels.h):
neighbors_within against the longdouble restatement (tests/neighbors_host.py) on the device's own rows --
the hit set exactly, the distances within each pair's bound; the symmetry of the hit graph; the bitwise
invariances -- slabs, how the index was filled, two calls, a subset of rows, a gamma in place of ids,
count_only; the capacity protocol; duplicates; dbscan against the breadth-first restatement; the model's
state, the buffers and the errors.

Every array is small: at most 1100 indexed documents and 130 topics.  The restatement's near-threshold
report -- how far any pair is from the radius, in bounds of the device's error -- stays above 100 on
the shapes here (tests/test_neighbors_host.py asserts it on the host's rows, the tests here on the
device's), and so does the gap between a border document's two nearest cores on the DBSCAN inputs: no
pair and no label is let off.

Observed on the MI355X, on the device's own rows against the restatement: every hit set equal on all 48
shapes at both radii; the distances at most 14.3 % of a pair's bound (K = 17, N = 1100, cosine); the
nearest pair 9.7e5 bounds from the radius (K = 33, N = 1100, cosine)."""
import ctypes as C

import numpy as np
import pytest

import neighbors_host as nh
import silhouette_host as sh

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


def _state():
    from trlda_amd import _ffi
    s = np.zeros(33, dtype=np.uint32)
    _ffi.lib().trlda_rng_get_state(s)
    return s


def _live():
    from trlda_amd import _ffi
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return live.value


def _same(p, q):
    return len(p) == len(q) and all(v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes()
                                    for v, w in zip(p, q))


def _distance(s, measure):
    """The host's distance formula (DocumentIndex._result) on a similarity."""
    rest = np.maximum(0.0, 1.0 - s)
    return np.sqrt(rest) if measure == "hellinger" else rest


def _rows_of(base, ids):
    """The CSR of the rows `ids` of the CSR `base`, in that order."""
    indptr, hit, val = base
    counts = np.diff(indptr)[ids]
    take = np.concatenate([np.arange(indptr[i], indptr[i + 1]) for i in ids] + [np.zeros(0, dtype=np.int64)])
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int64), hit[take], val[take]


# 1. the hit set against the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("measure", nh.MEASURES)
@pytest.mark.parametrize("N", nh.NS)
@pytest.mark.parametrize("K", nh.KS)
def test_hit_set_is_the_restatements(hip, K, N, measure):
    m = _model(K)
    ix = _filled(m, measure, sh.planted_gammas(K, N))
    d, bound = sh.pair_distances(ix.rows(), measure)
    for radius in nh.radii(d, K):
        ref = nh.join(d, bound, radius)
        assert ref.report > 100, (radius, ref.report)        # (so nobody is let off: the cap is 0)
        indptr, ids, dist = ix.neighbors_within(radius)
        assert indptr.dtype == ids.dtype == np.int64 and dist.dtype == np.float64
        assert indptr.shape == (N + 1,) and ids.shape == dist.shape == (int(indptr[-1]),)
        assert np.array_equal(indptr, ref.indptr) and np.array_equal(ids, ref.ids)
        share = 0.0
        if len(ids):
            err = np.abs(dist.astype(LD) - ref.dist).astype(np.float64)
            assert np.all(err <= ref.bound), (radius, float(np.max(err - ref.bound)))
            with np.errstate(divide="ignore", invalid="ignore"):
                share = float(np.max(np.where(err > 0, err / ref.bound, 0.0)))
        print("K = %d N = %d %s radius %g: %d pairs, err / bound %.3f, nearest pair %.3g bounds from the radius"
              % (K, N, measure, radius, len(ids), share, ref.report))
        # the similarity in place of the distance: the host's formula gives the device's distance, bit for bit
        indptr_s, ids_s, s = ix.neighbors_within(radius, return_similarity=True)
        assert np.array_equal(indptr_s, indptr) and np.array_equal(ids_s, ids)
        assert _distance(s, measure).tobytes() == dist.tobytes()
        assert np.array_equal(ix.neighbors_within(radius, count_only=True), indptr)
        if K == 1:
            # (every row is [1], every s exactly 1, every distance exactly 0: all pairs are hits)
            assert len(ids) == N * (N - 1) and np.all(dist == 0.0) and np.all(s == 1.0)
    m.close()


# 2. the symmetry of the hit graph -----------------------------------------------------------------------
@pytest.mark.parametrize("measure", nh.MEASURES)
def test_hits_are_symmetric_bit_for_bit(hip, measure):
    K, N = 33, 300
    m = _model(K)
    ix = _filled(m, measure, sh.planted_gammas(K, N))
    radius = nh.radii(sh.pair_distances(ix.rows(), measure)[0], K)[1]
    indptr, ids, s = ix.neighbors_within(radius, return_similarity=True)
    dist = ix.neighbors_within(radius)[2]
    rows = np.repeat(np.arange(N), np.diff(indptr))
    assert len(ids) > N and not np.any(rows == ids)
    there, back = np.argsort(rows * N + ids), np.argsort(ids * N + rows)
    assert np.array_equal((rows * N + ids)[there], (ids * N + rows)[back])       # (i, j) iff (j, i)
    assert s[there].tobytes() == s[back].tobytes() and dist[there].tobytes() == dist[back].tobytes()
    m.close()


# 3. the bitwise invariances -----------------------------------------------------------------------------
@pytest.mark.parametrize("measure", nh.MEASURES)
def test_results_do_not_depend_on_slabs_fill_subset_or_form(hip, measure):
    """1100 documents at K = 17: slabs of 64 and 128 columns and the default; an index filled in one
    add_gamma against ragged adds of 97 without reserve; two calls; a shuffled subset with repeats across
    more than one block of 128 rows, and a single row; gamma= of stored documents' own gamma, which is
    the stored-row result plus the self pair; count_only."""
    K, N = 17, 1100
    g = sh.planted_gammas(K, N)
    m = _model(K)
    whole = _filled(m, measure, g)
    radius = nh.radii(sh.pair_distances(whole.rows(), measure)[0], K)[1]
    base = whole.neighbors_within(radius)
    assert len(base[1]) > 10 * N
    assert _same(whole.neighbors_within(radius), base)
    for slab in (64, 128, 0):
        whole.set_slab_rows(slab)
        assert _same(whole.neighbors_within(radius), base), slab
        assert np.array_equal(whole.neighbors_within(radius, count_only=True), base[0])
    parts = m.document_index(measure)
    for at in range(0, N, 97):
        assert parts.add_gamma(g[:, at:at + 97]) == at
    assert len(parts) == N and np.array_equal(parts.rows(), whole.rows())
    assert _same(parts.neighbors_within(radius), base)
    rng = np.random.RandomState(8)
    for ids in (rng.permutation(N)[:301], np.concatenate([rng.randint(N, size=140), [N - 1, 0, N - 1]]), [513]):
        ids = np.asarray(ids)
        sub = whole.neighbors_within(radius, ids=ids)
        assert sub[0].shape == (len(ids) + 1,) and _same(sub, _rows_of(base, ids))
        assert np.array_equal(whole.neighbors_within(radius, ids=list(ids), count_only=True), sub[0])
        for slab in (64, 0):
            whole.set_slab_rows(slab)
            assert _same(whole.neighbors_within(radius, ids=ids), sub)
    # the documents' own gamma in place of their ids: nothing is left out, so the self pair joins
    for ids in (np.arange(N), np.array([700, 3, 3, 1099, 128, 127])):
        got = whole.neighbors_within(radius, gamma=g[:, ids])
        want = _rows_of(base, ids)
        assert np.array_equal(got[0], want[0] + np.arange(len(ids) + 1))
        rows = np.repeat(ids, np.diff(got[0]))
        me = got[1] == rows
        assert me.sum() == len(ids) and np.all(got[2][me] < 1e-7)
        assert np.array_equal(got[1][~me], want[1]) and got[2][~me].tobytes() == want[2].tobytes()
        scored = np.repeat(np.arange(len(ids)), np.diff(got[0]))
        assert np.all(np.diff(scored * N + got[1]) > 0)      # (and it stands in ascending id)
    m.close()


# 4. the capacity protocol -------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", nh.MEASURES)
def test_capacity_second_call_and_max_pairs(hip, measure):
    """N = 1100 at radius 1.0: every pair is a hit (s > 0 between positive rows), N (N - 1) = 1 208 900
    pairs, above the first guess of 2^20, so the call is made twice; a max_pairs below the total raises
    and names it, and the index goes on working."""
    K, N = 17, 1100
    m = _model(K)
    ix = _filled(m, measure, sh.planted_gammas(K, N))
    total = N * (N - 1)
    assert total > 1 << 20
    calls = []
    inner = ix._neighbors
    ix._neighbors = lambda *a: (calls.append(a[4]), inner(*a))[1]
    indptr, ids, dist = ix.neighbors_within(1.0)
    assert calls == [1 << 20, total]
    assert np.array_equal(indptr, np.arange(N + 1) * (N - 1))
    everyone = np.broadcast_to(np.arange(N), (N, N))
    assert np.array_equal(ids, everyone[~np.eye(N, dtype=bool)])
    assert np.all(dist < 1.0) and np.all(dist >= 0.0)
    del calls[:]
    assert _same(ix.neighbors_within(1.0, max_pairs=total), (indptr, ids, dist)) and calls == [1 << 20, total]
    live, state = _live(), _state()
    for max_pairs in (total - 1, 1 << 20, 5):
        del calls[:]
        with pytest.raises(RuntimeError, match=str(total)):
            ix.neighbors_within(1.0, max_pairs=max_pairs)
        assert calls == [min(max_pairs, 1 << 20)]
    assert _live() == live and np.array_equal(state, _state())
    # the index goes on working; count_only never raises
    assert np.array_equal(ix.neighbors_within(1.0, count_only=True, max_pairs=5), indptr)
    ix._neighbors = inner
    assert _same(ix.neighbors_within(1.0, ids=[N - 1, 0]), _rows_of((indptr, ids, dist), np.array([N - 1, 0])))
    m.close()


# 5. duplicates ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", nh.MEASURES)
def test_duplicates_find_each_other_and_a_small_radius_finds_nothing(hip, measure):
    """K = 130, 60 documents: 5, 20, 41, 59 are copies of one document and 7, 8 of another.  At radius
    1e-6 -- above the sqrt((K + 17) u) = 1.3e-7 that a zero distance may come out as -- every copy
    finds the others and nobody else.  Radius 0 need not: a copy's dot may round below 1."""
    K, N = 130, 60
    g = sh.planted_gammas(K, N).copy(order="F")
    for i in (20, 41, 59):
        g[:, i] = g[:, 5]
    g[:, 8] = g[:, 7]
    m = _model(K)
    ix = _filled(m, measure, g)
    ref = nh.neighbors(ix.rows(), measure, 1e-6)
    assert ref.report > 5                                    # (in bounds: 1e-6 against 1.3e-7 and less)
    indptr, ids, dist = ix.neighbors_within(1e-6)
    assert np.array_equal(indptr, ref.indptr) and np.array_equal(ids, ref.ids)
    want = {5: [20, 41, 59], 20: [5, 41, 59], 41: [5, 20, 59], 59: [5, 20, 41], 7: [8], 8: [7]}
    for i in range(N):
        assert ids[indptr[i]:indptr[i + 1]].tolist() == want.get(i, []), i
    assert np.all(dist <= ref.bound) and np.all(dist >= 0.0)
    # a radius below every distance (no duplicates here)
    m.close()
    m = _model(15)
    clean = _filled(m, measure, sh.planted_gammas(15, 17))
    d, bound = sh.pair_distances(clean.rows(), measure)
    radius = float(d[~np.eye(17, dtype=bool)].min()) / 2
    assert radius > 0 and nh.join(d, bound, radius).report > 100
    indptr, ids, dist = clean.neighbors_within(radius)
    assert not indptr.any() and indptr.shape == (18,) and ids.shape == dist.shape == (0,)
    assert ids.dtype == np.int64 and dist.dtype == np.float64
    assert not clean.neighbors_within(radius, ids=[3, 3], count_only=True).any()
    m.close()


# 6. dbscan ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", nh.MEASURES)
def test_dbscan_is_the_restatements(hip, measure):
    """Four planted groups of 40 and five far-away documents at K = 23 (neighbors_host.planted_groups)."""
    radius, min_samples = nh.DBSCAN_CASES[measure]
    g, truth = nh.planted_groups()
    N = g.shape[1]
    m = _model(g.shape[0])
    ix = _filled(m, measure, g)
    ref = nh.neighbors(ix.rows(), measure, radius)
    want, want_core, gap = nh.dbscan(ref.indptr, ref.ids, ref.dist, min_samples, ref.bound)
    assert ref.report > 100 and gap > 100                    # (so no label is let off)
    assert want.max() == 3 and np.any(~want_core & (want >= 0))
    labels, core = ix.dbscan(radius, min_samples, return_core=True)
    assert labels.dtype == np.int32 and labels.shape == (N,) and core.dtype == bool
    assert np.array_equal(labels, want) and np.array_equal(core, want_core)
    assert np.array_equal(ix.dbscan(radius, min_samples), labels)
    assert np.all(labels[-5:] == -1)                         # the planted outliers
    kept = labels[:len(truth)] >= 0
    assert len(set(zip(labels[:len(truth)][kept].tolist(), truth[kept].tolist()))) == 4
    # chunks: max_pairs as small as the longest list allows, and a few sizes above it
    longest = int(np.diff(ref.indptr).max())
    calls = []
    inner = ix._neighbors
    ix._neighbors = lambda *a: (calls.append(a[4]), inner(*a))[1]
    for max_pairs in (longest, longest + 1, 3 * longest + 7, 1000):
        del calls[:]
        assert np.array_equal(ix.dbscan(radius, min_samples, max_pairs=max_pairs), labels), max_pairs
        if max_pairs == longest:
            assert len(calls) > 20
    with pytest.raises(RuntimeError, match="max_pairs"):
        ix.dbscan(radius, min_samples, max_pairs=longest - 1)
    # min_samples = 1: every document is a core, the outliers are clusters of their own
    labels, core = ix.dbscan(radius, 1, return_core=True)
    assert core.all() and np.array_equal(labels, nh.dbscan(ref.indptr, ref.ids, ref.dist, 1)[0])
    assert labels.min() == 0 and len(set(labels[-5:].tolist())) == 5
    # nobody is a core
    assert np.all(ix.dbscan(radius, N + 1) == -1)
    for bad in (0, -3):
        with pytest.raises(ValueError):
            ix.dbscan(radius, bad)
    # the labels go into the silhouette once noise has a label of its own
    s = ix.silhouette(np.where(want < 0, want.max() + 1, want))
    assert s.shape == (N,) and np.all(np.abs(s) <= 1.0)
    m.close()


# 7. the model's state, the buffers and the errors --------------------------------------------------------
def test_state_is_left_alone(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K, N = 16, 40
    m = _model(K)
    g = sh.planted_gammas(K, N)
    ix = _filled(m, "hellinger", g)
    rows = ix.rows()
    rng = np.random.RandomState(31)
    docs = [[(int(w), int(rng.randint(1, 5))) for w in rng.choice(8, size=rng.randint(2, 7), replace=False)]
            for _ in range(9)]
    _, sstats = m.update_variables(docs, latents=np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 9)) + 0.1),
                                   max_iter=20)
    held = np.empty((K, 8), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, held))
    assert np.array_equal(held, sstats) and np.any(held > 0)
    before = (np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count)
    trlda_amd.seed(9)
    state, live = _state(), _live()
    ix.neighbors_within(0.3)
    ix.neighbors_within(0.3, ids=[3, 3, 39], return_similarity=True)
    ix.neighbors_within(0.3, gamma=g[:, :5], count_only=True)
    ix.dbscan(0.3, 3)
    with pytest.raises(RuntimeError, match="max_pairs"):
        ix.neighbors_within(1.0, max_pairs=7)
    assert np.array_equal(state, _state()) and _live() == live
    assert len(ix) == N and np.array_equal(ix.rows(), rows)
    assert np.array_equal(np.asarray(m.lambdas), before[0]) and np.array_equal(np.asarray(m.alpha), before[1])
    assert m.eta == before[2] and m.update_count == before[3]
    after_stats = np.empty((K, 8), order="F")
    _ffi.check(hip.trlda_model_get_sstats(m._handle, after_stats))
    assert np.array_equal(after_stats, held)                      # the model's statistics: no E-step ran
    m.close()


def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K, N = 8, 12
    m = _model(K)
    ix = m.document_index("cosine")
    g = sh.planted_gammas(K, N)
    trlda_amd.seed(3)
    before = _state()
    indptr = np.full(N + 2, -7, dtype=np.int64)
    out_i = np.full(4 * N * N, -7, dtype=np.int64)
    out_v = np.full(4 * N * N, -7.)
    ids = np.array([0, 5], dtype=np.int64)
    two = np.asfortranarray(g[:, :2].copy())

    def call(handle, radius=0.5, ids=None, gamma=None, count=0, capacity=len(out_i), ip=indptr, oi=out_i, ov=out_v):
        ptr = lambda a: None if a is None else a.ctypes.data
        return hip.trlda_docindex_neighbors(handle, radius, ptr(ids), ptr(gamma), count, 0, capacity, ptr(ip), ptr(oi),
                                            ptr(ov))

    live = _live()
    # an empty index
    assert call(ix._handle) == _ffi.ERR_ARG
    for refused in (lambda: ix.neighbors_within(0.5), lambda: ix.dbscan(0.5)):
        with pytest.raises(RuntimeError, match="empty"):
            refused()
    assert _live() == live
    ix.add_gamma(g)
    live = _live()
    # arguments: NULL index / indptr, both ids and gamma, no document with either, a negative capacity,
    # values without ids
    assert call(None) == _ffi.ERR_ARG and call(ix._handle, ip=None) == _ffi.ERR_ARG
    assert call(ix._handle, ids=ids, gamma=two, count=2) == _ffi.ERR_ARG
    for count in (0, -1):
        assert call(ix._handle, ids=ids, count=count) == _ffi.ERR_ARG
        assert call(ix._handle, gamma=two, count=count) == _ffi.ERR_ARG
    assert call(ix._handle, capacity=-1) == _ffi.ERR_ARG
    assert call(ix._handle, oi=None) == _ffi.ERR_ARG         # (out_v is given)
    assert _live() == live
    # values: the radius, an id outside [0, N), a gamma that is not finite and positive
    for radius in (-0.1, -0.0 - 1e-300, np.inf, -np.inf, np.nan):
        assert call(ix._handle, radius=radius) == _ffi.ERR_VALUE, radius
    for bad in (N, -1):
        assert call(ix._handle, ids=np.array([0, bad], dtype=np.int64), count=2) == _ffi.ERR_VALUE
    for bad in (0.0, -1.0, np.inf, np.nan):
        wrong = two.copy(order="F")
        wrong[3, 1] = bad
        assert call(ix._handle, gamma=wrong, count=2) == _ffi.ERR_VALUE
    assert _live() == live
    # nothing was written or drawn
    assert np.all(indptr == -7) and np.all(out_i == -7) and np.all(out_v == -7.)
    assert len(ix) == N and np.array_equal(before, _state())
    # the same through Python
    for bad, error in (((-0.1,), ValueError), ((np.nan,), ValueError), ((np.inf,), ValueError), (("a",), ValueError),
                       ((None,), TypeError)):
        with pytest.raises(error):
            ix.neighbors_within(*bad)
        with pytest.raises(error):
            ix.dbscan(*bad)
    for kwargs, error in ((dict(ids=[N]), RuntimeError), (dict(ids=[-1, 0]), RuntimeError),
                          (dict(ids=np.array([], dtype=np.int64)), RuntimeError), (dict(ids=[[0]]), RuntimeError),
                          (dict(ids=[0.5]), TypeError), (dict(ids=[0], gamma=two), ValueError),
                          (dict(gamma=g[:-1]), RuntimeError), (dict(gamma=-g), RuntimeError),
                          (dict(max_pairs=0), ValueError), (dict(max_pairs=1.5), TypeError)):
        with pytest.raises(error):
            ix.neighbors_within(0.5, **kwargs)
        assert _live() == live
    assert np.array_equal(before, _state()) and _live() == live
    # what the C call does with its arrays: a count-only call; a capacity below the total writes indptr
    # alone and returns TRLDA_OK; values may be left out; the exact capacity fills
    full = ix.neighbors_within(0.5)
    total = int(full[0][-1])
    assert 0 < total < len(out_i)
    assert call(ix._handle, oi=None, ov=None, capacity=0) == 0 and np.array_equal(indptr[:N + 1], full[0])
    indptr[:] = -7
    assert call(ix._handle, capacity=total - 1) == 0
    assert np.array_equal(indptr[:N + 1], full[0]) and indptr[N + 1] == -7
    assert np.all(out_i == -7) and np.all(out_v == -7.)
    assert call(ix._handle, ov=None, capacity=total) == 0
    assert np.array_equal(out_i[:total], full[1]) and np.all(out_i[total:] == -7) and np.all(out_v == -7.)
    assert call(ix._handle, capacity=total) == 0
    assert np.array_equal(out_v[:total], full[2]) and np.all(out_v[total:] == -7.)
    assert call(ix._handle, ids=ids, count=2, capacity=total) == 0
    assert np.array_equal(indptr[:3], ix.neighbors_within(0.5, ids=ids)[0]) and indptr[3] == full[0][3]
    assert _live() == live and np.array_equal(before, _state())
    # a closed index
    ix.close()
    live = _live()
    for refused in (lambda: ix.neighbors_within(0.5), lambda: ix.dbscan(0.5)):
        with pytest.raises(RuntimeError, match="closed"):
            refused()
        assert _live() == live
    m.close()
