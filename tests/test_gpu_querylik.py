"""DocumentIndex.query_likelihood on the GPU (csrc/querylik_kernels.h): scores and ids
against the restatement (tests/querylik_host.py) on theta^ of the device's own rows, exact ties, the
bitwise invariances, the edges and the device buffers.

Every array is small: V = 40 words, 300 indexed documents and 12 queries of 1 to 40 distinct words."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import querylik_host as qh
import topicdocs_host as th

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
GAP_FLOOR = 1e-9                         # 75 times the largest score bound (1.3e-11: 40 words at K = 513)
MEASURES = ["hellinger", "cosine"]
V, N_MAX = 40, 300
# one word; both sides of one tile of 16; two tiles plus one word; every word of V
LENGTHS = [1, 2, 3, 5, 15, 16, 17, 31, 33, 40, 1, 4]
KS = [3, 4, 5, 64, 65, 100, 513]


def prob_bound(K, V=V):
    """|P_dev - P_longdouble| / P, to first order: the bound of test_gpu_recommend.prob_bound for the
    same product and the same row sums -- V - 1 additions of a row sum, the division by it, a chain of
    K products and K additions, every term positive; theta^ is the device's own on both sides, so
    what that bound allows for sum(gamma) and its division is slack here."""
    return (V + 2 * K + 8) * U


def score_bound(K, P, s, query, V=V):
    """|s_dev - s_longdouble| per document for one query, to first order; P (N x V) and s (N) are the
    restatement's.  With t_i = c_i log P_i and every t_i <= 0 (P < 1) nothing cancels:
      log(P_dev) = log(P) + log(1 + e), |e| <= eps_P = prob_bound(K): off by eps_P absolutely;
      the device's log is taken as within 1 ulp = 2 u relatively, the product c_i * log one rounding, u:
        together 3 u |log P_i| per term, times c_i;
      the n_q - 1 additions of the terms (whatever their order: the partial sums have one sign and never
        exceed |s|) and the one of the tiles' sums to 0.0 (exact), with the reference's own rounding on
        top: (n_q + 1) u |s|.
    |s_dev - s_ld| <= sum_i c_i (eps_P + 3 u |log P_i|) + (n_q + 1) u |s|."""
    bound = np.zeros(P.shape[0], dtype=np.float64)
    for w, c in query:
        bound += c * (prob_bound(K, V) + 3 * U * np.abs(np.log(P[:, w]).astype(np.float64)))
    return bound + (len(query) + 1) * U * np.abs(np.asarray(s, dtype=np.float64))


@pytest.fixture(scope="module")
def hip():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


def _model(K, V=V, lam=None, alpha=.1, eta=.3):
    """An OnlineLDA holding `lam` without the constructor's K V 100 draws."""
    from trlda_amd.models import OnlineLDA
    if lam is None:
        lam = _lam(K)
    m = OnlineLDA.__new__(OnlineLDA)
    m._num_documents = 1000
    m._update_count = 0
    m._ada_tau = 1000.
    m._ada_rho = 1. / m._ada_tau
    m._ada_sq_norm = 1.
    m._setup(V, K, alpha, eta, None, _lambda=np.asfortranarray(lam))
    return m


def _lam(K, V=V):
    return np.random.RandomState(77).gamma(2.0, 1.0, size=(K, V)) + 0.05


def _gammas(K, n, seed):
    """n gamma columns: sparse-ish topic weights of very different totals."""
    rng = np.random.RandomState(seed)
    g = rng.gamma(0.3, 1.0, size=(K, n)) + 0.01
    return np.asfortranarray(g * rng.uniform(0.5, 40.0, size=n))


def _queries(K):
    """The 12 queries of a case: distinct words, counts 1 to 4."""
    rng = np.random.RandomState(500 + K)
    out = []
    for n in LENGTHS:
        words = rng.choice(V, n, replace=False)
        counts = rng.randint(1, 5, size=n)
        out.append([(int(w), int(c)) for w, c in zip(words, counts)])
    return out


def _state():
    from trlda_amd import _ffi
    s = np.zeros(33, dtype=np.uint32)
    _ffi.lib().trlda_rng_get_state(s)
    return s


_REFERENCE = {}


def _reference(K, measure, rows):
    """(P N x V, scores 12 x N, order 12 x N) of the restatement on theta^ of the device's rows of a
    case: computed once per (K, measure) and shared; a later caller's rows must be the same bits."""
    key = (K, measure)
    if key not in _REFERENCE:
        theta = th.theta_hat(rows, measure)
        P = qh.probs(theta, _lam(K))
        s = qh.scores(theta, _lam(K), _queries(K))
        for a in (P, s):
            a.flags.writeable = False
        _REFERENCE[key] = (rows.copy(), P, s, qh.rank(s))
    kept, P, s, order = _REFERENCE[key]
    assert np.array_equal(kept, rows)
    return P, s, order


def _index(m, measure, gamma):
    ix = m.document_index(measure)
    ix.add_gamma(gamma)
    return ix


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# 1. scores and ids ---------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", KS)
def test_scores_and_ids(hip, K, measure):
    """top_n in 1, 10, 100 over 300 documents.  The inputs have no near ties: the restatement's smallest
    gap among the first top_n + 1 stays above GAP_FLOOR for every query (asserted first) and is printed
    against the case's largest score bound (2.5e3 times it at K = 513, more elsewhere), so every id of
    every query is compared.  Observed on the MI355X: the worst error is 10.7 % of its bound (K = 5,
    cosine), 1.6 % at K = 513."""
    queries = _queries(K)
    m = _model(K)
    ix = _index(m, measure, _gammas(K, N_MAX, 4000 + K))
    P, want, order = _reference(K, measure, ix.rows())
    bounds = np.stack([score_bound(K, P, want[b], q) for b, q in enumerate(queries)])
    ranked = np.take_along_axis(want, order, axis=1)
    worst, least = 0.0, np.inf
    for top_n in (1, 10, 100):
        gap = qh.gaps(ranked, top_n)
        assert gap.min() > GAP_FLOOR, (top_n, gap.min())
        ids, s = ix.query_likelihood(queries, top_n=top_n)
        assert ids.dtype == np.int64 and s.dtype == np.float64 and ids.shape == s.shape == (12, top_n)
        assert np.array_equal(ids, order[:, :top_n]), top_n
        err = np.abs(s.astype(LD) - ranked[:, :top_n]).astype(np.float64)
        ratio = float(np.max(err / np.take_along_axis(bounds, ids, axis=1)))
        worst, least = max(worst, ratio), min(least, float(gap.min() / bounds.max()))
        assert ratio <= 1.0, (top_n, ratio)
        assert np.all(np.diff(s, axis=1) <= 0) and np.all(s < 0)
        ids_w, s_w = ix.query_likelihood(queries, top_n=top_n, per_word=True)
        totals = np.array([sum(c for _, c in q) for q in queries], dtype=np.float64)
        assert np.array_equal(ids_w, ids) and np.array_equal(s_w, s / totals[:, None])
    print("K = %d %s: worst error / bound %.3f, smallest gap / largest bound %.1e" % (K, measure, worst, least))
    m.close()


# 2. exact ties -------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", [4, 64])
def test_exact_ties_rank_by_id(hip, K, measure):
    """The same gamma column T at ids 7, 150 and 299 (three passes of 128 rows; with slabs of 64 three
    slabs): for every query the three scores are the same bits and come in id order.  To be among the
    first 100 of every query, ids 97 .. 298 (but 150) hold copies of one column J that scores below T
    for EVERY query -- the pair is picked from a pool with the restatement in float64, by a margin of
    1e-6 -- so at most the 96 documents of ids 0 .. 96 (but 7) come before T."""
    queries = _queries(K)
    pool = _gammas(K, 1200, 7000 + K)
    import docindex_host as dh
    s = qh.scores(th.theta_hat(dh.rows(pool, measure), measure), _lam(K), queries).astype(np.float64)
    below = np.array([np.all(s < s[:, t:t + 1] - 1e-6, axis=0).sum() for t in range(pool.shape[1])])
    T = int(below.argmax())
    assert below[T] > 0
    J = int(np.flatnonzero(np.all(s < s[:, T:T + 1] - 1e-6, axis=0))[0])
    gi = _gammas(K, N_MAX, 4000 + K)
    gi[:, 97:] = pool[:, J:J + 1]
    gi[:, [7, 150, 299]] = pool[:, T:T + 1]
    m = _model(K)
    ix = _index(m, measure, gi)
    for rows in (0, 64):
        ix.set_slab_rows(rows)
        ids, sc = ix.query_likelihood(queries, top_n=100)
        for b in range(12):
            at = int(np.flatnonzero(ids[b] == 7)[0])
            assert at <= 96 and list(ids[b, at:at + 3]) == [7, 150, 299], (b, ids[b])
            assert sc[b, at] == sc[b, at + 1] == sc[b, at + 2]
            # the copies of J that made it: one run behind T, in id order, all with the same bits
            run = np.flatnonzero((ids[b] >= 97) & (ids[b] != 150) & (ids[b] != 299))
            assert len(run) > 0 and run[0] > at + 2 and np.array_equal(run, np.arange(run[0], run[0] + len(run)))
            assert np.array_equal(ids[b, run], [i for i in range(97, 299) if i != 150][:len(run)])
            assert np.all(sc[b, run] == sc[b, run[0]]) and sc[b, run[0]] < sc[b, at]
    m.close()


# 3. invariances ------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", [5, 100])
def test_invariances(hip, K, measure):
    """All bitwise: the queries alone and in batches of 1, 5 and 12; slabs of 64, 112 (three slabs, the
    last of 76 rows) and the default; the index filled in calls of 7, 1 and 292 documents; the first
    130 documents against all 300; an uploaded batch against a list."""
    queries = _queries(K)
    gi = _gammas(K, N_MAX, 4000 + K)
    m = _model(K)
    ix = _index(m, measure, gi)
    whole = ix.query_likelihood(queries, top_n=100)
    for b, q in enumerate(queries):
        ids, s = ix.query_likelihood([q], top_n=100)
        assert np.array_equal(ids[0], whole[0][b]) and np.array_equal(s[0], whole[1][b]), b
    for B in (1, 5):
        ids, s = ix.query_likelihood(queries[-B:], top_n=100)
        assert np.array_equal(ids, whole[0][-B:]) and np.array_equal(s, whole[1][-B:])
    for rows in (64, 112, 0):
        ix.set_slab_rows(rows)
        assert _same(ix.query_likelihood(queries, top_n=100), whole), rows
        ids, s = ix.query_likelihood(queries, top_n=3)
        assert np.array_equal(ids, whole[0][:, :3]) and np.array_equal(s, whole[1][:, :3])
    batch = m.upload(queries)
    assert _same(ix.query_likelihood(batch, top_n=100), whole)
    assert _same(ix.query_likelihood(batch, top_n=100), whole)             # (the batch is still there)
    batch.close()
    parts = m.document_index(measure)
    parts.add_gamma(gi[:, :7])
    parts.add_gamma(gi[:, 7])
    parts.add_gamma(gi[:, 8:])
    assert _same(parts.query_likelihood(queries, top_n=100), whole)
    # fewer rows: a document present in both results has the same bits
    few = _index(m, measure, gi[:, :130])
    ids_f, s_f = few.query_likelihood(queries, top_n=100)
    shared = 0
    for b in range(12):
        both, at_f, at_w = np.intersect1d(ids_f[b], whole[0][b], return_indices=True)
        assert np.array_equal(s_f[b, at_f], whole[1][b, at_w])
        # (and they keep their order)
        assert np.array_equal(ids_f[b][np.isin(ids_f[b], both)], whole[0][b][np.isin(whole[0][b], both)])
        shared += len(both)
    assert shared > 12 * 20
    m.close()


# 4. edges ------------------------------------------------------------------------------------------
def test_empty_queries_and_small_indexes(hip):
    K = 5
    queries = _queries(K)
    gi = _gammas(K, N_MAX, 4000 + K)
    m = _model(K)
    ix = _index(m, "hellinger", gi)
    want = ix.query_likelihood(queries, top_n=10)
    mixed = [queries[3], [], queries[8], []]
    for per_word in (False, True):
        ids, s = ix.query_likelihood(mixed, top_n=10, per_word=per_word)
        for b in (1, 3):
            assert np.array_equal(ids[b], np.arange(10)) and np.all(s[b] == 0.0) and not np.any(np.signbit(s[b]))
    ids, s = ix.query_likelihood(mixed, top_n=10)
    assert np.array_equal(ids[[0, 2]], want[0][[3, 8]]) and np.array_equal(s[[0, 2]], want[1][[3, 8]])
    ids, s = ix.query_likelihood([[]], top_n=100)
    assert np.array_equal(ids[0], np.arange(100)) and np.all(s == 0.0)
    # an entry with a count of 0 adds nothing (behind the others: their positions stay)
    spare = min(set(range(V)) - {w for w, _ in queries[3]})
    ids, s = ix.query_likelihood([queries[3] + [(spare, 0)], [(2, 0)]], top_n=10)
    assert np.array_equal(ids[0], want[0][3]) and np.array_equal(s[0], want[1][3])
    assert np.array_equal(ids[1], np.arange(10)) and np.all(s[1] == 0.0)
    # no queries
    ids, s = ix.query_likelihood([], top_n=2)
    assert ids.shape == s.shape == (0, 2) and ids.dtype == np.int64
    # N = 1 and N = 17
    whole = ix.query_likelihood(queries, top_n=100)
    one = _index(m, "hellinger", gi[:, :1])
    ids, s = one.query_likelihood(queries, top_n=1)
    assert np.all(ids == 0) and np.all(np.isfinite(s)) and np.all(s < 0)
    some = _index(m, "hellinger", gi[:, :17])
    ids, s = some.query_likelihood(queries, top_n=17)
    assert np.array_equal(np.sort(ids, axis=1), np.tile(np.arange(17), (12, 1)))
    for b in range(12):
        both, at_s, at_w = np.intersect1d(ids[b], whole[0][b], return_indices=True)
        assert np.array_equal(s[b, at_s], whole[1][b, at_w])
        hit = np.flatnonzero(ids[b] == 0)
        assert s[b, hit[0]] == one.query_likelihood([queries[b]], top_n=1)[1][0, 0]
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_no_probability_is_minus_infinity(hip, measure):
    """No topic gives word 2 any probability: -inf for every document, ranked by id.  Word 1 has its
    mass in topic 0 alone, and documents 1 and 4 hold an exact zero of it (gamma_0 = 5e-324 against a
    sum of about 100: the quotient rounds to 0, and so do the row and theta^): -inf for those two,
    ranked last, by id, behind the finite ones.  No NaN anywhere."""
    K, N = 4, 6
    lam = _lam(K)
    lam[:, 2] = 0.0
    lam[1:, 1] = 0.0
    gi = _gammas(K, N, 3)
    gi[1:, [1, 4]] += 30.0
    gi[0, [1, 4]] = 5e-324
    m = _model(K, lam=lam)
    ix = _index(m, measure, gi)
    assert np.all(ix.rows()[[1, 4], 0] == 0.0)
    queries = [[(2, 1)], [(2, 3), (5, 1)], [(1, 2)], [(7, 2), (1, 1)], [(7, 2), (5, 1)]]
    ids, s = ix.query_likelihood(queries, top_n=N)
    assert not np.any(np.isnan(s))
    for b in (0, 1):
        assert np.array_equal(ids[b], np.arange(N)) and np.all(np.isneginf(s[b]))
    want_ids, want_s, _ = qh.search(th.theta_hat(ix.rows(), measure), lam, queries, N)
    assert np.array_equal(ids, want_ids)
    for b in (2, 3):
        assert list(ids[b, 4:]) == [1, 4] and np.all(np.isneginf(s[b, 4:])) and np.all(np.isfinite(s[b, :4]))
        assert np.allclose(s[b, :4], want_s[b, :4].astype(np.float64), rtol=1e-12, atol=0)
    assert np.all(np.isfinite(s[4]))
    m.close()


def test_refusals(hip):
    import trlda_amd
    from trlda_amd import _ffi
    from trlda_amd.documents import DeviceBatch
    K, N = 8, 12
    queries = _queries(K)[:4]
    m = _model(K)
    ix = m.document_index("cosine")
    trlda_amd.seed(3)
    before = _state()
    ids = np.full((4, 101), -7, dtype=np.int64)
    s = np.full((4, 101), -7.)
    mine = m.upload(queries)
    other = DeviceBatch(queries, V + 1, 0)

    def refused(top_n, batch=mine):
        handle = batch.handle if batch is not None else None
        assert hip.trlda_docindex_query_likelihood(ix._handle, handle, top_n, ids.ctypes.data,
                                                   s.ctypes.data) == _ffi.ERR_ARG

    refused(1)                                           # an empty index
    with pytest.raises(RuntimeError, match="top_n"):
        ix.query_likelihood(queries, top_n=1)
    ix.add_gamma(_gammas(K, N, 1))
    for top_n in (0, -1, N + 1, 101):
        refused(top_n)
        with pytest.raises(RuntimeError, match="top_n"):
            ix.query_likelihood(queries, top_n=top_n)
    with pytest.raises(TypeError):
        ix.query_likelihood(queries, top_n=2.5)
    refused(1, other)
    refused(1, None)
    assert hip.trlda_docindex_query_likelihood(None, mine.handle, 1, ids.ctypes.data, s.ctypes.data) == _ffi.ERR_ARG
    assert hip.trlda_docindex_query_likelihood(ix._handle, mine.handle, 1, None, s.ctypes.data) == _ffi.ERR_ARG
    with pytest.raises(RuntimeError, match="different model"):
        ix.query_likelihood(other, top_n=1)
    assert np.array_equal(before, _state()) and np.all(ids == -7) and np.all(s == -7.)
    # a lambda with a zero row: its row sum is refused
    lam = np.array(m.lambdas)
    spoiled = lam.copy()
    spoiled[K - 1] = 0.0
    m.lambdas = spoiled
    with pytest.raises(_ffi.TrldaError, match="row sums") as info:
        ix.query_likelihood(queries, top_n=1)
    assert info.value.code == _ffi.ERR_ARG
    refused(1)
    assert np.all(ids == -7) and np.all(s == -7.)
    m.lambdas = lam
    got, sc = ix.query_likelihood(mine, top_n=N)
    assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(N), (4, 1))) and np.all(np.diff(sc, axis=1) <= 0)
    ix.close()
    ix.close()
    with pytest.raises(RuntimeError, match="closed"):
        ix.query_likelihood(queries, top_n=1)
    for b in (mine, other):
        b.close()
    m.close()
    with pytest.raises(RuntimeError, match="closed"):
        ix.query_likelihood(queries, top_n=1)


def test_state_is_left_alone(hip):
    """Nothing is drawn, and an E-step before and one after the call give the bits they give without it."""
    import trlda_amd
    K = 16
    queries = _queries(K)
    rng = np.random.RandomState(21)
    docs = [[(int(w), int(c)) for w, c in zip(rng.choice(V, 12, replace=False), rng.randint(1, 5, size=12))]
            for _ in range(30)]
    g0 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 30)) + 0.1)
    g1 = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 12)) + 0.1)

    def run(between):
        m = _model(K, alpha=.2, eta=.05)
        out = [m.update_variables(docs, latents=g0, max_iter=20)]
        if between:
            kept = (np.asarray(m.lambdas).copy(), np.asarray(m.alpha).copy(), m.eta, m.update_count)
            ix = _index(m, "hellinger", out[0][0])
            trlda_amd.seed(9)
            state = _state()
            for per_word in (False, True):
                ix.query_likelihood(queries, top_n=7, per_word=per_word)
            assert np.array_equal(state, _state())
            assert np.array_equal(np.asarray(m.lambdas), kept[0]) and np.array_equal(np.asarray(m.alpha), kept[1])
            assert m.eta == kept[2] and m.update_count == kept[3]
        out.append(m.update_variables(queries, latents=g1, max_iter=20))
        m.close()
        return out

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def test_above_the_vi_bound(hip):
    """K = TRLDA_VI_MAX_TOPICS + 1: query refuses (it needs an E-step), query_likelihood runs."""
    from trlda_amd import _ffi
    K, Vs, N = _ffi.vi_max_topics() + 1, 20, 20
    lam = _lam(K, Vs)
    m = _model(K, Vs, lam)
    try:
        ix = _index(m, "hellinger", _gammas(K, N, 9))
        query = [[(3, 2), (11, 1), (19, 1)]]
        with pytest.raises(_ffi.TrldaError, match="TRLDA_VI_MAX_TOPICS"):
            ix.query(query, top_n=5)
        ids, s = ix.query_likelihood(query, top_n=N)
        theta = th.theta_hat(ix.rows(), "hellinger")
        want_ids, want_s, gap = qh.search(theta, lam, query, N)
        assert gap.min() > GAP_FLOOR
        assert np.array_equal(ids, want_ids)
        bound = score_bound(K, qh.probs(theta, lam), qh.scores(theta, lam, query)[0], query[0], Vs)[ids[0]]
        assert np.all(np.abs(s[0].astype(LD) - want_s[0]).astype(np.float64) <= bound)
    finally:
        m.close()


# 5. device buffers ---------------------------------------------------------------------------------
def test_closing_releases_every_device_buffer(hip):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "querylik_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout
