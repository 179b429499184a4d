"""The entry points that read only lambda, or a word-by-word table built beside it, share their host
stages (csrc/trlda_hip.hip): one wait for queued copies, one waited upload of a
caller's array, one flag read, one plan and one merge loop of the top-N tree, one top_n check.  What the
sharing claims, held to every entry point of the family:

* a shared check refuses with the same code and message wherever it is made (the table below, written
  from the source before the stages were shared: this module passes on that library too);
* a refusal queues nothing: the valid call made before it gives the same bits after it;
* a batch that trlda_anchor_add refuses on the device leaves the accumulator as it found it;
* trlda_anchor_read gives the same rows however they are named: all of them, their ids, a permutation;
* the workspace that relevance, word similarity and the diagnostics share carries nothing from one to
  the next;
* a lambda with a non-positive entry (trlda_model_set_lambda accepts it) is refused by each entry point
  with its own message, and the valid call on the restored lambda gives the old bits;
* the top-N tree with a merge level (11 tiles of 1024 words x 100 = 1100 candidates per row, the
  smallest shape that has one) and without (3 tiles x 10) ranks as the host restatements do.

The small model: K = 5 and K = 130 (rows of 8 and 132 doubles: a pad and none modulo 4 of K), V = 40, a
batch of 4 documents of 6 distinct words, an accumulator filled from it and one loaded from an exactly
separable 40 x 40 matrix.  Its calls go to the library through ctypes, past the Python checks."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import anchor_host as ah
import coherence_host as ch
import relevance_host as vh
from test_gpu_relevance import Ref, _check_relevance, _check_salient, _given, _lam, _model

pytestmark = pytest.mark.gpu

V, B, TOP, CAP, LISTS, ANCHORS = 40, 4, 3, 101, 2, 3
ERR_ARG, ERR_WORD_ID, ERR_VALUE = -1, -3, -6
TOP_N = "top_n must lie in [1, min(num_words, 100)]"
TOP_N_SELF = "top_n must lie in [1, min(num_words - 1, 100)]"
WEIGHTS = "topic weights should be finite and positive"
WEIGHT = "weight must lie in [0, 1]"
MEASURE = "unknown measure"
WORD_ID = "word id outside [0, num_words)"
ANCHOR_COUNT = "the number of anchors must lie in "
ONCE = "a co-occurrence batch must list a word at most once per document"


def p(a):
    return None if a is None else a.ctypes.data


@pytest.fixture(scope="module", params=[5, 130], ids=lambda K: "K%d" % K)
def S(request):
    from trlda_amd import _ffi
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.models import OnlineLDA
    _ffi.require_gpu()
    K = request.param
    rng = np.random.RandomState(K)
    L = _ffi.lib()
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    lam = np.asfortranarray(rng.gamma(2.0, 1.0, size=(K, V)) + 0.05)
    model.lambdas = lam
    indptr = np.arange(B + 1, dtype=np.int32) * 6
    ids = np.concatenate([rng.choice(V, 6, replace=False) for _ in range(B)]).astype(np.int32)
    batch = model.upload(CSRDocuments(indptr, ids, rng.randint(1, 4, size=6 * B).astype(np.int32)))
    twice = model.upload(CSRDocuments([0, 3, 5], [4, 7, 4, 1, 2], [1, 2, 1, 1, 1]))
    handles = [_ffi.vp() for _ in range(2)]
    for h in handles:
        assert L.trlda_anchor_create(model._handle, 1 << 30, C.byref(h)) == 0
    assert L.trlda_anchor_add(handles[0], batch.handle) == 0
    Q, _, planted = ah.planted(ANCHORS, V)
    s = SimpleNamespace(
        L=L, K=K, model=model, m=model._handle, lam=lam, batch=batch, twice=twice, filled=handles[0],
        loaded=handles[1], Q=np.ascontiguousarray(Q), anchors=np.asarray(planted, dtype=np.int32),
        doc_freq=rng.randint(0, 9, size=V).astype(np.int64),
        given=rng.gamma(0.5, 1.0, K) + 0.01, other=rng.gamma(0.5, 1.0, K) + 0.01,
        lists=np.array([3, 0, 39, 7, 3, 21], dtype=np.int32),       # LISTS x TOP
        topic_words=np.tile(np.array([9, 0, 39], dtype=np.int32), K),
        ids=np.array([5, 0, 39, 5], dtype=np.int32),
        props=np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, B)) + 0.01))
    yield s
    for h in handles:
        L.trlda_anchor_destroy(h)
    twice.close()
    batch.close()
    model.close()


def f64(n):
    return np.full(n, np.nan)


def i64(n):
    return np.full(n, -7, dtype=np.int64)


def i32(n):
    return np.full(n, -7, dtype=np.int32)


# One function per entry point: (status, everything it wrote).  Without keywords it is the valid call; a
# keyword replaces one argument.  Outputs have room for the largest top_n a refusal names.

def top_words(S, top_n=TOP):
    out = (i32(S.K * CAP),)
    return S.L.trlda_model_top_words(S.m, top_n, out[0]), out


def cooc(S, words=None, T=LISTS, N=TOP):
    """create, add the batch, read, destroy: the status of the first that fails"""
    handle = C.c_void_p()
    rc = S.L.trlda_cooc_create(S.m, S.lists if words is None else words, T, N, C.byref(handle))
    if rc:
        assert not handle.value
        return rc, ()
    out, docs = (i64(T * N), i64(T * N * N)), C.c_int64(-7)
    rc = S.L.trlda_cooc_add(handle, S.batch.handle) or S.L.trlda_cooc_read(handle, out[0], out[1], C.byref(docs))
    S.L.trlda_cooc_destroy(handle)
    return rc, out + (np.array([docs.value]),)


def word_stats(S, weights=None):
    out = f64(V), f64(V), f64(V)
    return S.L.trlda_model_word_stats(S.m, p(weights), p(out[0]), p(out[1]), p(out[2])), out


def relevant_words(S, top_n=TOP, weight=0.6, weights=None):
    out = i32(S.K * CAP), f64(S.K * CAP)
    return S.L.trlda_model_relevant_words(S.m, top_n, weight, p(weights), p(out[0]), p(out[1])), out


def salient_words(S, top_n=TOP, weights=None):
    out = i32(CAP), f64(CAP)
    return S.L.trlda_model_salient_words(S.m, top_n, p(weights), p(out[0]), p(out[1])), out


def word_diagnostics(S, top_n=TOP, weights=None, words=None):
    out = tuple(f64(S.K) for _ in range(5))
    w = S.topic_words if words is None else words
    return S.L.trlda_model_word_diagnostics(S.m, top_n, p(weights), p(w), *[p(a) for a in out]), out


def similar_words(S, ids=None, top_n=TOP, measure=0, weights=None, exclude_self=1):
    out = i32(B * CAP), f64(B * CAP)
    return S.L.trlda_model_similar_words(S.m, p(S.ids if ids is None else ids), B, top_n, measure, p(weights),
                                         exclude_self, p(out[0]), p(out[1])), out


def similar_words_rows(S, props=None, top_n=TOP, measure=0, weights=None):
    out = i32(B * CAP), f64(B * CAP)
    return S.L.trlda_model_similar_words_rows(S.m, p(S.props if props is None else props), B, top_n, measure,
                                              p(weights), p(out[0]), p(out[1])), out


def word_topic_proportions(S, ids=None, weights=None):
    out = (f64(S.K * B),)
    return S.L.trlda_model_word_topic_proportions(S.m, p(S.ids if ids is None else ids), B, p(weights),
                                                  p(out[0])), out


def topic_distances(S, other=False, lam=None, K2=None, measure=0):
    out = (f64(S.K * (S.K + 1)),)
    return S.L.trlda_model_topic_distances(S.m, S.m if other else None, p(lam), S.K if K2 is None else K2, measure,
                                           p(out[0])), out


def anchor_load(S, Q=None, doc_freq=None):
    """load, then every row"""
    rc = S.L.trlda_anchor_load(S.loaded, p(S.Q if Q is None else Q), p(S.doc_freq if doc_freq is None else doc_freq))
    return (rc, ()) if rc else anchor_read(S)


def anchor_read(S, rows=None, n=None, handle=None):
    out = (f64(V * V),)
    n = (V if rows is None else len(rows)) if n is None else n
    return S.L.trlda_anchor_read(handle or S.loaded, p(rows), n, p(out[0])), out


def anchor_counts(S, handle):
    out = i64(V), i64(V), i64(3)
    return S.L.trlda_anchor_counts(handle, *out), out


def anchor_row_sums(S):
    out, total = (f64(V),), C.c_double(-7.0)
    rc = S.L.trlda_anchor_row_sums(S.loaded, p(out[0]), C.byref(total))
    return rc, out + (np.array([total.value]),)


def anchor_select(S, num=ANCHORS):
    out = i32(V + 1), f64(V + 1), f64(V + 1)
    return S.L.trlda_anchor_select(S.loaded, num, 0, out[0], p(out[1]), p(out[2])), out


def anchor_recover(S, anchors=None, A=ANCHORS):
    out = f64(V * (V + 1)), f64(V + 1), f64(V * (V + 1)), i32(V), f64(V)
    return S.L.trlda_anchor_recover(S.loaded, S.anchors if anchors is None else anchors, A, 1e-9, 50,
                                    *[p(a) for a in out]), out


def _with(a, i, v):
    a = a.copy(order="K")
    a.flat[i] = v
    return a


def _refusals(S):
    """(entry point, keywords of the refused call, code, a piece of the message): every shared check at
    every entry point that makes it."""
    K = S.K
    table = []
    for top_n in (0, 101, V + 1):
        table += [(call, dict(top_n=top_n), ERR_ARG, TOP_N)
                  for call in (top_words, relevant_words, salient_words, word_diagnostics, similar_words_rows)]
        table += [(similar_words, dict(top_n=top_n, exclude_self=0), ERR_ARG, TOP_N)]
    table += [(similar_words, dict(top_n=top_n), ERR_ARG, TOP_N_SELF) for top_n in (0, 101, V)]
    for call in (word_stats, relevant_words, salient_words, word_diagnostics, similar_words, similar_words_rows,
                 word_topic_proportions):
        table += [(call, dict(weights=_with(S.given, i, bad)), ERR_ARG, WEIGHTS)
                  for i, bad in ((0, 0.0), (K - 1, -1.0), (2, np.nan), (K // 2, np.inf))]
    table += [(relevant_words, dict(weight=bad), ERR_ARG, WEIGHT) for bad in (-0.1, 1.5, np.nan)]
    for bad in (-1, 99):
        table += [(call, dict(measure=bad), ERR_ARG, MEASURE)
                  for call in (similar_words, similar_words_rows, topic_distances)]
    for call in (similar_words, word_topic_proportions):
        table += [(call, dict(ids=_with(S.ids, 1, -1)), ERR_WORD_ID, WORD_ID),
                  (call, dict(ids=_with(S.ids, 3, V)), ERR_WORD_ID, WORD_ID)]
    table += [(similar_words_rows, dict(props=_with(S.props, i, bad)), ERR_VALUE,
               "proportions should be finite and positive")
              for i, bad in ((0, 0.0), (K * B - 1, -1.0), (K + 1, np.nan), (3, np.inf))]
    in_lists = WORD_ID + " in the word lists"
    table += [(word_diagnostics, dict(words=_with(S.topic_words, 1, -1)), ERR_WORD_ID, in_lists),
              (word_diagnostics, dict(words=_with(S.topic_words, K * TOP - 1, V)), ERR_WORD_ID, in_lists),
              (word_diagnostics, dict(words=_with(S.topic_words, K * TOP - 1, 9)), ERR_ARG,
               "a word list holds a word twice")]
    shape = "word lists must number at least one and hold 2 to 100 ids each"
    table += [(cooc, dict(T=0), ERR_ARG, shape), (cooc, dict(N=1), ERR_ARG, shape),
              (cooc, dict(words=np.zeros(101, dtype=np.int32), T=1, N=101), ERR_ARG, shape),
              (cooc, dict(words=_with(S.lists, 4, -1)), ERR_ARG, "word id out of range in the word lists"),
              (cooc, dict(words=_with(S.lists, 2, V)), ERR_ARG, "word id out of range in the word lists"),
              (cooc, dict(words=_with(S.lists, 5, 7)), ERR_ARG, "a word occurs twice in one word list")]
    table += [(anchor_select, dict(num=0), ERR_ARG, ANCHOR_COUNT + "[1, num_words]"),
              (anchor_select, dict(num=V + 1), ERR_ARG, ANCHOR_COUNT + "[1, num_words]"),
              (anchor_recover, dict(A=0), ERR_ARG, ANCHOR_COUNT + "[1, min(num_words, "),
              (anchor_recover, dict(anchors=np.arange(V + 1, dtype=np.int32), A=V + 1), ERR_ARG,
               ANCHOR_COUNT + "[1, min(num_words, "),
              (anchor_recover, dict(anchors=_with(S.anchors, 1, -1)), ERR_ARG, "anchor word out of range"),
              (anchor_recover, dict(anchors=_with(S.anchors, 2, V)), ERR_ARG, "anchor word out of range"),
              (anchor_recover, dict(anchors=_with(S.anchors, 2, S.anchors[0])), ERR_ARG,
               "an anchor word occurs twice"),
              (anchor_read, dict(n=-1), ERR_ARG, "bad number of rows"),
              (anchor_read, dict(n=V + 1), ERR_ARG, "bad number of rows"),
              (anchor_read, dict(rows=_with(S.ids, 0, -1)), ERR_ARG, "row out of range"),
              (anchor_read, dict(rows=_with(S.ids, 3, V)), ERR_ARG, "row out of range")]
    values = "the co-occurrence matrix must be finite and non-negative"
    table += [(anchor_load, dict(Q=_with(S.Q, V + 1, np.nan)), ERR_VALUE, values),
              (anchor_load, dict(Q=_with(S.Q, V * V - 1, np.inf)), ERR_VALUE, values),
              (anchor_load, dict(Q=_with(S.Q, 5, -1.0)), ERR_VALUE, values),
              (anchor_load, dict(Q=_with(S.Q, 3 * V + 1, S.Q[3, 1] + 1.0)), ERR_VALUE,
               "the co-occurrence matrix must be symmetric"),
              (anchor_load, dict(doc_freq=_with(S.doc_freq, V - 1, -1)), ERR_VALUE, "doc_freq must not be negative")]
    table += [(topic_distances, dict(other=True, lam=np.asfortranarray(S.lam)), ERR_ARG,
               "give another model or a host lambda, not both"),
              (topic_distances, dict(K2=K + 1), ERR_ARG, "K2 is not the second lambda's number of topics"),
              (topic_distances, dict(K2=0), ERR_ARG, "K2 is not the second lambda's number of topics"),
              (topic_distances, dict(lam=np.asfortranarray(S.lam), K2=0), ERR_ARG,
               "K2 is not the second lambda's number of topics")]
    return table


def _bits(out):
    return [a.tobytes() for a in out]


def _valid(S, call, **kwargs):
    rc, out = call(S, **kwargs)
    assert rc == 0, (call.__name__, sorted(kwargs), S.L.trlda_last_error())
    return _bits(out)


def test_shared_checks_refuse_alike_and_queue_nothing(S):
    # (the loaded accumulator first: select, recover and read work from it)
    valid = {call: _valid(S, call) for call in (anchor_load, anchor_row_sums)}
    for call, kwargs, code, message in _refusals(S):
        if call not in valid:
            valid[call] = _valid(S, call)
        rc, _ = call(S, **kwargs)
        said = S.L.trlda_last_error().decode()
        assert rc == code and message in said, (call.__name__, sorted(kwargs), rc, said)
        assert _valid(S, call) == valid[call], (call.__name__, sorted(kwargs))
    assert _valid(S, anchor_row_sums) == valid[anchor_row_sums]
    assert len(valid) == 15


def test_a_batch_refused_on_the_device_leaves_the_accumulator_as_it_was(S):
    from trlda_amd import _ffi
    handles = [_ffi.vp() for _ in range(2)]
    try:
        for h in handles:
            assert S.L.trlda_anchor_create(S.m, 1 << 30, C.byref(h)) == 0
        rc = S.L.trlda_anchor_add(handles[0], S.twice.handle)
        said = S.L.trlda_last_error().decode()
        assert rc == ERR_VALUE and ONCE in said, (rc, said)
        got = []
        for h in handles:
            assert S.L.trlda_anchor_add(h, S.batch.handle) == 0
            got.append(_valid(S, anchor_counts, handle=h) + _valid(S, anchor_read, handle=h))
        assert got[0] == got[1]
        # (and it is what the fixture's accumulator holds, with its 4 documents counted)
        assert got[0] == _valid(S, anchor_counts, handle=S.filled) + _valid(S, anchor_read, handle=S.filled)
        assert np.frombuffer(got[0][2], dtype=np.int64)[0] == B
    finally:
        for h in handles:
            S.L.trlda_anchor_destroy(h)


def test_anchor_read_gives_the_same_rows_however_they_are_named(S):
    _valid(S, anchor_load)
    for handle in (S.loaded, S.filled):
        rc, (every,) = anchor_read(S, handle=handle)
        assert rc == 0
        every = every.reshape(V, V)
        assert np.array_equal(every, every.T) and every.any()
        perm = np.random.RandomState(3).permutation(V).astype(np.int32)
        for rows in (np.arange(V, dtype=np.int32), perm, S.ids):
            rc, (got,) = anchor_read(S, rows=rows, handle=handle)
            assert rc == 0
            assert got[:len(rows) * V].tobytes() == every[rows].tobytes()
            assert np.isnan(got[len(rows) * V:]).all()
        rc, (got,) = anchor_read(S, n=0, handle=handle)             # no row: nothing is written
        assert rc == 0 and np.isnan(got).all()
        rc, (got,) = anchor_read(S, n=7, handle=handle)             # the first rows
        assert rc == 0 and got[:7 * V].tobytes() == every[:7].tobytes() and np.isnan(got[7 * V:]).all()
    assert np.array_equal(anchor_read(S)[1][0].reshape(V, V), S.Q)


def test_the_shared_workspace_carries_nothing_over(S):
    """relevance.coef, .stats, .pi and .flag serve relevance, the word similarities and the diagnostics:
    each call forms what it reads."""
    calls = [(relevant_words, dict(weights=S.given)), (similar_words, dict()),
             (word_diagnostics, dict(weights=S.other))]
    for first in range(3):
        order = calls[first:] + calls[:first]
        want = _valid(S, order[0][0], **order[0][1])
        for call, kwargs in order[1:]:
            _valid(S, call, **kwargs)
        assert _valid(S, order[0][0], **order[0][1]) == want, order[0][0].__name__


def test_a_bad_lambda_is_refused_by_each_with_its_own_message(S):
    flagged = [(word_stats, "relevance"), (relevant_words, "relevance"), (salient_words, "relevance"),
               (word_diagnostics, "topic diagnostics"), (similar_words, "word similarity"),
               (similar_words_rows, "word similarity"), (word_topic_proportions, "word similarity")]
    valid = {call: _valid(S, call) for call, _ in flagged}
    valid[top_words] = _valid(S, top_words)
    bad = S.lam.copy(order="F")
    bad[S.K - 2, 17] = 0.0
    try:
        S.model.lambdas = bad
        for call, what in flagged:
            rc, out = call(S)
            said = S.L.trlda_last_error().decode()
            assert rc == ERR_VALUE and said.endswith(what + " needs a positive, finite lambda"), (call.__name__, said)
            assert all(np.isnan(a).all() if a.dtype == np.float64 else (a == -7).all() for a in out)
    finally:
        S.model.lambdas = S.lam
    for call in valid:
        assert _valid(S, call) == valid[call], call.__name__


# ---- the tree ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("V_tree, top_n", [(10300, 100), (2100, 10)], ids=["one-merge-level", "no-merge-level"])
def test_the_top_n_tree_ranks_as_the_host_does(V_tree, top_n):
    """K = 9: two tiles of 8 topics.  V = 10 300, top_n = 100: ceil(V / 1024) x top_n = 1100 > 1024
    candidates per row, one merge level before the final one; V = 2100, top_n = 10: 30 candidates, the
    final level alone.  Continuous random lambda: no ties (the restatements' gaps are asserted by the
    checks of tests/test_gpu_relevance.py, whose bounds these are)."""
    from trlda_amd import _ffi
    _ffi.require_gpu()
    K = 9
    lam = _lam(K, V_tree)
    m = _model(K, V_tree, lam)
    try:
        words = m.top_words(top_n)
        assert words.dtype == np.int32 and np.array_equal(words, ch.top_words(lam, top_n))
        for given, weight in ((None, 0.6), (_given(K), 0.3)):
            ref = Ref(lam, given)
            _check_relevance(m, ref, weight, top_n)
            _check_salient(m, ref, top_n)
        # weight = 1 ranks by lambda's rows: the two trees agree
        assert np.array_equal(m.relevant_words(top_n, 1.0), words)
        assert vh.rank(lam[0], top_n, relative=False)[0].tolist() == words[0].tolist()
    finally:
        m.close()
