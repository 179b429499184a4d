"""The document index's entry points share their host stages (csrc/trlda_hip.hip):
one check each for the empty index, top_n, the scored rows' arguments and values, the labels and the
weights.  What the sharing claims, held to every entry point on one small index:

* a shared check refuses with the same code and message wherever it is made (the table below, written
  from the source before the stages were shared: this module passes on that library too);
* a refusal queues nothing: the valid call made before it gives the same bits after it;
* the scored rows are the same rows however they are named: all of them, their ids, a permutation of the
  ids, and -- where a gamma is taken -- the gamma they were added from.

Both measures, K = 5 and K = 130 (rows of 8 and 132 doubles: a pad and none modulo 4 of K), 37 rows
(no multiple of 16), 3 labels.  The calls of the first two go to the library through ctypes, past the
Python checks."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, V, LABELS, P, B, TOP = 37, 40, 3, 2, 4, 3
ERR_ARG, ERR_VALUE = -1, -6
EMPTY = "the index is empty"
TOP_N = "top_n must lie in [1, min(number of indexed documents, 100)]"
BOTH = "the scored rows are either ids or a gamma, not both"
NONE_SCORED = "a list of ids or a gamma needs at least one document"
ID_RANGE = "an id lies outside [0, number of indexed documents)"
GAMMA = "gamma should be finite and positive"
WEIGHT = "a weight should be finite and not negative"


def p(a):
    return None if a is None else a.ctypes.data


@pytest.fixture(scope="module", params=[(measure, K) for measure in ("hellinger", "cosine") for K in (5, 130)],
                ids=lambda c: "%s-K%d" % c)
def S(request):
    from trlda_amd import _ffi
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.models import OnlineLDA
    _ffi.require_gpu()
    measure, K = request.param
    rng = np.random.RandomState(K)
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    model.lambdas = np.asfortranarray(rng.gamma(100., 1. / 100., size=(K, V)))
    indptr = np.arange(B + 1, dtype=np.int32) * 6
    batch = model.upload(CSRDocuments(indptr, rng.randint(0, V, size=6 * B).astype(np.int32),
                                      rng.randint(1, 4, size=6 * B).astype(np.int32)))
    gamma = np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, N)) + 0.01)
    index, empty = model.document_index(measure), model.document_index(measure)
    index.add_gamma(gamma)
    rows = index.rows()
    rest = np.maximum(0.0, 1.0 - rows @ rows.T)[~np.eye(N, dtype=bool)]
    s = SimpleNamespace(
        L=_ffi.lib(), K=K, index=index, empty=empty, batch=batch, gamma=gamma,
        radius=float(np.median(rest if measure == "cosine" else np.sqrt(rest))),
        g0=np.asfortranarray(rng.gamma(100., 1. / 100., size=(K, B))),
        centroids=np.asfortranarray(gamma[:, :LABELS]),
        labels=(np.arange(N) % LABELS).astype(np.int32),            # silhouette: [0, C)
        groups=(np.arange(N) % (LABELS + 1) - 1).astype(np.int32),  # groups and classes: [-1, C)
        weights=rng.uniform(0.5, 2.0, size=N),
        design=np.ascontiguousarray(rng.normal(size=(N, P))),
        coef=np.ascontiguousarray(rng.normal(size=(LABELS, K))),
        slopes=np.ascontiguousarray(rng.normal(size=(K, P))),
        ids=np.array([5, 0, 36, 5], dtype=np.int64))
    yield s
    s.L.trlda_docindex_classify_clear(index._handle)
    index.close()
    empty.close()
    batch.close()
    model.close()


def f64(n):
    return np.full(n, np.nan)


def i64(n):
    return np.full(n, -7, dtype=np.int64)


def i32(n):
    return np.full(n, -7, dtype=np.int32)


# One function per entry point: (status, the bytes of everything it wrote).  Without keywords it is the
# valid call; a keyword replaces one argument.

def query_gamma(S, x, gamma=None, top_n=TOP):
    g = np.asfortranarray(S.gamma[:, :B]) if gamma is None else gamma
    out = i64(B * TOP), f64(B * TOP)
    return S.L.trlda_docindex_query_gamma(x, p(g), B, top_n, p(out[0]), p(out[1])), out


def query(S, x, batch=True, top_n=TOP):
    out = S.g0.copy(order="F"), i64(B * TOP), f64(B * TOP)
    return S.L.trlda_docindex_query(x, S.batch.handle if batch else None, p(out[0]), 20, 1e-3, top_n, p(out[1]),
                                    p(out[2])), out


def query_likelihood(S, x, batch=True, top_n=TOP):
    out = i64(B * TOP), f64(B * TOP)
    return S.L.trlda_docindex_query_likelihood(x, S.batch.handle if batch else None, top_n, p(out[0]), p(out[1])), out


def topic_documents(S, x, top_n=TOP):
    out = i64(S.K * TOP), f64(S.K * TOP)
    return S.L.trlda_docindex_topic_documents(x, top_n, p(out[0]), p(out[1])), out


def topic_moments(S, x):
    out = f64(S.K), f64(S.K * S.K)
    return S.L.trlda_docindex_topic_moments(x, p(out[0]), p(out[1])), out


def assign(S, x, gamma=None):
    g = np.asfortranarray(S.gamma[:, :B]) if gamma is None else gamma
    out = i32(B), f64(B)
    return S.L.trlda_docindex_assign(x, p(S.centroids), LABELS, p(g), B, p(out[0]), p(out[1])), out


def cluster(S, x):
    out = S.centroids.copy(order="F"), i32(N), f64(N), i64(LABELS)
    it, conv = C.c_int(-7), C.c_int(-7)
    rc = S.L.trlda_docindex_cluster(x, LABELS, p(out[0]), 3, p(out[1]), p(out[2]), p(out[3]), C.byref(it),
                                    C.byref(conv))
    return rc, out + (np.array([it.value, conv.value]),)


def silhouette(S, x, labels=None, ids=None, M=None):
    lab = S.labels if labels is None else labels
    M = (0 if ids is None else len(ids)) if M is None else M
    out = f64(N), f64(N), f64(N), i32(N)
    return S.L.trlda_docindex_silhouette(x, p(lab), LABELS, p(ids), M, p(out[0]), p(out[1]), p(out[2]),
                                         p(out[3])), out


def neighbors(S, x, ids=None, gamma=None, M=0):
    out = i64(N + 1), i64(N * N), f64(N * N)
    return S.L.trlda_docindex_neighbors(x, S.radius, p(ids), p(gamma), M, 0, N * N, p(out[0]), p(out[1]),
                                        p(out[2])), out


def mst_sweep(S, x):
    comp, out = np.arange(N, dtype=np.int32), (i64(N), f64(N))
    return S.L.trlda_docindex_mst_sweep(x, p(comp), None, p(out[0]), p(out[1])), out


def group_moments(S, x, labels=None, weights=None):
    w = S.weights if weights is None else weights
    out = f64(S.K * LABELS), f64(LABELS), i64(LABELS), f64(S.K * LABELS)
    return S.L.trlda_docindex_group_moments(x, p(S.groups if labels is None else labels), LABELS, p(w), p(out[0]),
                                            p(out[1]), p(out[2]), p(out[3])), out


def regress_products(S, x, weights=None):
    w = S.weights if weights is None else weights
    out = f64(P * P), f64(P * S.K)
    return S.L.trlda_docindex_regress_products(x, p(S.design), P, p(w), p(out[0]), p(out[1])), out


def regress_residuals(S, x, weights=None):
    w = S.weights if weights is None else weights
    out = (f64(S.K),)
    return S.L.trlda_docindex_regress_residuals(x, p(S.design), P, p(w), p(S.slopes), p(out[0])), out


def classify_set(S, x, labels=None, weights=None):
    w = S.weights if weights is None else weights
    out = f64(1), i64(LABELS)
    return S.L.trlda_docindex_classify_set(x, p(S.groups if labels is None else labels), LABELS, p(w), p(out[0]),
                                           p(out[1])), out


def classify_predict(S, x, ids=None, gamma=None, M=0):
    out = i32(N), f64(N * LABELS)
    return S.L.trlda_docindex_classify_predict(x, p(S.coef), LABELS, p(gamma), M, p(ids), p(out[0]), p(out[1])), out


def tsne_project(S, x):
    mean, axes, out = np.full(S.K, .5), np.ones(2 * S.K), (f64(2 * N),)
    return S.L.trlda_docindex_tsne_project(x, p(mean), p(axes), p(out[0])), out


def _with(a, i, v):
    a = a.copy(order="K")
    a.flat[i] = v
    return a


def _refusals(S):
    """(entry point, keywords of the refused call, code, a piece of the message): every shared check at
    every entry point that makes it.  `empty=True`: the call goes to the index that holds nothing."""
    few = np.asfortranarray(S.gamma[:, :B])
    table = [(call, dict(empty=True), ERR_ARG, EMPTY)
             for call in (query_gamma, query, query_likelihood, topic_documents, topic_moments, assign, cluster,
                          silhouette, neighbors, mst_sweep, group_moments, regress_products, regress_residuals,
                          classify_set, classify_predict, tsne_project)]
    # (the empty index and top_n are looked at before the batch is)
    table += [(query, dict(empty=True, batch=False), ERR_ARG, EMPTY),
              (query_likelihood, dict(empty=True, batch=False), ERR_ARG, EMPTY)]
    for top_n in (0, N + 1):
        table += [(call, dict(top_n=top_n), ERR_ARG, TOP_N)
                  for call in (query_gamma, query, query_likelihood, topic_documents)]
        table += [(query, dict(top_n=top_n, batch=False), ERR_ARG, TOP_N)]
    for call in (neighbors, classify_predict):
        table += [(call, dict(ids=S.ids, gamma=few, M=B), ERR_ARG, BOTH),
                  (call, dict(ids=S.ids, M=0), ERR_ARG, NONE_SCORED),
                  (call, dict(gamma=few, M=0), ERR_ARG, NONE_SCORED),
                  (call, dict(ids=_with(S.ids, 2, -1), M=4), ERR_VALUE, ID_RANGE),
                  (call, dict(ids=_with(S.ids, 3, N), M=4), ERR_VALUE, ID_RANGE),
                  (call, dict(gamma=_with(few, 7, 0.0), M=B), ERR_VALUE, GAMMA),
                  (call, dict(gamma=_with(few, 2, np.nan), M=B), ERR_VALUE, GAMMA)]
    table += [(silhouette, dict(ids=S.ids, M=0), ERR_ARG, "a list of ids needs at least one id"),
              (silhouette, dict(ids=_with(S.ids, 0, -1)), ERR_VALUE, ID_RANGE),
              (silhouette, dict(ids=_with(S.ids, 3, N)), ERR_VALUE, ID_RANGE)]
    for call in (query_gamma, assign):
        table += [(call, dict(gamma=_with(few, 7, 0.0)), ERR_VALUE, GAMMA),
                  (call, dict(gamma=_with(few, 2, np.nan)), ERR_VALUE, GAMMA)]
    for call, labels, message in ((silhouette, S.labels, "a label lies outside [0, C)"),
                                  (group_moments, S.groups, "a label lies outside [-1, G)"),
                                  (classify_set, S.groups, "a label lies outside [-1, C)")):
        table += [(call, dict(labels=_with(labels, 9, LABELS)), ERR_VALUE, message),
                  (call, dict(labels=_with(labels, N - 1, -2)), ERR_VALUE, message)]
    for call in (group_moments, regress_products, regress_residuals, classify_set):
        table += [(call, dict(weights=_with(S.weights, 4, -1.0)), ERR_VALUE, WEIGHT),
                  (call, dict(weights=_with(S.weights, N - 1, np.inf)), ERR_VALUE, WEIGHT)]
    return table


def _bits(out):
    return [a.tobytes() for a in out]


def test_shared_checks_refuse_alike_and_queue_nothing(S):
    valid = {}
    for call, kwargs, code, message in _refusals(S):
        if call not in valid:
            rc, out = call(S, S.index._handle)
            assert rc == 0, (call.__name__, S.L.trlda_last_error())
            valid[call] = _bits(out)
        kwargs = dict(kwargs)
        x = S.empty._handle if kwargs.pop("empty", False) else S.index._handle
        rc, _ = call(S, x, **kwargs)
        said = S.L.trlda_last_error().decode()
        assert rc == code and message in said, (call.__name__, sorted(kwargs), rc, said)
        rc, out = call(S, S.index._handle)
        assert rc == 0 and _bits(out) == valid[call], (call.__name__, sorted(kwargs))


def _lists(indptr, ids, val, drop_self=False):
    out = []
    for q in range(len(indptr) - 1):
        hit, v = ids[indptr[q]:indptr[q + 1]], val[indptr[q]:indptr[q + 1]]
        keep = hit != q if drop_self else np.ones(len(hit), dtype=bool)
        out.append((hit[keep].tobytes(), v[keep].tobytes()))
    return out


def test_scored_rows_are_the_same_rows_however_they_are_named(S):
    perm = np.random.RandomState(3).permutation(N)
    everyone = np.arange(N)
    # neighbors_within: the hit lists per scored document (a gamma finds its own document too)
    want = _lists(*S.index.neighbors_within(S.radius))
    assert 0 < sum(len(h) for h, _ in want) // 8 < N * (N - 1)
    assert _lists(*S.index.neighbors_within(S.radius, ids=everyone)) == want
    assert _lists(*S.index.neighbors_within(S.radius, ids=perm)) == [want[d] for d in perm]
    got = S.index.neighbors_within(S.radius, gamma=S.gamma)
    assert all(q in got[1][got[0][q]:got[0][q + 1]] for q in range(N))
    assert _lists(*got, drop_self=True) == want
    # predict: the classes and their probabilities
    labels, proba = S.index.predict(S.coef, return_proba=True)
    for kwargs, order in ((dict(ids=everyone), everyone), (dict(ids=perm), perm), (dict(gamma=S.gamma), everyone)):
        got_labels, got_proba = S.index.predict(S.coef, return_proba=True, **kwargs)
        assert np.array_equal(got_labels, labels[order]), sorted(kwargs)
        assert got_proba.tobytes() == proba[order].tobytes(), sorted(kwargs)
    # silhouette: the scores and their parts
    parts = S.index.silhouette(S.labels, return_parts=True)
    for order in (everyone, perm):
        got_parts = S.index.silhouette(S.labels, ids=order, return_parts=True)
        for a, b in zip(got_parts, parts):
            assert np.asarray(a).tobytes() == np.asarray(b)[order].tobytes()
