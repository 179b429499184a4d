"""Indexed documents classified from their topic proportions on the GPU (csrc/classify_kernels.h,
DESIGN.md 3.35): ``DocumentIndex.classifier_loss``, ``fit_classifier``, ``predict`` and ``knn_predict`` of
both measures against the restatement (tests/classify_host.py) of the device's own rows: the loss and the
gradient within their first-order rounding bounds at every edge of K, C and N, an exact and a wide-range
case, what the sums do not depend on bit for bit, the fit against the restatement's Newton optimum within
the strong-convexity bound, the predictions, the vote, the model's state, the buffers and the errors.

Every array is small: at most 300 indexed documents, 130 topics and 128 classes.  The observed shares of
the bounds are printed by each test and recorded in DESIGN.md 3.35."""
import os
import subprocess
import sys

import numpy as np
import pytest

import classify_host as ch

pytestmark = pytest.mark.gpu

U = ch.U
LD = np.longdouble
MEASURES = ["hellinger", "cosine"]
N_MAX = 300
PARITY = 1e-9                                   # the relative parity tolerance of the project's tests (README)
SHAPES = ([(K, 5, N_MAX) for K in (1, 3, 16, 33, 65, 130)] +
          [(17, C, N_MAX) for C in (2, 3, 16, 17, 63, 64, 65, 128)] +
          [(17, 3, N) for N in (1, 2, 63, 64, 65, 129)])
FIT_SHAPES = [(6, 3, 120), (17, 5, 300), (65, 17, 300)]


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
    return _gammas(K, N_MAX, 6000 + K)[:, :N]


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


def _labels(N, C, seed=1):
    """Labels over scattered ids: class 1 without members (from C = 3), about one document in six left
    out (-1) but never document 0."""
    rng = np.random.RandomState(100 * seed + 7 * N + C)
    lab = rng.randint(0, C, size=N)
    if C >= 3:
        lab[lab == 1] = 0
    order = 1 + rng.permutation(N - 1) if N > 1 else np.zeros(0, dtype=int)
    lab[order[5::6]] = -1
    return lab.astype(np.int64)


def _weights(N, seed=5):
    """Weights with zeros (never document 0's)."""
    w = np.random.RandomState(seed).uniform(0.5, 30.0, size=N)
    w[3::11] = 0.0
    return w


def _coef(C, K, seed=3, scale=3.0):
    return np.random.RandomState(seed + 31 * C + K).normal(size=(C, K)) * scale


def _raw(hip, ix, W, labels, C, w=None):
    """(loss_sum, grad_sum, weight_sum, counts) straight from the library."""
    from trlda_amd import _ffi
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    W = np.ascontiguousarray(W, dtype=np.float64)
    omega, counts = np.zeros(1), np.zeros(C, dtype=np.int64)
    loss, grad = np.zeros(1), np.empty((C, ix._K))
    _ffi.check(hip.trlda_docindex_classify_set(ix._handle, lab.ctypes.data, C, None if w is None else w.ctypes.data,
                                               omega.ctypes.data, counts.ctypes.data))
    try:
        _ffi.check(hip.trlda_docindex_classify_eval(ix._handle, W.ctypes.data, loss.ctypes.data, grad.ctypes.data))
    finally:
        _ffi.check(hip.trlda_docindex_classify_clear(ix._handle))
    return float(loss[0]), grad, float(omega[0]), counts


def _check_sums(name, theta, W, lab, w, loss, grad, omega):
    """The device's sums within their bounds of the longdouble ones; the bounds are not vacuous."""
    N = theta.shape[0]
    want_loss, want_grad, want_omega = ch.loss_grad(theta, W, lab, w)
    lb, gb = ch.loss_bound(theta, W, lab, w), ch.grad_bound(theta, W, lab, w)
    le = abs(float(LD(loss) - want_loss))
    ge = np.abs(np.asarray(grad.astype(LD) - want_grad, dtype=np.float64))
    print("%s: loss error %.3g = %.3f of its bound (%.3g of the loss), gradient %.3f of its bound (%.3g of max |grad|)"
          % (name, le, le / lb, lb / float(want_loss), float(np.max(ge / gb)),
             float(gb.max() / np.max(np.abs(want_grad)))))
    assert np.isfinite(loss) and np.all(np.isfinite(grad))
    assert lb <= PARITY * float(want_loss) and gb.max() <= PARITY * float(np.max(np.abs(want_grad)))
    assert le <= lb
    assert np.all(ge <= gb), float(np.max(ge / gb))
    assert abs(float(LD(omega) - want_omega)) <= (N + 16) * U * float(want_omega)


# -- the loss and the gradient ---------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K,C,N", SHAPES)
def test_loss_and_gradient_within_their_bounds(hip, measure, K, C, N):
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    theta = ch.theta_hat(ix.rows(), measure)
    lab, W = _labels(N, C), _coef(C, K)
    for w in (None, _weights(N)):
        loss, grad, omega = ix.classifier_loss(W, lab, weights=w, num_classes=C)
        assert grad.shape == (C, K) and grad.dtype == np.float64
        _check_sums("%s K %d C %d N %d %s" % (measure, K, C, N, "weighted" if w is not None else "plain"),
                    theta, W, lab, w, loss, grad, omega)
        raw = _raw(hip, ix, W, lab, C, w)
        assert raw[0] == loss and np.array_equal(raw[1], grad) and raw[2] == omega
        assert np.array_equal(raw[3], np.bincount(lab[lab >= 0], minlength=C))
        if C >= 3:
            assert raw[3][1] == 0                                     # (the class without members)
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_zero_coefficients_are_the_uniform_model(hip, measure):
    K, C, N = 17, 5, N_MAX
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    theta = ch.theta_hat(ix.rows(), measure)
    lab, w, W = _labels(N, C), _weights(N), np.zeros((C, K))
    loss, grad, omega = ix.classifier_loss(W, lab, weights=w, num_classes=C)
    _check_sums(measure + " zero coefficients", theta, W, lab, w, loss, grad, omega)
    want = np.asarray(ch._weights(w, lab).sum() * np.log(LD(C)), dtype=np.float64)
    assert abs(loss - want) <= ch.loss_bound(theta, W, lab, w)
    labels, p = ix.predict(W, return_proba=True)
    assert np.all(labels == 0)                                        # (all logits equal: the smallest class)
    assert np.all(np.abs(p - 1.0 / C) <= ch.proba_bound(theta, W))
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_wide_range_coefficients(hip, measure):
    K, C, N = 17, 5, N_MAX
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    theta = ch.theta_hat(ix.rows(), measure)
    lab, w = _labels(N, C), _weights(N)
    W = np.random.RandomState(12).uniform(-1e3, 1e3, size=(C, K))
    z = theta.dot(W.T)
    assert np.max(z.max(axis=1) - z.min(axis=1)) > 300.0              # (logits hundreds apart)
    loss, grad, omega = ix.classifier_loss(W, lab, weights=w, num_classes=C)
    _check_sums(measure + " wide range", theta, W, lab, w, loss, grad, omega)
    labels, p = ix.predict(W, return_proba=True)
    want = np.asarray(ch.forward(theta, W)["p"], dtype=np.float64)
    assert np.all(np.isfinite(p)) and np.all(p >= 0) and np.all(np.abs(p - want) <= ch.proba_bound(theta, W))
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_sums_are_bitwise_independent_of_slab_filling_and_call(hip, measure):
    K, C, N = 17, 5, N_MAX
    g = _case(K, N)
    m = _model(K)
    ix = _filled(m, measure, g)
    lab, w, W = _labels(N, C), _weights(N), _coef(C, K)
    first = ix.classifier_loss(W, lab, weights=w, num_classes=C)
    again = ix.classifier_loss(W, lab, weights=w, num_classes=C)
    assert first[0] == again[0] and np.array_equal(first[1], again[1]) and first[2] == again[2]
    for rows in (64, 128, 0):
        ix.set_classify_slab(rows)
        got = ix.classifier_loss(W, lab, weights=w, num_classes=C)
        assert got[0] == first[0] and np.array_equal(got[1], first[1]), rows
    stepped = _filled(m, measure, g, step=7)
    assert np.array_equal(stepped.rows(), ix.rows())
    got = stepped.classifier_loss(W, lab, weights=w, num_classes=C)
    assert got[0] == first[0] and np.array_equal(got[1], first[1])
    # a document relabelled -1, and the same document given weight 0: the same sums
    d = int(np.flatnonzero((lab >= 0) & (w > 0))[17])
    out, zero = lab.copy(), w.copy()
    out[d], zero[d] = -1, 0.0
    a = ix.classifier_loss(W, out, weights=w, num_classes=C)
    b = ix.classifier_loss(W, lab, weights=zero, num_classes=C)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert a[0] != first[0] and not np.array_equal(a[1], first[1])
    # what a left-out document is labelled otherwise does not matter, nor does its weight
    moved = w.copy()
    moved[lab < 0] = 99.0
    c = ix.classifier_loss(W, lab, weights=moved, num_classes=C)
    assert c[0] == first[0] and np.array_equal(c[1], first[1])
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_renumbering_the_classes_permutes_the_gradient(hip, measure):
    """Two classes swapped: S = e_0 + e_1 is the same bits either way, so the rows of grad_sum swap and
    nothing else changes.  With more classes a renumbering changes the order in which S is added (it is
    the ascending class order by contract), so the sums agree within their bounds, not bit for bit."""
    K, N = 17, N_MAX
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    theta = ch.theta_hat(ix.rows(), measure)
    w = _weights(N)
    lab, W = _labels(N, 2), _coef(2, K)
    a = ix.classifier_loss(W, lab, weights=w, num_classes=2)
    b = ix.classifier_loss(W[::-1], np.where(lab >= 0, 1 - lab, -1), weights=w, num_classes=2)
    assert a[0] == b[0] and np.array_equal(a[1], b[1][::-1]) and a[2] == b[2]
    C = 5
    perm = np.array([3, 0, 4, 1, 2])                                  # class c becomes perm[c]
    lab, W = _labels(N, C), _coef(C, K)
    Wp = np.empty_like(W)
    Wp[perm] = W
    labp = np.where(lab >= 0, perm[np.maximum(lab, 0)], -1)
    a = ix.classifier_loss(W, lab, weights=w, num_classes=C)
    b = ix.classifier_loss(Wp, labp, weights=w, num_classes=C)
    _check_sums(measure + " renumbered", theta, Wp, labp, w, b[0], b[1], b[2])
    assert abs(a[0] - b[0]) <= 2 * ch.loss_bound(theta, W, lab, w)
    assert np.all(np.abs(a[1] - b[1][perm]) <= 2 * ch.grad_bound(theta, W, lab, w)) and a[2] == b[2]
    m.close()


# -- the fit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K,C,N", FIT_SHAPES)
def test_fit_reaches_the_newton_optimum(hip, measure, K, C, N):
    import trlda_amd
    l2, tol = 1e-2, 1e-9
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    theta = ch.theta_hat(ix.rows(), measure)
    rng = np.random.RandomState(40 + K)
    true = rng.normal(size=(C, K)) * 6.0
    lab = np.argmax(theta.dot(true.T) + rng.gumbel(size=(N, C)), axis=1)
    lab[rng.permutation(N)[:N // 6]] = -1
    w = _weights(N)
    trlda_amd.seed(4)
    state, lam = _state(), np.asarray(m.lambdas).copy()
    fit = ix.fit_classifier(lab, num_classes=C, l2=l2, weights=w, tol=tol)
    assert np.array_equal(state, _state()) and np.array_equal(np.asarray(m.lambdas), lam)
    assert fit["converged"] and fit["coef"].shape == (C, K) and fit["l2"] == l2
    assert 1 <= fit["iterations"] <= 200 and fit["evaluations"] > fit["iterations"]
    assert fit["nobs"] == np.count_nonzero((lab >= 0) & (w > 0))
    assert fit["counts"].dtype == np.int64 and np.array_equal(fit["counts"], np.bincount(lab[lab >= 0], minlength=C))
    W = fit["coef"]
    omega = float(ch._weights(w, lab).sum())
    F, g = ch.objective(theta, W, lab, w, l2)
    gb = float(ch.grad_bound(theta, W, lab, w).max()) / omega
    gb += 4 * U * float(np.max(np.abs(g)) + l2 * np.max(np.abs(W)))          # (the division and the penalty)
    lb = ch.loss_bound(theta, W, lab, w) / omega + (C * K + 16) * U * float(F)
    gmax = float(np.max(np.abs(g)))
    assert gmax <= tol + gb
    assert abs(fit["loss"] - float(F)) <= lb and abs(fit["grad_norm"] - gmax) <= gb
    W_newton, _ = ch.newton(theta, lab, w, l2, C)
    g_newton = ch.objective(theta, W_newton, lab, w, l2)[1]
    dist = float(np.sqrt(((W.astype(LD) - W_newton) ** 2).sum()))
    bound = float(np.sqrt((g * g).sum()) + np.sqrt((g_newton * g_newton).sum())) / l2
    print("%s K %d C %d N %d: %d iterations, %d evaluations, max |grad F| %.3g, |W - W*| %.3g = %.3f of the bound"
          % (measure, K, C, N, fit["iterations"], fit["evaluations"], gmax, dist, dist / bound))
    assert dist <= bound
    warm = ix.fit_classifier(lab, num_classes=C, l2=l2, weights=w, tol=tol, init=W)
    assert warm["converged"] and warm["evaluations"] == 1 and warm["iterations"] == 0
    assert np.array_equal(warm["coef"], W)
    short = ix.fit_classifier(lab, num_classes=C, l2=l2, weights=w, tol=tol, max_iter=1)
    assert short["converged"] is False and short["iterations"] == 1
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_fit_separates_well_separated_classes(hip, measure):
    K, C, N = 12, 4, 200
    rng = np.random.RandomState(21)
    lab = np.arange(N) % C
    g = np.full((K, N), 0.05)
    for c in range(C):
        g[3 * c:3 * c + 3, lab == c] += rng.gamma(4.0, 2.0, size=(3, np.count_nonzero(lab == c)))
    m = _model(K)
    ix = _filled(m, measure, np.asfortranarray(g))
    theta = ch.theta_hat(ix.rows(), measure)
    fit = ix.fit_classifier(lab)
    want, _, near = ch.predict(theta, fit["coef"])
    assert near.size == 0 and np.array_equal(want, lab)               # the restatement does: assert that first
    assert np.array_equal(ix.predict(fit["coef"]), lab)
    m.close()


# -- the predictions -------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K,C,N", [(17, 5, N_MAX), (65, 17, N_MAX), (17, 128, 129), (3, 2, 65)])
def test_predictions_equal_the_restatement(hip, measure, K, C, N):
    g = _case(K, N)
    m = _model(K)
    ix = _filled(m, measure, g)
    theta = ch.theta_hat(ix.rows(), measure)
    W = _coef(C, K)
    want, p, near = ch.predict(theta, W)
    assert near.size == 0                                             # nothing is excused
    labels, proba = ix.predict(W, return_proba=True)
    assert labels.dtype == np.int32 and proba.shape == (N, C)
    assert np.array_equal(labels, want) and np.array_equal(ix.predict(W), labels)
    err = np.abs(np.asarray(proba.astype(LD) - p, dtype=np.float64))
    bound = ch.proba_bound(theta, W)
    print("%s K %d C %d N %d: p within %.3f of its bound" % (measure, K, C, N, float(np.max(err / bound))))
    assert np.all(err <= bound) and bound.max() <= PARITY
    assert np.all(np.abs(np.asarray(proba.astype(LD).sum(axis=1) - 1, dtype=np.float64)) <= C * U)
    # the same document by its id, among all N, and by its gamma: the same bits
    ids = np.array([N - 1, 0, N // 2, 0], dtype=np.int64)
    by_id = ix.predict(W, ids=ids, return_proba=True)
    by_gamma = ix.predict(W, gamma=np.asfortranarray(g[:, ids]), return_proba=True)
    for got in (by_id, by_gamma):
        assert np.array_equal(got[0], labels[ids]) and np.array_equal(got[1], proba[ids])
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_an_exact_tie_goes_to_the_smaller_class(hip, measure):
    K, C, N = 17, 6, N_MAX
    m = _model(K)
    ix = _filled(m, measure, _case(K, N))
    W = _coef(C, K, scale=1.0)
    W[4] = W[1] = W[1] + 4.0                                          # two identical rows, mostly the largest
    labels, p = ix.predict(W, return_proba=True)
    assert np.count_nonzero(labels == 1) > N // 2 and not np.any(labels == 4)
    assert np.array_equal(p[:, 1], p[:, 4])
    m.close()


@pytest.mark.parametrize("measure", MEASURES)
def test_knn_predict_is_the_vote_on_the_devices_lists(hip, measure):
    K, C, N, top = 17, 5, N_MAX, 7
    g = _case(K, N)
    m = _model(K)
    ix = _filled(m, measure, g)
    lab = _labels(N, C)
    fresh = _gammas(K, 40, 99)
    for weighting in ("uniform", "similarity"):
        nearest, sim = ix.nearest_neighbors(top_n=top, return_similarity=True)
        want = ch.knn_predict(nearest, sim, lab, C, weighting)
        got = ix.knn_predict(lab, top_n=top, weighting=weighting, num_classes=C, return_votes=True)
        assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert not np.any(nearest == np.arange(N)[:, None])           # (leave-one-out: the own id is not a neighbour)
        ids = np.array([5, N - 1, 5, 0])
        some = ix.knn_predict(lab, ids=ids, top_n=top, weighting=weighting, num_classes=C)
        assert np.array_equal(some, want[0][ids])
        nearest, sim = ix.query_gamma(fresh, top_n=top, return_similarity=True)
        want = ch.knn_predict(nearest, sim, lab, C, weighting)
        got = ix.knn_predict(lab, gamma=fresh, top_n=top, weighting=weighting, num_classes=C, return_votes=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        if weighting == "uniform":
            assert np.array_equal(got[1], np.round(got[1])) and got[1].sum(axis=1).max() <= top
    none = ix.knn_predict(np.where(np.arange(N) < 2, lab[:N] * 0, -1), top_n=1, num_classes=2)
    assert np.count_nonzero(none == -1) > 0 and set(none.tolist()) <= {-1, 0}
    m.close()


# -- the buffers and the errors ----------------------------------------------------------------------------
def test_no_buffer_is_kept_by_the_calls(hip):
    """A fresh process (the count is the process's): the calls, the refused and the interrupted ones
    included, leave the live count as it was, and after close() the library holds no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "classify_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout


def test_errors_come_before_anything_runs(hip):
    import trlda_amd
    from trlda_amd import _ffi
    K, N, C = 8, 12, 3
    m = _model(K)
    ix = m.document_index("cosine")
    trlda_amd.seed(3)
    before = _state()
    f = np.full(256 * K, -7.0)
    cnt = np.full(256, -7, dtype=np.int64)
    out = np.full(N, -7, dtype=np.int32)
    lab = (np.arange(N) % C).astype(np.int32)
    W = np.ascontiguousarray(_coef(C, K))
    g = _case(K, N)
    ids = np.arange(3, dtype=np.int64)
    p, null = f.ctypes.data, None

    def fit_set(labels, classes, weights=null, omega=p, counts=cnt.ctypes.data):
        return hip.trlda_docindex_classify_set(ix._handle, labels, classes, weights, omega, counts)

    def predict(coef, classes, gamma=null, M=0, rows=null, labels=out.ctypes.data):
        return hip.trlda_docindex_classify_predict(ix._handle, coef, classes, gamma, M, rows, labels, null)

    # an empty index
    assert fit_set(lab.ctypes.data, C) == _ffi.ERR_ARG and predict(W.ctypes.data, C) == _ffi.ERR_ARG
    with pytest.raises(RuntimeError, match="empty"):
        ix.fit_classifier(np.zeros(0, dtype=int))
    with pytest.raises(RuntimeError, match="empty"):
        ix.predict(W)
    ix.add_gamma(g)
    # NULL arguments, C out of range, an evaluation without labels, ids with a gamma
    assert fit_set(null, C) == _ffi.ERR_ARG and fit_set(lab.ctypes.data, C, omega=null) == _ffi.ERR_ARG
    assert fit_set(lab.ctypes.data, C, counts=null) == _ffi.ERR_ARG
    for bad in (1, 0, -2, 129):
        assert fit_set(lab.ctypes.data, bad) == _ffi.ERR_ARG and predict(W.ctypes.data, bad) == _ffi.ERR_ARG
    assert hip.trlda_docindex_classify_eval(ix._handle, W.ctypes.data, p, p) == _ffi.ERR_ARG
    assert predict(null, C) == _ffi.ERR_ARG and predict(W.ctypes.data, C, labels=null) == _ffi.ERR_ARG
    assert predict(W.ctypes.data, C, gamma=g.ctypes.data, M=3, rows=ids.ctypes.data) == _ffi.ERR_ARG
    assert predict(W.ctypes.data, C, gamma=g.ctypes.data, M=0) == _ffi.ERR_ARG
    assert hip.trlda_docindex_set_classify_slab(ix._handle, -64) == _ffi.ERR_ARG
    # values: labels, weights, coefficients, ids, gamma
    for value in (-2, C):
        bad = lab.copy()
        bad[5] = value
        assert fit_set(bad.ctypes.data, C) == _ffi.ERR_VALUE
    for value in (-1.0, np.nan, np.inf):
        bad = np.ones(N)
        bad[7] = value
        assert fit_set(lab.ctypes.data, C, weights=bad.ctypes.data) == _ffi.ERR_VALUE
    assert fit_set(lab.ctypes.data, C) == _ffi.OK
    assert hip.trlda_docindex_set_classify_slab(ix._handle, 64) == _ffi.ERR_ARG     # (while labels are set)
    for value in (np.nan, np.inf, -np.inf):
        bad = W.copy()
        bad[2, 3] = value
        assert hip.trlda_docindex_classify_eval(ix._handle, bad.ctypes.data, p, p) == _ffi.ERR_VALUE
        assert predict(bad.ctypes.data, C) == _ffi.ERR_VALUE
    assert hip.trlda_docindex_classify_eval(ix._handle, null, p, p) == _ffi.ERR_ARG
    assert hip.trlda_docindex_classify_eval(ix._handle, W.ctypes.data, null, p) == _ffi.ERR_ARG
    ix.add_gamma(g[:, :1])                                            # the index grows under the labels
    assert hip.trlda_docindex_classify_eval(ix._handle, W.ctypes.data, p, p) == _ffi.ERR_ARG
    assert hip.trlda_docindex_classify_clear(ix._handle) == _ffi.OK
    assert hip.trlda_docindex_classify_clear(ix._handle) == _ffi.OK                 # (nothing is kept: still fine)
    N1 = N + 1
    for value in (-1, N1):
        bad = ids.copy()
        bad[1] = value
        assert predict(W.ctypes.data, C, M=3, rows=bad.ctypes.data) == _ffi.ERR_VALUE
    bad = g.copy(order="F")
    bad[2, 1] = 0.0
    assert predict(W.ctypes.data, C, gamma=bad.ctypes.data, M=3) == _ffi.ERR_VALUE
    # nothing was written
    f[0] = -7.0                                                       # (the one set that succeeded wrote its sums)
    cnt[:C] = -7
    assert np.all(f == -7.0) and np.all(cnt == -7) and np.all(out == -7)
    # the Python forms
    lab1 = np.append(lab, 0)
    for classes in (1, 129):
        with pytest.raises(RuntimeError, match="num_classes"):
            ix.fit_classifier(lab1, num_classes=classes)
    with pytest.raises(ValueError, match="labels"):
        ix.fit_classifier(lab1, num_classes=2)                        # a label >= C
    nan = W.copy()
    nan[0, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        ix.classifier_loss(nan, lab1)
    with pytest.raises(ValueError, match="finite"):
        ix.predict(nan)
    for bad in (W[:, :-1], W.T, W[:2]):
        with pytest.raises(RuntimeError, match="coef"):
            ix.classifier_loss(bad, lab1)
    with pytest.raises(RuntimeError):
        ix.predict(W[:, :-1])
    with pytest.raises(ValueError, match="not both"):
        ix.predict(W, gamma=g, ids=ids)
    with pytest.raises(ValueError, match="l2"):
        ix.fit_classifier(lab1, l2=0)
    with pytest.raises(RuntimeError):
        ix.predict(W, ids=[N1])
    # nothing was drawn, and the index still works after the refusals
    assert len(ix) == N1 and np.array_equal(before, _state())
    fit = ix.fit_classifier(lab1)
    assert np.array_equal(fit["counts"], np.bincount(lab1, minlength=C)) and fit["nobs"] == N1
    assert ix.predict(fit["coef"]).shape == (N1,)
    ix.close()
    for call in (lambda: ix.fit_classifier(lab1), lambda: ix.classifier_loss(W, lab1), lambda: ix.predict(W),
                 lambda: ix.knn_predict(lab1), lambda: ix.set_classify_slab(0)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    m.close()
