"""CPU checks of the classification of indexed documents from their topic proportions:
the restatement (tests/classify_host.py) against central differences and its own Newton solver, the
package's L-BFGS driven by the restatement in float64, the vote of ``knn_predict`` on hand-made
neighbour lists, and what the library and ``DocumentIndex`` answer before any GPU work."""
import numpy as np
import pytest

import classify_host as ch

LD = np.longdouble
SHAPES = [(3, 2, 40), (6, 3, 120), (17, 5, 200)]


def _theta(N, K, seed):
    g = np.random.RandomState(seed).gamma(0.3, 1.0, size=(K, N)) + 0.01
    return (g / g.sum(axis=0)).T


def _problem(K, C, N, seed=11, weighted=True):
    """theta, labels that depend on theta (with noise, a sixth left out) and weights with zeros."""
    rng = np.random.RandomState(seed + K)
    theta = _theta(N, K, seed)
    true = rng.normal(size=(C, K)) * 6.0
    labels = np.argmax(theta.dot(true.T) + rng.gumbel(size=(N, C)), axis=1)
    labels[rng.permutation(N)[:N // 6]] = -1
    w = None
    if weighted:
        w = rng.uniform(0.5, 3.0, size=N)
        w[::9] = 0.0
    return theta, labels, w


# -- the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_restated_gradient_against_central_differences(weighted):
    K, C, N = 5, 4, 60
    theta, labels, w = _problem(K, C, N, weighted=weighted)
    W = np.random.RandomState(2).normal(size=(C, K))
    F, g = ch.objective(theta, W, labels, w, 1e-2)
    assert g.dtype == LD and g.shape == (C, K)
    h = LD(2.0) ** -24
    for c in range(C):
        for k in range(K):
            E = np.zeros((C, K), dtype=LD)
            E[c, k] = h
            fd = (ch.objective(theta, W.astype(LD) + E, labels, w, 1e-2)[0] -
                  ch.objective(theta, W.astype(LD) - E, labels, w, 1e-2)[0]) / (2 * h)
            assert abs(float(fd - g[c, k])) <= 1e-9, (c, k, float(fd), float(g[c, k]))
    # the unnormalised sums are the same objective without the penalty
    loss, grad, omega = ch.loss_grad(theta, W, labels, w)
    F0, g0 = ch.objective(theta, W, labels, w, 0.0)
    assert abs(float(loss / omega - F0)) <= 1e-17 and np.max(np.abs(grad / omega - g0)) <= 1e-17
    # and the float64 callable agrees with them
    F64, g64 = ch.fun64(theta, labels, w, 1e-2)(W)
    assert abs(F64 - float(F)) <= 1e-13 and np.max(np.abs(g64 - g.astype(np.float64))) <= 1e-13
    # a left-out document and a document of weight 0 add nothing
    f = ch.forward(theta, W, labels, w)
    out = labels < 0 if w is None else (labels < 0) | (w == 0)
    assert np.all(f["r"][out] == 0) and np.all((f["w"] * f["l"])[out] == 0)


@pytest.mark.parametrize("K,C,N", SHAPES)
def test_newton_satisfies_the_first_order_condition(K, C, N):
    theta, labels, w = _problem(K, C, N)
    W, norm = ch.newton(theta, labels, w, 1e-2, C)
    assert W.dtype == LD and norm < 1e-13
    _, g = ch.objective(theta, W, labels, w, 1e-2)
    assert float(np.sqrt((g * g).sum())) < 1e-13
    # the Hessian is that of F: symmetric, and at least l2 everywhere
    H = ch.hessian(theta, np.asarray(W, dtype=np.float64), labels, w, 1e-2)
    assert np.max(np.abs(H - H.T)) <= 1e-15 and np.linalg.eigvalsh(H)[0] >= 1e-2 * (1 - 1e-9)


# -- the optimiser ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,C,N", SHAPES)
def test_lbfgs_reaches_newtons_optimum(K, C, N):
    from trlda_amd.index import lbfgs_minimize
    l2, tol = 1e-2, 1e-9
    theta, labels, w = _problem(K, C, N)
    fun = ch.fun64(theta, labels, w, l2)
    fit = lbfgs_minimize(fun, np.zeros((C, K)), max_iter=200, tol=tol)
    assert fit["converged"] and fit["grad_norm"] <= tol and 1 <= fit["iterations"] <= 200
    assert fit["evaluations"] > fit["iterations"] and fit["coef"].shape == (C, K) and fit["coef"].dtype == np.float64
    W_newton, _ = ch.newton(theta, labels, w, l2, C)
    g = ch.objective(theta, fit["coef"], labels, w, l2)[1]
    g_newton = ch.objective(theta, W_newton, labels, w, l2)[1]
    dist = float(np.sqrt(((fit["coef"].astype(LD) - W_newton) ** 2).sum()))
    bound = float(np.sqrt((g * g).sum()) + np.sqrt((g_newton * g_newton).sum())) / l2
    print("K %d C %d N %d: %d iterations, %d evaluations, |W - W*| %.3g of the bound %.3g"
          % (K, C, N, fit["iterations"], fit["evaluations"], dist, bound))
    assert dist <= bound
    again = lbfgs_minimize(fun, np.zeros((C, K)), max_iter=200, tol=tol)
    assert np.array_equal(again["coef"], fit["coef"]) and again["loss"] == fit["loss"]
    assert again["iterations"] == fit["iterations"] and again["evaluations"] == fit["evaluations"]
    # a converged start returns after its one evaluation
    warm = lbfgs_minimize(fun, fit["coef"], max_iter=200, tol=tol)
    assert warm["converged"] and warm["evaluations"] == 1 and warm["iterations"] == 0
    assert np.array_equal(warm["coef"], fit["coef"])
    # one iteration is not enough, and that is not an error
    short = lbfgs_minimize(fun, np.zeros((C, K)), max_iter=1, tol=tol)
    assert short["converged"] is False and short["iterations"] == 1 and short["grad_norm"] > tol
    assert short["loss"] < fun(np.zeros((C, K)))[0]


def test_lbfgs_on_separable_data_returns_finite_numbers():
    from trlda_amd.index import lbfgs_minimize
    K, C, N = 4, 2, 60
    rng = np.random.RandomState(8)
    labels = np.arange(N) % C
    g = np.full((N, K), 0.01)
    g[np.arange(N), labels] = 5.0 + rng.uniform(size=N)              # each class on its own topic
    theta = g / g.sum(axis=1)[:, None]
    fit = lbfgs_minimize(ch.fun64(theta, labels, None, 1e-8), np.zeros((C, K)), max_iter=200, tol=1e-6)
    assert np.all(np.isfinite(fit["coef"])) and np.isfinite(fit["loss"]) and np.isfinite(fit["grad_norm"])
    assert isinstance(fit["converged"], bool) and fit["loss"] < np.log(2.0)
    assert np.array_equal(np.argmax(theta.dot(fit["coef"].T), axis=1), labels)


def test_lbfgs_stops_when_the_search_cannot_decrease():
    from trlda_amd.index import lbfgs_minimize
    # F's gradient points the wrong way: no step lowers F, and the answer is converged=False, not an error
    fit = lbfgs_minimize(lambda W: (float(np.sum(W * W)), -2.0 * W), np.ones((2, 3)), max_iter=50, tol=1e-9)
    assert fit["converged"] is False and fit["iterations"] == 0 and np.array_equal(fit["coef"], np.ones((2, 3)))


# -- the vote --------------------------------------------------------------------------------------------
def test_knn_votes_on_hand_made_lists():
    from trlda_amd.index import knn_votes
    labels = np.array([0, 1, 1, -1, 2, 0, 2])
    nearest = np.array([[1, 2, 0],        # two votes for 1, one for 0
                        [0, 1, 3],        # a tie of 0 and 1 (document 3 does not vote): the smaller id
                        [3, 3, 3],        # no voter
                        [4, 5, 1],        # a three-way tie: class 0
                        [3, 6, -1],       # one voter, and a missing neighbour
                        [6, 4, 5]])       # two votes for 2
    sim = np.array([[.9, .8, .7], [.9, .8, .7], [.9, .8, .7], [.5, .4, .3], [.9, .2, .1], [.3, .2, .9]])
    pred, votes = knn_votes(nearest, sim, labels, 3, "uniform")
    assert pred.dtype == np.int32 and pred.tolist() == [1, 0, -1, 0, 2, 2]
    assert votes.tolist() == [[1, 2, 0], [1, 1, 0], [0, 0, 0], [1, 1, 1], [0, 0, 1], [1, 0, 2]]
    want, want_votes = ch.knn_predict(nearest, sim, labels, 3, "uniform")
    assert np.array_equal(pred, want) and np.array_equal(votes, want_votes)
    pred, votes = knn_votes(nearest, sim, labels, 3, "similarity")
    # by similarity the single closest neighbour can outvote two others, and the three-way tie is gone
    assert pred.tolist() == [1, 0, -1, 2, 2, 0]
    assert votes[0].tolist() == [.7, .9 + .8, 0.0] and votes[5].tolist() == [.9, 0.0, .3 + .2]
    want, want_votes = ch.knn_predict(nearest, sim, labels, 3, "similarity")
    assert np.array_equal(pred, want) and np.array_equal(votes, want_votes)
    # random lists: the vectorised vote is the brute-force one bit for bit
    rng = np.random.RandomState(3)
    lab = rng.randint(-1, 5, size=40)
    near = rng.randint(-1, 40, size=(25, 7))
    s = rng.uniform(size=(25, 7))
    for weighting in ("uniform", "similarity"):
        a, b = knn_votes(near, s, lab, 5, weighting), ch.knn_predict(near, s, lab, 5, weighting)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# -- the library and the arguments ------------------------------------------------------------------------
def test_classify_entry_points_are_exported(hip_lib):
    from trlda_amd import _ffi
    names = ["trlda_docindex_" + n for n in ("classify_set", "classify_clear", "classify_eval", "classify_predict",
                                             "set_classify_slab")]
    for name in names:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    # (no index: the argument check answers before any device is touched)
    f, i = np.full(8, -7.0), np.full(8, -7, dtype=np.int64)
    lab = np.zeros(4, dtype=np.int32)
    p = f.ctypes.data
    assert hip_lib.trlda_docindex_classify_set(None, lab.ctypes.data, 2, None, p, i.ctypes.data) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_classify_clear(None) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_classify_eval(None, p, p, p) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_classify_predict(None, p, 2, None, 0, None, lab.ctypes.data, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_set_classify_slab(None, 64) == _ffi.ERR_ARG
    assert np.all(f == -7.0) and np.all(i == -7) and np.all(lab == 0)


class _Shell(object):
    """A DocumentIndex without a device side: `n` documents of 3 topics, no handle."""

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
    W = np.zeros((2, 3))
    calls = (lambda l, **kw: x.fit_classifier(l, **kw), lambda l, **kw: x.classifier_loss(kw.pop("coef", W), l, **kw),
             lambda l, **kw: x.knn_predict(l, **kw))
    for call in calls:
        for bad in (lab.astype(np.float64), "01011", None):
            with pytest.raises(TypeError):
                call(bad)
        for bad in (lab[:4], lab.reshape(5, 1)):
            with pytest.raises(RuntimeError, match="labels"):
                call(bad)
        for classes in (1, 0, 129):
            with pytest.raises(RuntimeError, match="num_classes"):
                call(lab, num_classes=classes)
        with pytest.raises(RuntimeError, match="num_classes"):
            call(np.array([0, 0, -1, 0, 0]))                          # (one class: C = 1)
        with pytest.raises(RuntimeError, match="num_classes"):
            call(np.array([0, 1, 2, 3, 128]))
        for bad in (np.array([0, 1, -2, 1, 0]), np.array([0, 1, 2, 1, 0])):
            with pytest.raises(ValueError, match="labels"):
                call(bad, num_classes=2)
    with pytest.raises(RuntimeError, match="empty"):
        _Shell(0).fit_classifier(np.zeros(0, dtype=int))
    for call in calls[:2]:
        for bad in ([1.0, 2.0, np.nan, 1.0, 1.0], [1.0, -1.0, 1.0, 1.0, 1.0], np.zeros(5)):
            with pytest.raises(ValueError, match="weights"):
                call(lab, weights=bad)
        with pytest.raises(RuntimeError, match="weights"):
            call(lab, weights=np.ones(4))
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="l2"):
            x.fit_classifier(lab, l2=bad)
    with pytest.raises(ValueError, match="positive weight"):
        x.fit_classifier(lab, weights=[0.0, 0.0, 5.0, 0.0, 0.0])       # (the only weight is a left-out document's)
    with pytest.raises(ValueError):
        x.fit_classifier(lab, max_iter=-1)
    # coefficients
    for bad in (np.zeros((2, 4)), np.zeros((3, 3)), np.zeros(6), np.zeros((2, 3, 1))):
        with pytest.raises(RuntimeError, match="coef"):
            x.classifier_loss(bad, lab)
        with pytest.raises(RuntimeError, match="coef"):
            x.fit_classifier(lab, init=bad)
    for bad in (np.zeros((1, 3)), np.zeros((129, 3)), np.zeros((2, 4))):
        with pytest.raises(RuntimeError):
            x.predict(bad)
    nan = W.copy()
    nan[1, 2] = np.nan
    for call in (lambda: x.classifier_loss(nan, lab), lambda: x.fit_classifier(lab, init=nan), lambda: x.predict(nan)):
        with pytest.raises(ValueError, match="coef"):
            call()
    with pytest.raises(TypeError):
        x.predict("abc")
    with pytest.raises(ValueError, match="not both"):
        x.predict(W, gamma=np.ones((3, 1)), ids=[0])
    with pytest.raises(ValueError, match="not both"):
        x.knn_predict(lab, gamma=np.ones((3, 1)), ids=[0])
    with pytest.raises(ValueError, match="weighting"):
        x.knn_predict(lab, weighting="rank")
    # and with the arguments in order it is the missing device side that answers
    for call in (lambda: x.fit_classifier(lab), lambda: x.classifier_loss(W, lab), lambda: x.predict(W),
                 lambda: x.knn_predict(lab), lambda: x.set_classify_slab(64)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
