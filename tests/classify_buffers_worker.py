"""Child process of tests/test_gpu_classify.py: classifier_loss, fit_classifier, predict, knn_predict and
the library calls of both measures keep no device buffer -- the live count of trlda_debug_device_buffers
is the same before and after the calls, the refused ones and a fit interrupted from inside the optimiser
included -- and after close() the library holds none: an exact zero (the count is the process's, hence a
process of its own)."""
import ctypes as C
import gc
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd import index as index_module                           # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402

K, V, N, CLASSES = 65, 20, 300, 4


def counts():
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return live.value, total.value


def refused(call, error):
    try:
        call()
    except error:
        return
    raise AssertionError("the call was not refused")


class Interrupted(Exception):
    pass


def interrupting(fun, W0, **kwargs):
    """In place of the optimiser: one evaluation on the device, then an exception."""
    F, grad = fun(W0)
    assert np.isfinite(F) and grad.shape == W0.shape
    raise Interrupted()


def main():
    _ffi.require_gpu()
    assert counts() == (0, 0), counts()
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    rng = np.random.RandomState(5)
    gamma = np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, N)) + 0.01)
    indexes = [model.document_index(measure) for measure in ("hellinger", "cosine")]
    labels = (np.arange(N) % (CLASSES + 1) - 1).astype(np.int32)
    for ix in indexes:
        ix.add_gamma(gamma)
        # (the searches knn_predict runs keep the index's grow-only query workspaces: they are the
        # index's, made by the first search and held until close())
        ix.nearest_neighbors(top_n=10)
        ix.query_gamma(gamma[:, :9], top_n=10)
    live, made = counts()
    lib = _ffi.lib()
    w = rng.uniform(0.0, 3.0, size=N)
    W = np.ascontiguousarray(rng.normal(size=(CLASSES, K)))
    out = np.empty(K * CLASSES)
    cnt = np.empty(CLASSES, dtype=np.int64)
    lab_out = np.empty(N, dtype=np.int32)
    for ix in indexes:
        loss, grad, omega = ix.classifier_loss(W, labels, weights=w)
        assert np.isfinite(loss) and grad.shape == (CLASSES, K) and omega > 0
        assert counts()[0] == live, (counts(), live)
        ix.set_classify_slab(64)
        fit = ix.fit_classifier(labels, weights=w, l2=1e-2, max_iter=5)
        ix.set_classify_slab(0)
        assert fit["coef"].shape == (CLASSES, K) and fit["iterations"] <= 5
        assert counts()[0] == live, (counts(), live)
        pred, proba = ix.predict(fit["coef"], return_proba=True)
        assert pred.shape == (N,) and proba.shape == (N, CLASSES)
        ix.predict(fit["coef"], ids=[3, 1, 3])
        ix.predict(fit["coef"], gamma=gamma[:, :70])
        assert counts()[0] == live, (counts(), live)
        assert ix.knn_predict(labels, top_n=5).shape == (N,)
        assert ix.knn_predict(labels, gamma=gamma[:, :9], weighting="similarity").shape == (9,)
        assert counts()[0] == live, (counts(), live)
        # a fit interrupted by an exception from inside the optimiser: the labels leave the device
        kept = index_module.lbfgs_minimize
        index_module.lbfgs_minimize = interrupting
        try:
            refused(lambda: ix.fit_classifier(labels, weights=w), Interrupted)
        finally:
            index_module.lbfgs_minimize = kept
        assert counts()[0] == live, (counts(), live)
        refused(lambda: ix.fit_classifier(labels, num_classes=2), ValueError)
        refused(lambda: ix.fit_classifier(labels, weights=-w), ValueError)
        refused(lambda: ix.classifier_loss(W[:, :-1], labels), RuntimeError)
        refused(lambda: ix.predict(W, gamma=gamma, ids=[0]), ValueError)
        refused(lambda: ix.predict(W, gamma=-gamma), _ffi.TrldaError)
        # the library's own refusals, past the Python checks
        bad = labels.copy()
        bad[9] = CLASSES
        p, q = out.ctypes.data, cnt.ctypes.data
        assert lib.trlda_docindex_classify_set(ix._handle, bad.ctypes.data, CLASSES, None, p, q) == _ffi.ERR_VALUE
        assert lib.trlda_docindex_classify_set(ix._handle, labels.ctypes.data, 129, None, p, q) == _ffi.ERR_ARG
        heavy = w.copy()
        heavy[4] = np.inf
        assert lib.trlda_docindex_classify_set(ix._handle, labels.ctypes.data, CLASSES, heavy.ctypes.data, p,
                                               cnt.ctypes.data) == _ffi.ERR_VALUE
        assert lib.trlda_docindex_classify_eval(ix._handle, W.ctypes.data, p, p) == _ffi.ERR_ARG       # (no labels)
        assert counts()[0] == live, (counts(), live)
        assert lib.trlda_docindex_classify_set(ix._handle, labels.ctypes.data, CLASSES, None, p, q) == _ffi.OK
        assert counts()[0] > live                                     # (the labels and the scratch are kept ...)
        nan = W.copy()
        nan[1, 1] = np.nan
        assert lib.trlda_docindex_classify_eval(ix._handle, nan.ctypes.data, p, p) == _ffi.ERR_VALUE
        assert lib.trlda_docindex_classify_predict(ix._handle, nan.ctypes.data, CLASSES, None, 0, None,
                                                   lab_out.ctypes.data, None) == _ffi.ERR_VALUE
        assert lib.trlda_docindex_classify_clear(ix._handle) == _ffi.OK
        assert counts()[0] == live, (counts(), live)                  # (... until they are cleared)
    # labels that are still set when the index is closed go with it
    assert lib.trlda_docindex_classify_set(indexes[0]._handle, labels.ctypes.data, CLASSES, None, out.ctypes.data,
                                           cnt.ctypes.data) == _ffi.OK
    assert counts()[1] > made                                         # (the calls did allocate)
    for ix in indexes:
        ix.close()
    model.close()
    del indexes, ix, model
    gc.collect()
    after = counts()
    print("%d buffers live around the calls, %d made, %d live after close" % (live, after[1], after[0]))
    assert live > 0 and after[0] == 0, (live, after)
    print("buffers ok")


if __name__ == "__main__":
    main()
