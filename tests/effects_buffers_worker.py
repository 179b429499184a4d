"""Child process of tests/test_gpu_effects.py: group_prevalence, topic_trends, topic_effects and the three
library calls of both measures keep no device buffer -- the live count of trlda_debug_device_buffers is
the same before and after the calls, the refused ones included -- and after close() the library holds
none: an exact zero (the count is the process's, hence a process of its own)."""
import ctypes as C
import gc
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402

K, V, N = 65, 20, 300


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


def main():
    _ffi.require_gpu()
    assert counts() == (0, 0), counts()
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    rng = np.random.RandomState(5)
    gamma = np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, N)) + 0.01)
    indexes = [model.document_index(measure) for measure in ("hellinger", "cosine")]
    for ix in indexes:
        ix.add_gamma(gamma)
    live, made = counts()
    lib = _ffi.lib()
    labels = (np.arange(N) % 4 - 1).astype(np.int32)
    w = rng.uniform(0.0, 3.0, size=N)
    X = rng.normal(size=(N, 5))
    Z = np.ascontiguousarray(np.hstack([np.ones((N, 1)), X]))
    out = np.empty(K * 8)
    cnt = np.empty(8, dtype=np.int64)
    for ix in indexes:
        mean, members, var = ix.group_prevalence(labels, weights=w, return_variance=True)
        assert mean.shape == var.shape == (K, 3) and members.sum() == np.count_nonzero(labels >= 0)
        assert counts()[0] == live, (counts(), live)
        ix.group_prevalence(labels)
        edges, mean, members = ix.topic_trends(X[:, 0], 5)
        assert mean.shape == (K, 5) and members.sum() == N
        assert counts()[0] == live, (counts(), live)
        fit = ix.topic_effects(X, weights=w)
        assert fit["coef"].shape == (6, K) and np.all(fit["rss"] <= fit["tss"])
        ix.topic_effects(X, intercept=False)
        assert counts()[0] == live, (counts(), live)
        refused(lambda: ix.group_prevalence(labels, num_groups=2), ValueError)
        refused(lambda: ix.group_prevalence(labels, weights=-w), ValueError)
        refused(lambda: ix.topic_effects(X[:-1]), RuntimeError)
        refused(lambda: ix.topic_effects(np.hstack([X, X])), ValueError)          # (refused after the products)
        # the library's own refusals, past the Python checks
        bad = labels.copy()
        bad[9] = 3
        p = out.ctypes.data
        assert lib.trlda_docindex_group_moments(ix._handle, bad.ctypes.data, 3, None, p, p, cnt.ctypes.data,
                                                None) == _ffi.ERR_VALUE
        assert lib.trlda_docindex_group_moments(ix._handle, labels.ctypes.data, 0, None, p, p, cnt.ctypes.data,
                                                None) == _ffi.ERR_ARG
        heavy = w.copy()
        heavy[4] = np.inf
        assert lib.trlda_docindex_regress_products(ix._handle, Z.ctypes.data, 6, heavy.ctypes.data, p, p) == _ffi.ERR_VALUE
        assert lib.trlda_docindex_regress_products(ix._handle, Z.ctypes.data, 257, None, p, p) == _ffi.ERR_ARG
        assert lib.trlda_docindex_regress_residuals(ix._handle, Z.ctypes.data, 6, None, None, p) == _ffi.ERR_ARG
        assert counts()[0] == live, (counts(), live)
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
