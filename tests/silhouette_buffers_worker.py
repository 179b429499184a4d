"""Child process of tests/test_gpu_silhouette.py: silhouette and select_num_clusters of both measures
keep no device buffer -- the live count of trlda_debug_device_buffers is the same before and after the
calls, the refused ones included -- and after close() the library holds none: an exact zero (the count
is the process's, hence a process of its own)."""
import ctypes as C
import gc
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trlda_amd                                                      # noqa: E402
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
    gamma = np.asfortranarray(np.random.RandomState(5).gamma(0.3, 1.0, size=(K, N)) + 0.01)
    indexes = [model.document_index(measure) for measure in ("hellinger", "cosine")]
    for ix in indexes:
        ix.add_gamma(gamma)
    live, made = counts()
    labels = (np.arange(N) % 7).astype(np.int32)
    trlda_amd.seed(4)
    for ix in indexes:
        s, a, b, neighbour = ix.silhouette(labels, return_parts=True)
        assert s.shape == a.shape == b.shape == neighbour.shape == (N,) and np.all(np.abs(s) <= 1)
        assert counts()[0] == live, (counts(), live)
        part = ix.silhouette(labels, ids=[5, 299, 5])
        assert np.array_equal(part, s[[5, 299, 5]])
        assert counts()[0] == live, (counts(), live)
        best, scores = ix.select_num_clusters((2, 5), max_iter=3, ids=np.arange(0, N, 3))
        assert best in scores and len(scores) == 2
        assert counts()[0] == live, (counts(), live)
        refused(lambda: ix.silhouette(np.zeros(N, dtype=np.int32)), ValueError)
        refused(lambda: ix.silhouette(labels[:-1]), RuntimeError)
        refused(lambda: ix.silhouette(labels - 1), RuntimeError)
        refused(lambda: ix.silhouette(labels * 1000), RuntimeError)
        refused(lambda: ix.silhouette(labels.astype(np.float64)), TypeError)
        refused(lambda: ix.silhouette(labels, ids=[N]), RuntimeError)
        # the library's own refusals, past the Python checks
        out = np.empty(N)
        bad = labels.copy()
        bad[3] = 7
        lib = _ffi.lib()
        assert lib.trlda_docindex_silhouette(ix._handle, bad.ctypes.data, 7, None, 0, out.ctypes.data, None, None,
                                             None) == _ffi.ERR_VALUE
        assert lib.trlda_docindex_silhouette(ix._handle, labels.ctypes.data, 1, None, 0, out.ctypes.data, None, None,
                                             None) == _ffi.ERR_ARG
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
