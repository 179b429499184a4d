"""Child process of tests/test_gpu_cluster.py: cluster and nearest_centroid of both measures keep no
device buffer -- the live count of trlda_debug_device_buffers is the same before and after the calls,
the refused ones included -- and after close() the library holds none: an exact zero (the count is the
process's, hence a process of its own)."""
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
    gamma = np.asfortranarray(np.random.RandomState(5).gamma(0.3, 1.0, size=(K, N)) + 0.01)
    indexes = [model.document_index(measure) for measure in ("hellinger", "cosine")]
    for ix in indexes:
        ix.add_gamma(gamma)
    live, made = counts()
    for ix in indexes:
        labels, centroids, info = ix.cluster(7, init=list(range(0, N, 43)), return_info=True)
        assert labels.shape == (N,) and info["sizes"].sum() == N
        assert counts()[0] == live, (counts(), live)
        again, sim = ix.nearest_centroid(centroids, return_similarity=True)
        # (the rows are formed again from the returned proportions: the same within rounding)
        assert np.array_equal(again, labels) and np.max(np.abs(sim - info["similarity"])) < 1e-12
        new = ix.nearest_centroid(centroids, gamma=gamma[:, :9])
        assert np.array_equal(new, labels[:9])
        assert counts()[0] == live, (counts(), live)
        bad = centroids.copy(order="F")
        bad[3, 2] = 0.0
        refused(lambda: ix.cluster(7, init=bad), _ffi.TrldaError)
        refused(lambda: ix.nearest_centroid(bad), _ffi.TrldaError)
        refused(lambda: ix.nearest_centroid(centroids, gamma=bad), _ffi.TrldaError)
        refused(lambda: ix.cluster(N + 1), RuntimeError)
        refused(lambda: ix.cluster(7, max_iter=-1), ValueError)
        refused(lambda: ix.cluster(2, init=[4, 4]), ValueError)
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
