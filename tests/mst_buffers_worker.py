"""Child process of tests/test_gpu_mst.py: spanning_tree, single_linkage, hdbscan and the sweep of both
measures keep no device buffer -- the live count of trlda_debug_device_buffers is the same before and
after the calls, the refused ones included -- and after close() the library holds none: an exact zero
(the count is the process's, hence a process of its own)."""
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
        ix.nearest_neighbors(4)                                       # (the index's grow-only query workspaces)
    live, made = counts()
    lib = _ffi.lib()
    for ix in indexes:
        u, v, w = ix.spanning_tree()
        assert u.shape == v.shape == w.shape == (N - 1,)
        assert counts()[0] == live, (counts(), live)
        u, v, w, core = ix.spanning_tree(5, return_core=True)
        assert core.shape == (N,) and np.all(w >= core[u]) and np.all(w >= core[v])
        assert counts()[0] == live, (counts(), live)
        Z = ix.single_linkage(3)
        assert Z.shape == (N - 1, 4) and len(np.unique(ix.cut_linkage(Z, num_clusters=4))) == 4
        labels = ix.hdbscan(min_cluster_size=4)
        assert labels.shape == (N,)
        assert counts()[0] == live, (counts(), live)
        refused(lambda: ix.spanning_tree(0), RuntimeError)
        refused(lambda: ix.spanning_tree(101), RuntimeError)
        refused(lambda: ix.hdbscan(selection="best"), ValueError)
        # the library's own refusals, past the Python checks
        comp = np.zeros(N, dtype=np.int32)
        best, weight = np.empty(N, dtype=np.int64), np.empty(N)
        bad = np.full(N, -1.0)
        assert lib.trlda_docindex_mst_sweep(ix._handle, comp.ctypes.data, bad.ctypes.data, best.ctypes.data,
                                            weight.ctypes.data) == _ffi.ERR_VALUE
        assert lib.trlda_docindex_mst_sweep(ix._handle, None, None, best.ctypes.data,
                                            weight.ctypes.data) == _ffi.ERR_ARG
        _ffi.check(lib.trlda_docindex_mst_sweep(ix._handle, comp.ctypes.data, None, best.ctypes.data,
                                                weight.ctypes.data))
        assert np.all(best == -1)
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
