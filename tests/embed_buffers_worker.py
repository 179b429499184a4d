"""Child process of tests/test_gpu_embed.py: nearest_neighbors, affinities, embedding_gradient and embed
of both measures keep no device buffer beyond the index's grow-only query workspaces -- the live count
of trlda_debug_device_buffers is the same before and after the calls, the refused ones included -- and
after close() the library holds none: an exact zero (the count is the process's, hence a process of its
own)."""
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
        ix.nearest_neighbors(99)                                      # (the query workspaces, at their largest)
    live, made = counts()
    for ix in indexes:
        ids, dist = ix.nearest_neighbors(10)
        assert ids.shape == dist.shape == (N, 10)
        assert counts()[0] == live, (counts(), live)
        aff = ix.affinities(10.0)
        ix.affinities(33.0, return_conditional=True)
        assert counts()[0] == live, (counts(), live)
        Y, info = ix.embed(num_iterations=30, exaggeration_iterations=10, affinities=aff, return_info=True)
        grad, kl = ix.embedding_gradient(Y, aff)
        assert Y.shape == grad.shape == (N, 2) and abs(kl - info["kl"][-1]) < 1.0
        assert counts()[0] == live, (counts(), live)
        refused(lambda: ix.nearest_neighbors(N), RuntimeError)
        refused(lambda: ix.affinities(40.0), ValueError)
        refused(lambda: ix.embed(init=Y[:-1]), ValueError)
        refused(lambda: ix.embedding_gradient(Y, (aff[0][:-1], aff[1], aff[2])), ValueError)
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
