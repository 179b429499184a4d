"""Child process of tests/test_gpu_topicdocs.py: topic_documents, topic_covariance and
topic_correlations of both measures (with the automatic and a forced chunk) keep no device buffer --
the live count of trlda_debug_device_buffers is the same before and after the calls -- and after
close() the library holds none: an exact zero (the count is the process's, hence a process of its
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
        ids, theta = ix.topic_documents(100, return_theta=True)
        assert ids.shape == (K, 100) and np.all(np.diff(theta, axis=1) <= 0)
        cov, mean = ix.topic_covariance(return_mean=True)
        assert abs(mean.sum() - 1.0) < 1e-12 and np.array_equal(cov, cov.T)
        ix.set_moment_chunk(40)
        corr = ix.topic_correlations()
        assert np.all(np.diag(corr) == 1.0)
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
