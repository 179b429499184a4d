"""Child process of tests/test_gpu_querylik.py: query_likelihood of both measures with B = 1 and
B = 12 keeps no device buffer -- the live count of trlda_debug_device_buffers is the same before and
after the calls, the row sums of lambda apart, which the model keeps -- and after close() the library
holds none: an exact zero (the count is the process's, hence a process of its own)."""
import ctypes as C
import gc
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402

K, V, N = 65, 40, 300
LENGTHS = [1, 2, 3, 5, 15, 16, 17, 31, 33, 40, 1, 4]


def counts():
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return live.value, total.value


def main():
    _ffi.require_gpu()
    assert counts() == (0, 0), counts()
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    rng = np.random.RandomState(5)
    gamma = np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, N)) + 0.01)
    queries = [[(int(w), int(c)) for w, c in zip(rng.choice(V, n, replace=False), rng.randint(1, 5, size=n))]
               for n in LENGTHS]
    indexes = [model.document_index(measure) for measure in ("hellinger", "cosine")]
    for ix in indexes:
        ix.add_gamma(gamma)
    indexes[0].query_likelihood(queries[:1], top_n=1)                 # (the model's row-sum scratch is made)
    live, made = counts()
    for ix in indexes:
        for B in (1, 12):
            ids, s = ix.query_likelihood(queries[:B], top_n=100)
            assert ids.shape == (B, 100) and np.all(np.diff(s, axis=1) <= 0)
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
