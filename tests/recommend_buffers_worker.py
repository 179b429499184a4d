"""Child process of tests/test_gpu_recommend.py: after recommend, recommend_gamma (with and without
seen words, two slab widths, both query kernels) and recall_at, and close(), the library holds no
device buffer: an exact zero, counted by trlda_debug_device_buffers (the count is the process's,
hence a process of its own)."""
import ctypes as C
import gc
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd.documents import CSRDocuments                          # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402
from trlda_amd.utils.synthetic import make_corpus                     # noqa: E402

K, V, B = 16, 500, 32


def counts():
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return live.value, total.value


def main():
    _ffi.require_gpu()
    assert counts() == (0, 0), counts()
    docs = CSRDocuments(*make_corpus(B, V, seed=7, mean_unique=40))
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    batch = model.upload(docs)
    words, probs, gamma = model.recommend(batch, top_n=10, latents=np.ones((K, B)), return_gamma=True)
    _ffi.check(_ffi.lib().trlda_model_set_recommend_slab_words(model._handle, 64))
    again = model.recommend_gamma(gamma, top_n=10, docs=batch)
    assert np.array_equal(words, again[0]) and np.array_equal(probs, again[1])
    every, _ = model.recommend_gamma(gamma, top_n=100)
    assert every.shape == (B, 100) and np.all(every >= 0)
    recall = model.recall_at(docs.slice(0, 16), docs.slice(16, 32), top_n=20, latents=np.ones((K, 16)))
    assert 0.0 <= recall <= 1.0
    live = counts()[0]
    batch.close()
    model.close()
    del batch, model
    gc.collect()
    after = counts()
    print("%d buffers live while open, %d made, %d live after close" % (live, after[1], after[0]))
    assert live > 0 and after[0] == 0, (live, after)
    print("buffers ok")


if __name__ == "__main__":
    main()
