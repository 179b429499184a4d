"""Child process of tests/test_gpu_ranks.py: after heldout_ranks, heldout_ranks_gamma (with and without
seen words, two slab widths, two threshold chunks) and ranking_metrics, and close(), the library holds
no device buffer: an exact zero, counted by trlda_debug_device_buffers (the count is the process's,
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


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def main():
    _ffi.require_gpu()
    assert counts() == (0, 0), counts()
    docs = CSRDocuments(*make_corpus(2 * B, V, seed=7, mean_unique=40))
    observed, heldout = docs.slice(0, B), docs.slice(B, 2 * B)
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    o_batch, h_batch = model.upload(observed), model.upload(heldout)
    out = model.heldout_ranks(o_batch, h_batch, latents=np.ones((K, B)), return_scores=True, return_gamma=True)
    assert len(out[1]) > 0 and np.all(out[2] >= 1)
    _ffi.check(_ffi.lib().trlda_model_set_recommend_slab_words(model._handle, 64))
    _ffi.check(_ffi.lib().trlda_model_set_ranks_chunk(model._handle, 5))
    assert same(model.heldout_ranks_gamma(out[5], h_batch, docs=o_batch, return_scores=True), out[:5])
    every = model.heldout_ranks_gamma(out[5], heldout)
    assert np.all(every[3] == V)
    figures = model.ranking_metrics(observed, heldout, top_n=(20, 200), latents=np.ones((K, B)))
    assert 0.0 <= figures["recall"][20] <= figures["recall"][200] <= 1.0
    live = counts()[0]
    o_batch.close()
    h_batch.close()
    model.close()
    del o_batch, h_batch, model
    gc.collect()
    after = counts()
    print("%d buffers live while open, %d made, %d live after close" % (live, after[1], after[0]))
    assert live > 0 and after[0] == 0, (live, after)
    print("buffers ok")


if __name__ == "__main__":
    main()
