"""Child process of tests/test_gpu_wordsim.py: after similar_words, words_near and
word_topic_proportions under both measures (default and given weights, both widths of the query
kernel, several slabs) and close(), the library holds no device buffer: an exact zero, counted by
trlda_debug_device_buffers (the count is the process's, hence a process of its own)."""
import ctypes as C
import gc
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402

K, V, B = 16, 2100, 70


def counts():
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return live.value, total.value


def main():
    _ffi.require_gpu()
    assert counts() == (0, 0), counts()
    rng = np.random.RandomState(3)
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    model.lambdas = rng.gamma(0.3, 1.0, size=(K, V)) + 0.01
    words = rng.randint(0, V, size=B)
    given = rng.gamma(2.0, 1.0, K) + 0.1
    _ffi.check(_ffi.lib().trlda_model_set_wordsim_slab_words(model._handle, 512))
    for measure in ("hellinger", "cosine"):
        for pi in (None, given):
            for top_n in (10, 100):
                ids, dist = model.similar_words(words, top_n, measure=measure, topic_weights=pi)
                assert ids.shape == dist.shape == (B, top_n) and np.all(np.diff(dist, axis=1) >= 0)
                assert not np.any(ids == words[:, None])
            p = model.word_topic_proportions(words, topic_weights=pi)
            assert p.shape == (K, B) and np.max(np.abs(p.sum(axis=0) - 1.0)) < 1e-13
            near, dist = model.words_near(p, 5, measure=measure, topic_weights=pi)
            assert np.array_equal(near[:, 0], model.similar_words(words, 1, measure=measure, topic_weights=pi,
                                                                  exclude_self=False)[0][:, 0])
    live = counts()[0]
    model.close()
    del model
    gc.collect()
    after = counts()
    print("%d buffers live while open, %d made, %d live after close" % (live, after[1], after[0]))
    assert live > 0 and after[0] == 0, (live, after)
    print("buffers ok")


if __name__ == "__main__":
    main()
