"""Child process of tests/test_gpu_relevance.py: after relevant_words, word_statistics, salient_words
(default and given weights, one tile and several levels of the selection), topic_prevalence in both
forms over an iterator of batches, and close(), the library holds no device buffer: an exact zero,
counted by trlda_debug_device_buffers (the count is the process's, hence a process of its own)."""
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

K, V, B = 16, 12000, 32                  # 12 tiles x 100 candidates: a middle level of the selection


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
    pi = model.topic_prevalence(iter([batch, docs.slice(0, 16)]), latents=np.ones((K, B + 16)), max_iter=10)
    assert pi.shape == (K,) and abs(pi.sum() - 1.0) < 1e-14
    gamma, _ = model.update_variables(batch, latents=np.ones((K, B)), max_iter=10)
    again = model.topic_prevalence_gamma(gamma, batch, weight_by_length=False)
    assert again.shape == (K,)
    words, scores = model.relevant_words(100, 0.6, topic_weights=pi, return_scores=True)
    assert words.shape == (K, 100) and np.all(np.diff(scores, axis=1) <= 0)
    assert np.array_equal(model.relevant_words(100, 1.0), model.top_words(100))
    p, d, s = model.word_statistics()
    assert abs(p.sum() - 1.0) < 1e-12 and np.all(d >= 0) and p.shape == (V,)
    sal, val = model.salient_words(100, topic_weights=pi)
    assert len(set(sal)) == 100 and np.all(np.diff(val) <= 0)
    assert np.array_equal(model.salient_words(5)[0], np.lexsort((np.arange(V), -s))[:5])
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
