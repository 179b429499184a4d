"""Child process of tests/test_gpu_diagnostics.py: after topic_word_diagnostics (default and given
weights, the model's and given lists, several chunks of the vocabulary), topic_document_diagnostics in
both forms over an iterator of batches, topic_diagnostics, and close(), the library holds no device
buffer: an exact zero, counted by trlda_debug_device_buffers (the count is the process's, hence a
process of its own)."""
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

K, V, B = 16, 3000, 32                   # 12 chunks of 256 words


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
    d = model.topic_document_diagnostics(iter([batch, docs.slice(0, 16)]), latents=np.ones((K, B + 16)), max_iter=10)
    assert d["num_docs"] == B + 16 and d["rank_1_docs"].sum() == B + 16
    assert abs(d["tokens"].sum() - (docs.cnts.sum() + docs.slice(0, 16).cnts.sum())) < 1e-9 * d["tokens"].sum()
    gamma, _ = model.update_variables(batch, latents=np.ones((K, B)), max_iter=10)
    again = model.topic_document_diagnostics_gamma(gamma, iter([docs.slice(0, 16), docs.slice(16, B)]),
                                                   weight_by_length=False)
    assert again["num_docs"] == B and abs(again["tokens"].sum() - B) < 1e-12 * B
    pi = d["tokens"] / d["tokens"].sum()
    w = model.topic_word_diagnostics(100, topic_weights=pi)
    assert np.array_equal(w["top_words"], model.top_words(100))
    assert np.all(w["eff_num_words"] >= 1) and np.all(w["eff_num_words"] <= V) and np.all(w["corpus_dist"] >= 0)
    assert np.all(w["exclusivity"] > 0) and np.all(w["exclusivity"] <= 1)
    mine = model.topic_word_diagnostics(words=model.relevant_words(10, 0.3))
    assert mine["top_words"].shape == (K, 10)
    both = model.topic_diagnostics(batch, latents=np.ones((K, B)), max_iter=10, top_n=5)
    assert both["top_words"].shape == (K, 5) and both["num_docs"] == B
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
