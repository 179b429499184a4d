"""Child process of tests/test_gpu_anchor.py: after word_cooccurrence over a stream, anchor_words,
recover_topics (G in LDS and in global memory), initialize_spectral, a loaded matrix and close(), the
library holds no device buffer: an exact zero, counted by trlda_debug_device_buffers (the count is
the process's, hence a process of its own)."""
import ctypes as C
import gc
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trlda_amd import WordCooccurrence, _ffi                          # noqa: E402
from trlda_amd.documents import CSRDocuments                          # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402
from trlda_amd.utils.synthetic import make_corpus                     # noqa: E402

K, V, B = 5, 90, 200


def counts():
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return live.value, total.value


def main():
    _ffi.require_gpu()
    assert counts() == (0, 0), counts()
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    csr = CSRDocuments(*make_corpus(B, V, seed=4, mean_unique=20))
    cooc = model.word_cooccurrence(iter([csr.slice(0, 120), csr.slice(120, B)]))
    anchors = model.anchor_words(cooc)
    for mode in (0, 1):
        cooc._set_gram_lds(mode)
        beta, pi = model.recover_topics(cooc, anchors)
        assert np.isfinite(beta).all() and abs(pi.sum() - 1) < 1e-12
    model.initialize_spectral(csr)
    loaded = WordCooccurrence.from_matrix(model, cooc.read(), doc_freq=cooc.doc_freq)
    assert np.array_equal(model.anchor_words(loaded), anchors)
    try:
        cooc.add(CSRDocuments([0, 2], [1, 1], [1, 1]))                # refused: nothing may leak
    except RuntimeError:
        pass
    live = counts()[0]
    loaded.close()                                                    # one by hand, one with the model
    model.close()
    del model, cooc, loaded
    gc.collect()
    after = counts()
    print("%d buffers live while open, %d made, %d live after close" % (live, after[1], after[0]))
    assert live > 0 and after[0] == 0, (live, after)
    print("buffers ok")


if __name__ == "__main__":
    main()
