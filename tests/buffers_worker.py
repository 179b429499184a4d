"""Child process of tests/test_gpu_buffers.py: every device buffer the library owns (DevBuf,
csrc/trlda_hip.hip) is released when its owner is closed.  Started with TRLDA_MERGED_STAMPS=1 (read once
per process), so that the launches' diagnostic stamps buffers -- which once leaked -- exist too.

Two rounds of: a model at smoke()'s shapes (K = 16, V = 500, batches of 32 documents) driven through
every entry point that has a workspace of its own, a document index at K = 8 that crosses one growth
copy (300, then 1800 rows: 1024 -> 4096), everything closed through the package's own close paths.
The count of live buffers is exactly 0 before, between and after.  Prints one line per round."""
import ctypes as C
import gc
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trlda_amd                                                      # noqa: E402
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd.documents import CSRDocuments                          # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402
from trlda_amd.utils.synthetic import make_corpus                     # noqa: E402

K, V, B, D = 16, 500, 32, 1000


def counts():
    live, total = C.c_longlong(-1), C.c_longlong(-1)
    _ffi.check(_ffi.lib().trlda_debug_device_buffers(C.byref(live), C.byref(total)))
    return live.value, total.value


def stream_of_esteps(model, batches, g0):
    """smoke()'s stream: four E-steps on a fixed lambda over two batches, statistics deferred into the
    next launch, two lanes.  The callers' arrays are trlda_dev_alloc's: theirs, not counted."""
    L = _ffi.lib()
    ptrs = []
    for c in range(4):
        p = [_ffi.vp() for _ in range(3)]
        for q, nbytes in zip(p, (K * B * 8, K * B * 8, K * V * 8)):
            _ffi.check(L.trlda_dev_alloc(0, nbytes, C.byref(q)))
        _ffi.check(L.trlda_dev_upload(0, p[0], g0.ctypes.data, g0.nbytes))
        ptrs.append(p)
    _ffi.check(L.trlda_model_set_deferred_stats(model._handle, 1))
    _ffi.check(L.trlda_model_set_stream_lanes(model._handle, 2))
    up = (C.c_void_p * 2)()
    for c in range(4):
        up[0], up[1] = batches[(c + 1) % 2].handle.value, batches[c % 2].handle.value
        _ffi.check(L.trlda_model_estep_io_ahead(model._handle, batches[c % 2].handle, up, min(2, 3 - c),
                                                ptrs[c][0], ptrs[c][1], ptrs[c][2], 20, 1e-3, None))
    _ffi.check(L.trlda_model_synchronize(model._handle))
    for p in ptrs:
        for q in p:
            _ffi.check(L.trlda_dev_free(0, q))
    _ffi.check(L.trlda_model_set_stream_lanes(model._handle, 1))
    _ffi.check(L.trlda_model_set_deferred_stats(model._handle, 0))


def drive():
    """Step 2 to 5: make, use and close; returns the live count while everything was open."""
    L = _ffi.lib()
    trlda_amd.seed(11)
    docs = CSRDocuments(*make_corpus(B, V, seed=7, mean_unique=40))
    more = CSRDocuments(*make_corpus(B, V, seed=8, mean_unique=40))
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=D, alpha=.1, eta=.3, device=0)
    lam0 = np.array(model.lambdas)
    g0 = np.asfortranarray(np.random.RandomState(12).gamma(1.0, 1.0, size=(K, B)) + 0.1)
    model.do_e_step(docs, latents=g0, max_iter=20)
    model.update_parameters(docs, max_iter_tr=2, max_iter_inference=20)
    # (an E-step with the merged launch asked for, as tools/merged_stamps.py: its stamps buffer exists
    # whatever update_parameters chose)
    _ffi.check(L.trlda_model_set_merged_launch(model._handle, 2))
    model.update_variables(docs, latents=g0, max_iter=20)
    _ffi.check(L.trlda_model_set_merged_launch(model._handle, 1))
    model.lambdas = lam0
    batches = [model.upload(docs), model.upload(more)]
    stream_of_esteps(model, batches, g0)
    model.update_variables(docs, inference_method='gibbs', num_samples=2, burn_in=1)
    model.sample(B, 20, return_theta=True)
    model.predictive_log_likelihood(batches[0], batches[1], latents=g0, max_iter=20)
    model.document_log_likelihood(batches[0], num_samples=32, latents=g0, max_iter=20)
    model.left_to_right(batches[0], num_particles=4)
    model.word_topics(batches[0], top_n=2, latents=g0, max_iter=20)
    model.top_words(5)
    model.topic_coherence(batches[0], top_n=5)                       # (makes and closes its accumulator)
    stamps = np.zeros(3 * 1024, dtype=np.uint64)
    _ffi.check(L.trlda_debug_merged_stamps(model._handle, stamps.ctypes.data))

    small = OnlineLDA(num_words=V, num_topics=8, num_documents=D, alpha=.1, eta=.3, device=0)
    rows = np.asfortranarray(np.random.RandomState(11).gamma(0.3, 1.0, size=(8, 2100)) + 0.01)
    index = small.document_index()
    assert index.add_gamma(rows[:, :300]) == 0
    assert index.add_gamma(rows[:, 300:]) == 300                     # 1024 rows -> 4096: the growth copy
    assert index.add(docs, max_iter=20) == 2100
    ids, _ = index.query(docs, top_n=5, max_iter=20)
    assert ids.shape == (B, 5) and len(index) == 2100 + B
    assert np.array_equal(index.rows(0, 2100), index.rows()[:2100])

    live = counts()[0]
    index.close()
    for b in batches:
        b.close()
    small.close()
    model.close()
    del index, batches, small, model
    gc.collect()
    return live


def main():
    _ffi.require_gpu()
    assert os.environ.get("TRLDA_MERGED_STAMPS"), "start me with TRLDA_MERGED_STAMPS=1"
    assert counts() == (0, 0), counts()
    made = []
    for rnd in range(2):
        before = counts()[1]
        live = drive()
        after = counts()
        made.append(after[1] - before)
        print("round %d: %d buffers live while open, %d made, %d live after close" % (rnd, live, made[-1], after[0]))
        assert live > 0, live
        assert after[0] == 0, after
    # the second round makes what the first did (the same calls on the same shapes; only what a process
    # learns once -- whether two lanes' streams overlap -- may differ): the total roughly doubled
    assert abs(made[1] - made[0]) <= made[0] // 10, made
    print("buffers ok")


if __name__ == "__main__":
    main()
