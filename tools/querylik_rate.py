"""Whole-call times of DocumentIndex.query_likelihood against query_gamma on one index:
10^6 documents at K = 100 filled by add_gamma_device, 64 four-word queries against 64 gamma columns.

    python tools/querylik_rate.py [--out FILE]

Host clock around calls that end in a synchronise; two warm-up calls, then the median of 15."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402

K, V, N, B, CHUNK, REPS = 100, 2000, 1000000, 64, 100000, 15


def main():
    _ffi.require_gpu()
    hip = _ffi.lib()
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else open(os.devnull, "w")
    out.write("# python tools/querylik_rate.py\n")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    model = OnlineLDA(num_words=V, num_topics=K, num_documents=N, alpha=.1, eta=.3, device=0)
    rng = np.random.RandomState(1)
    ix = model.document_index("hellinger")
    ix.reserve(N)
    ptr = _ffi.vp()
    _ffi.check(hip.trlda_dev_alloc(0, K * CHUNK * 8, C.byref(ptr)))
    for at in range(0, N, CHUNK):
        g = np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, CHUNK)) + 0.01)
        _ffi.check(hip.trlda_dev_upload(0, ptr, g.ctypes.data, g.nbytes))
        ix.add_gamma_device(ptr, CHUNK)
        _ffi.check(hip.trlda_model_synchronize(model._handle))
    hip.trlda_dev_free(0, ptr)
    assert len(ix) == N
    queries = [[(int(w), int(c)) for w, c in zip(rng.choice(V, 4, replace=False), rng.randint(1, 5, size=4))]
               for _ in range(B)]
    gq = np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, B)) + 0.01)
    batch = model.upload(queries)

    def timed(f):
        f()
        f()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    table_bytes = N * K * 8
    hbm = table_bytes / 8.0e12
    say("N = %d, K = %d, V = %d, B = %d, top_n = 10, %d calls each after 2 warm-up calls" % (N, K, V, B, REPS))
    say("table %.0f MB: one read at the 8.0 TB/s peak takes %.3f ms" % (table_bytes / 1e6, hbm * 1e3))
    results = {}
    for name, f in (("query_likelihood, 64 four-word queries", lambda: ix.query_likelihood(batch, top_n=10)),
                    ("query_gamma, 64 queries", lambda: ix.query_gamma(gq, top_n=10)),
                    ("query_likelihood, 1 four-word query", lambda: ix.query_likelihood(queries[:1], top_n=10)),
                    ("query_likelihood, 64 four-word queries", lambda: ix.query_likelihood(batch, top_n=10)),
                    ("query_gamma, 64 queries", lambda: ix.query_gamma(gq, top_n=10))):
        med, lo, hi = timed(f)
        results.setdefault(name, []).append(med)
        say("%-42s median %8.3f ms  (min %8.3f, max %8.3f)  table read at peak / median = %.4f"
            % (name, med * 1e3, lo * 1e3, hi * 1e3, hbm / med))
    ql = min(results["query_likelihood, 64 four-word queries"])
    qg = min(results["query_gamma, 64 queries"])
    say("ratio query_likelihood / query_gamma = %.2f" % (ql / qg))
    ids, s = ix.query_likelihood(batch, top_n=10)
    ix.set_slab_rows(4096)
    ids2, s2 = ix.query_likelihood(batch, top_n=10)
    say("slabs of 4096 rows against 2048: the same bits: %s" % (np.array_equal(ids, ids2) and np.array_equal(s, s2)))
    med, lo, hi = timed(lambda: ix.query_likelihood(batch, top_n=10))
    say("%-42s median %8.3f ms  (slabs of 4096 rows)" % ("query_likelihood, 64 four-word queries", med * 1e3))
    batch.close()
    model.close()
    out.close()


if __name__ == "__main__":
    main()
