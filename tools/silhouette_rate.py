"""Whole-call time of DocumentIndex.silhouette on one index: 20 000 documents at
K = 100 under the labels of cluster(8), hellinger, every document scored.

    python tools/silhouette_rate.py [--out FILE]

Host clock around calls that end in a synchronise (the labels' upload and the four results' download
included); one warm-up call, then the median of 5."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trlda_amd                                                      # noqa: E402
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402

K, V, N, CLUSTERS, REPS = 100, 2000, 20000, 8, 5


def main():
    _ffi.require_gpu()
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else open(os.devnull, "w")
    out.write("# python tools/silhouette_rate.py\n")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    model = OnlineLDA(num_words=V, num_topics=K, num_documents=N, alpha=.1, eta=.3, device=0)
    rng = np.random.RandomState(1)
    ix = model.document_index("hellinger")
    ix.add_gamma(np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, N)) + 0.01))
    trlda_amd.seed(1)
    labels, _, info = ix.cluster(CLUSTERS, return_info=True)

    def timed(f):
        f()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    flops = 2.0 * N * N * K
    say("N = %d, K = %d, C = %d (sizes %s), hellinger, %d calls after 1 warm-up call"
        % (N, K, CLUSTERS, info["sizes"].tolist(), REPS))
    med, lo, hi = timed(lambda: ix.silhouette(labels, return_parts=True))
    say("silhouette, all %d documents: median %.3f ms (min %.3f, max %.3f); 2 N^2 K = %.3g flop: %.2f Tflop/s, "
        "%.3g pairs/s" % (N, med * 1e3, lo * 1e3, hi * 1e3, flops, flops / med / 1e12, N * float(N) / med))
    ids = np.arange(0, N, 10)
    med, lo, hi = timed(lambda: ix.silhouette(labels, ids=ids))
    say("silhouette, %d ids: median %.3f ms (min %.3f, max %.3f)" % (len(ids), med * 1e3, lo * 1e3, hi * 1e3))
    s = ix.silhouette(labels)
    say("mean silhouette %.6f" % (float(np.sum(s)) / N))
    model.close()
    out.close()


if __name__ == "__main__":
    main()
