"""Whole-call time of DocumentIndex.neighbors_within on one index: 20 000 documents at
K = 100, hellinger, every document scored, at a radius that about 1 pair in 1000 meets.

    python tools/neighbors_rate.py [--out FILE]

Host clock around calls that end in a synchronise (the downloads of indptr, ids and distances
included); one warm-up call, then the median of 5.  count_only forms the N x N x K product once, the
full call twice."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402

K, V, N, REPS = 100, 2000, 20000, 5


def main():
    _ffi.require_gpu()
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else open(os.devnull, "w")
    out.write("# python tools/neighbors_rate.py\n")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    model = OnlineLDA(num_words=V, num_topics=K, num_documents=N, alpha=.1, eta=.3, device=0)
    rng = np.random.RandomState(1)
    ix = model.document_index("hellinger")
    ix.add_gamma(np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, N)) + 0.01))
    # the radius: the 0.1 % quantile of the distances of 200 documents to all
    probe = ix.neighbors_within(2.0, ids=np.arange(0, N, N // 200))[2]
    radius = float(np.quantile(probe, 0.001))

    def timed(f):
        f()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    flops = 2.0 * N * N * K
    total = int(ix.neighbors_within(radius, count_only=True)[-1])
    say("N = %d, K = %d, hellinger, radius %.4f: %d pairs (%.3g of N^2), %d calls after 1 warm-up call"
        % (N, K, radius, total, total / float(N) / N, REPS))
    med, lo, hi = timed(lambda: ix.neighbors_within(radius, count_only=True))
    say("count_only, all %d documents: median %.3f ms (min %.3f, max %.3f); 2 N^2 K = %.3g flop once: %.2f Tflop/s, "
        "%.3g pairs/s" % (N, med * 1e3, lo * 1e3, hi * 1e3, flops, flops / med / 1e12, N * float(N) / med))
    med, lo, hi = timed(lambda: ix.neighbors_within(radius))
    say("neighbors_within, all %d documents: median %.3f ms (min %.3f, max %.3f); the product twice: %.2f Tflop/s"
        % (N, med * 1e3, lo * 1e3, hi * 1e3, 2 * flops / med / 1e12))
    ids = np.arange(0, N, 100)
    for slab in (0, 2048):
        ix.set_slab_rows(slab)
        med, lo, hi = timed(lambda: ix.neighbors_within(radius, ids=ids))
        say("neighbors_within, %d ids, slab %s: median %.3f ms (min %.3f, max %.3f)"
            % (len(ids), slab or "default", med * 1e3, lo * 1e3, hi * 1e3))
    ix.set_slab_rows(0)
    med, lo, hi = timed(lambda: ix.dbscan(radius, 5))
    labels = ix.dbscan(radius, 5)
    say("dbscan(min_samples=5): median %.3f ms (min %.3f, max %.3f); %d clusters, %d noise"
        % (med * 1e3, lo * 1e3, hi * 1e3, int(labels.max()) + 1, int((labels < 0).sum())))
    model.close()
    out.close()


if __name__ == "__main__":
    main()
