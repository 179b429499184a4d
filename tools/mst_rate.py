"""Time of one sweep of DocumentIndex.spanning_tree and of the whole call on one index:
40 000 documents at K = 100, hellinger, beside neighbors_within(count_only=True) on the same index, which
forms the same N x N x K product once and is the yardstick for a sweep.

    python tools/mst_rate.py [--out FILE] [--once]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mst_rate.py --once

Host clock around calls that end in a synchronise (uploads and downloads included); one warm-up call,
then the median of 3; the sweep also with the search's slab of 2048 rows forced, which is what its own
default is measured against.  --once makes every call once after its warm-up, for a run under rocprofv3, whose
kernel statistics give the device time of mst_sweep_kernel and neighbors_count_kernel alone: there the
sweep of the first round (every document alone) is called 2 times, the count-only pass 2 times, and a
whole spanning_tree twice (min_samples 1 and 5)."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402

K, V, N = 100, 2000, 40000


def main():
    _ffi.require_gpu()
    reps = 1 if "--once" in sys.argv else 3
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else open(os.devnull, "w")
    out.write("# python tools/mst_rate.py\n")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    model = OnlineLDA(num_words=V, num_topics=K, num_documents=N, alpha=.1, eta=.3, device=0)
    rng = np.random.RandomState(1)
    ix = model.document_index("hellinger")
    ix.add_gamma(np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, N)) + 0.01))
    probe = ix.neighbors_within(2.0, ids=np.arange(0, N, N // 200))[2]
    radius = float(np.quantile(probe, 0.001))

    def timed(f):
        f()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    flops = 2.0 * N * N * K
    say("N = %d, K = %d, hellinger; %d call(s) after 1 warm-up call; 2 N^2 K = %.3g flop" % (N, K, reps, flops))
    med, lo, hi = timed(lambda: ix.neighbors_within(radius, count_only=True))
    say("neighbors_within(%.4f, count_only=True): median %.1f ms (min %.1f, max %.1f): %.2f Tflop/s"
        % (radius, med * 1e3, lo * 1e3, hi * 1e3, flops / med / 1e12))
    count = med
    comp = np.arange(N, dtype=np.int32)
    med, lo, hi = timed(lambda: ix._sweep(comp, None))
    say("one sweep, every document alone, no core distances: median %.1f ms (min %.1f, max %.1f): %.2f Tflop/s, "
        "%.2f of the count-only pass" % (med * 1e3, lo * 1e3, hi * 1e3, flops / med / 1e12, med / count))
    if "--once" not in sys.argv:
        ix.set_slab_rows(2048)                                        # the search's default slab: 20 workgroups
        med, lo, hi = timed(lambda: ix._sweep(comp, None))
        ix.set_slab_rows(0)
        say("the same sweep with slabs of 2048 rows: median %.1f ms (min %.1f, max %.1f)" % (med * 1e3, lo * 1e3, hi * 1e3))
    for ms in (1, 5):
        rounds = []
        sweep = ix._sweep
        ix._sweep = lambda c, r: rounds.append(len(np.unique(c))) or sweep(c, r)
        t0 = time.perf_counter()
        u, v, w = ix.spanning_tree(ms)
        whole = time.perf_counter() - t0
        ix._sweep = sweep
        say("spanning_tree(min_samples=%d): %.1f ms, %d sweeps on %s components; total weight %.6f"
            % (ms, whole * 1e3, len(rounds), rounds, float(np.sum(w))))
    t0 = time.perf_counter()
    labels = ix.hdbscan()
    say("hdbscan(): %.1f ms; %d clusters, %d noise" % ((time.perf_counter() - t0) * 1e3, int(labels.max()) + 1,
                                                      int((labels < 0).sum())))
    model.close()
    out.close()


if __name__ == "__main__":
    main()
