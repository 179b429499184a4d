"""Whole-call times of DocumentIndex.embed and its stages at K = 100, hellinger,
N in 1000, 20 000, 100 000, and the NumPy restatement's time per iteration at N = 2000 for scale.

    python tools/embed_rate.py [--out FILE] [--sizes 1000,20000] [--one N]

Host clock around calls that end in a synchronise (uploads and downloads included); one warm-up call,
then the median of 3 (the N = 100 000 map: one call after a 10-iteration warm-up).  Time per iteration
is (embed of 250 iterations - embed of 0 iterations) / 250 on the same affinities; the pair rate N (N -
1) / that time is a lower bound of the repulsion kernel's own rate, since an iteration also holds the
six small launches behind it.  `--one N` runs a single 50-iteration embed and nothing else: the
program to put behind `rocprofv3 --kernel-trace --stats --` for the kernel's own share of the call."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from trlda_amd import _ffi                                            # noqa: E402
from trlda_amd.models import OnlineLDA                                # noqa: E402

K, V, ITERS = 100, 2000, 250


def timed(f, reps=3, warm=True):
    if warm:
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def index_of(model, N):
    rng = np.random.RandomState(N)
    ix = model.document_index("hellinger")
    ix.add_gamma(np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, N)) + 0.01))
    return ix


def main():
    _ffi.require_gpu()
    arg = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
    model = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)
    if arg("--one"):
        ix = index_of(model, int(arg("--one")))
        ix.embed(num_iterations=50)
        model.close()
        return
    out = open(arg("--out"), "w") if arg("--out") else open(os.devnull, "w")
    out.write("# python tools/embed_rate.py\n")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    sizes = [int(n) for n in (arg("--sizes") or "1000,20000,100000").split(",")]
    for N in sizes:
        ix = index_of(model, N)
        big = N >= 50000
        reps = 1 if big else 3
        med, lo, hi = timed(lambda: ix.nearest_neighbors(90), reps)
        say("N = %d: nearest_neighbors(90): median %.1f ms (min %.1f, max %.1f); 2 N^2 K = %.3g flop: %.2f Tflop/s"
            % (N, med * 1e3, lo * 1e3, hi * 1e3, 2.0 * N * N * K, 2.0 * N * N * K / med / 1e12))
        med, lo, hi = timed(lambda: ix.affinities(30.0, return_conditional=True), reps)
        say("N = %d: affinities(30), conditional (the same graph and the calibration): median %.1f ms (min %.1f, "
            "max %.1f)" % (N, med * 1e3, lo * 1e3, hi * 1e3))
        med, lo, hi = timed(lambda: ix.affinities(30.0), reps)
        say("N = %d: affinities(30), symmetrised on the host: median %.1f ms (min %.1f, max %.1f)"
            % (N, med * 1e3, lo * 1e3, hi * 1e3))
        aff = ix.affinities(30.0)
        y0 = ix._pca_start(N)
        ix.embed(num_iterations=10, init=y0, affinities=aff)                 # warm-up
        zero, _, _ = timed(lambda: ix.embed(num_iterations=0, init=y0, affinities=aff), reps, warm=False)
        med, lo, hi = timed(lambda: ix.embed(num_iterations=ITERS, init=y0, affinities=aff), reps, warm=False)
        per = (med - zero) / ITERS
        say("N = %d: embed, %d iterations on given affinities: median %.1f ms (min %.1f, max %.1f); %.3f ms per "
            "iteration; N (N - 1) / iteration = %.3g pair terms/s (a lower bound of the repulsion kernel's rate)"
            % (N, ITERS, med * 1e3, lo * 1e3, hi * 1e3, per * 1e3, N * (N - 1.0) / per))
        med, lo, hi = timed(lambda: ix.embed(num_iterations=ITERS), 1, warm=False)
        say("N = %d: embed(perplexity=30, num_iterations=%d), whole call with graph, calibration, symmetrisation and "
            "PCA start: %.1f ms" % (N, ITERS, med * 1e3))
        ix.close()
    # the restatement, for scale
    import docindex_host as dh
    import embed_host as eh
    gamma, _ = eh.planted(2000, 1, 6)
    P = eh.affinities(dh.rows(gamma), 30.0)
    y = eh.pca_start(eh.theta_of(dh.rows(gamma)))
    t0 = time.perf_counter()
    eh.loop(y, P, 3)
    say("NumPy restatement, N = 2000: %.1f ms per iteration" % ((time.perf_counter() - t0) / 3 * 1e3))
    model.close()
    out.close()


if __name__ == "__main__":
    main()
