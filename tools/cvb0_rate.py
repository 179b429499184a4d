"""Throughput of CVB0 inference, update_variables(inference_method='cvb0') (csrc/cvb0_kernels.h):
entry-updates (one phi row renormalised) and documents per second of whole calls, in-process, inputs
resident as a DeviceBatch, after a warm-up call -- and, in the same run on the same batch, the Gibbs
path's token rate over as many sweeps and the VI E-step, for scale.  Whole calls: each includes the
download of theta / gamma (K x B) and of the statistics (K x V).  The synthetic corpus is
trlda_amd.utils.synthetic's (Zipf words, Poisson lengths).

    python tools/cvb0_rate.py [--configs k100_b200,k100_b1600,...] [--calls N] [--out profiles/cvb0_rate.txt]

Run on the GPU box from the repo root; one JSON line per configuration and method.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SWEEPS = 20
CONFIGS = {
    # name: (K, V, B)
    "k100_b200": (100, 7000, 200),
    "k100_b1600": (100, 7000, 1600),
    "k500_b200": (500, 7000, 200),
    "k500_b1600": (500, 7000, 1600),
}


def timed(call, calls):
    call()                                                            # warm-up
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = call()                                                  # (every entry point synchronises)
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times)), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import trlda_amd
    from trlda_amd.documents import CSRDocuments, DeviceBatch
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils.synthetic import make_corpus

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for name in args.configs.split(","):
        K, V, B = CONFIGS[name]
        indptr, ids, cnts = make_corpus(B, V, seed=3)
        entries = int((cnts > 0).sum())
        tokens = int(np.maximum(cnts, 0).sum())
        trlda_amd.seed(1)
        model = OnlineLDA(num_words=V, num_topics=K, num_documents=10 * B, device=0)
        batch = DeviceBatch(CSRDocuments(indptr, ids, cnts), V, 0)
        base = {"config": name, "K": K, "V": V, "B": B, "entries": entries, "tokens": tokens,
                "calls": args.calls}

        (_, _, iters), med, best = timed(lambda: model.update_variables(
            batch, inference_method="cvb0", max_iter=SWEEPS, threshold=0.0, return_iterations=True), args.calls)
        assert int(iters.max()) == SWEEPS
        # (init and the sweeps: SWEEPS + 1 passes over a document's entries)
        emit(dict(base, method="cvb0", sweeps=SWEEPS, ms_median=round(med * 1e3, 3), ms_min=round(best * 1e3, 3),
                  entry_updates_per_s=round(entries * SWEEPS / med), docs_per_s=round(B / med)))

        (_, _, iters), med, best = timed(lambda: model.update_variables(
            batch, inference_method="cvb0", max_iter=100, threshold=1e-3, return_iterations=True), args.calls)
        emit(dict(base, method="cvb0 (max_iter=100, threshold=1e-3)", mean_sweeps=round(float(iters.mean()), 2),
                  max_sweeps=int(iters.max()), ms_median=round(med * 1e3, 3), ms_min=round(best * 1e3, 3),
                  docs_per_s=round(B / med)))

        _, med, best = timed(lambda: model.update_variables(
            batch, inference_method="gibbs", burn_in=SWEEPS - 1, num_samples=1), args.calls)
        emit(dict(base, method="gibbs", sweeps=SWEEPS, ms_median=round(med * 1e3, 3), ms_min=round(best * 1e3, 3),
                  token_sweeps_per_s=round(tokens * SWEEPS / med), docs_per_s=round(B / med)))

        (_, _, iters), med, best = timed(lambda: model.update_variables(
            batch, max_iter=SWEEPS, threshold=0.0, return_iterations=True), args.calls)
        emit(dict(base, method="vi", iterations=int(iters.max()), ms_median=round(med * 1e3, 3),
                  ms_min=round(best * 1e3, 3), entry_updates_per_s=round(entries * int(iters.max()) / med),
                  docs_per_s=round(B / med)))
        batch.close()
        model.close()


if __name__ == "__main__":
    main()
