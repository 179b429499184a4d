"""Throughput of the Gibbs E-step, update_variables(inference_method='gibbs') (csrc/gibbs_kernels.h):
tokens and documents per second of whole calls, in-process, inputs resident as a DeviceBatch, after
a warm-up call.  The synthetic corpus is trlda_amd.utils.synthetic's (Zipf words, Poisson lengths).

    python tools/gibbs_rate.py [--configs k100_b200,k100_b6400,...] [--calls N]

Run on the GPU box from the repo root; one JSON line per configuration.
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

CONFIGS = {
    # name: (K, V, B, burn_in, num_samples)
    "k100_b200": (100, 7000, 200, 2, 1),
    "k100_b6400": (100, 7000, 6400, 2, 1),
    "k100_b200_long": (100, 7000, 200, 10, 20),
    "k100_b6400_long": (100, 7000, 6400, 10, 20),
    "k500_b512": (500, 100000, 512, 2, 1),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    import trlda_amd
    from trlda_amd.documents import CSRDocuments, DeviceBatch
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils.synthetic import make_corpus

    for name in args.configs.split(","):
        K, V, B, burn_in, num_samples = CONFIGS[name]
        indptr, ids, cnts = make_corpus(B, V, seed=3)
        tokens = int(np.maximum(cnts, 0).sum())
        trlda_amd.seed(1)
        model = OnlineLDA(num_words=V, num_topics=K, num_documents=10 * B, device=0)
        batch = DeviceBatch(CSRDocuments(indptr, ids, cnts), V, 0)
        model.update_variables(batch, inference_method="gibbs", burn_in=burn_in,
                               num_samples=num_samples)                       # warm-up
        times = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            model.update_variables(batch, inference_method="gibbs", burn_in=burn_in,
                                   num_samples=num_samples)
            times.append(time.perf_counter() - t0)
        batch.close()
        model.close()
        best, med = min(times), float(np.median(times))
        print(json.dumps({
            "config": name, "K": K, "V": V, "B": B, "burn_in": burn_in, "num_samples": num_samples,
            "tokens": tokens, "calls": args.calls, "ms_median": round(med * 1e3, 3),
            "ms_min": round(best * 1e3, 3), "tokens_per_s": round(tokens / med),
            "token_sweeps_per_s": round(tokens * (burn_in + num_samples) / med),
            "docs_per_s": round(B / med)}), flush=True)


if __name__ == "__main__":
    main()
