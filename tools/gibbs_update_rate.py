"""Time of whole Gibbs updates, OnlineLDA.update_parameters(inference_method='gibbs') (csrc/gibbs_kernels.h,
gibbs_mstep_kernel), against the loop a user had to write before it: max_iter_tr x
{update_variables(inference_method='gibbs'), the blend in NumPy, lambdas = ...}.  In-process, the
batch resident as a DeviceBatch, after a warm-up call; the synthetic corpus is
trlda_amd.utils.synthetic's (Zipf words, Poisson lengths).

    python tools/gibbs_update_rate.py [--configs k100_b200,k500_b512] [--calls N] [--only device]

`device` reuses one DeviceBatch, so its Gibbs plan (token offsets, document order: one small
download and two waits) is made once; `device_fresh_batch` uploads a new DeviceBatch every call,
as a loop over fresh mini-batches does, and so pays the upload and the plan each time.

Run on the GPU box from the repo root; one JSON line per configuration and path.
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
    # name: (K, V, B, max_iter_tr)
    "k100_b200": (100, 7000, 200, 10),
    "k500_b512": (500, 100000, 512, 10),
}


def by_hand(model, batch, T, rho, D, B):
    """onlinelda.cpp:68-101 as a user writes it with update_variables(gibbs) (the initial step from
    the word counts left out: it only makes the hand-written loop faster)."""
    lam_p = np.array(model.lambdas)
    for _ in range(T):
        _, sstats = model.update_variables(batch, inference_method="gibbs")
        model.lambdas = (1. - rho) * lam_p + rho * (model.eta + D / B * sstats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", default="device,device_fresh_batch,by_hand")
    args = ap.parse_args()
    import trlda_amd
    from trlda_amd.documents import CSRDocuments, DeviceBatch
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils.synthetic import make_corpus

    for name in args.configs.split(","):
        K, V, B, T = CONFIGS[name]
        indptr, ids, cnts = make_corpus(B, V, seed=3)
        tokens = int(np.maximum(cnts, 0).sum())
        D = 10 * B
        for path in args.only.split(","):
            trlda_amd.seed(1)
            model = OnlineLDA(num_words=V, num_topics=K, num_documents=D, device=0)
            batch = DeviceBatch(CSRDocuments(indptr, ids, cnts), V, 0)

            def call():
                if path in ("device", "device_fresh_batch"):
                    if path == "device":
                        model.update_parameters(batch, max_iter_tr=T, inference_method="gibbs")
                    else:                # a new mini-batch each call: upload and Gibbs plan included
                        b = DeviceBatch(CSRDocuments(indptr, ids, cnts), V, 0)
                        model.update_parameters(b, max_iter_tr=T, inference_method="gibbs")
                        b.close()
                    from trlda_amd import _ffi
                    _ffi.check(_ffi.lib().trlda_model_synchronize(model._handle))
                else:
                    by_hand(model, batch, T, 0.5, D, B)
            call()                                                           # warm-up
            times = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                call()
                times.append(time.perf_counter() - t0)
            batch.close()
            model.close()
            med = float(np.median(times))
            print(json.dumps({
                "config": name, "path": path, "K": K, "V": V, "B": B, "max_iter_tr": T,
                "tokens": tokens, "calls": args.calls, "ms_median": round(med * 1e3, 3),
                "ms_min": round(min(times) * 1e3, 3), "ms_per_iteration": round(med * 1e3 / T, 3)}),
                flush=True)


if __name__ == "__main__":
    main()
