"""Cost of LDA.word_topics (csrc/wordtopics_kernels.h) next to the E-step it follows: whole calls,
in-process, the batch resident as a DeviceBatch, the same gamma0 for every call, after a warm-up call.

    word_topics   E-step + scoring stage; copies gamma and entries x top_n results to the host
    do_e_step     the same E-step; copies gamma and the K x V statistics to the host
    scoring       trlda_model_word_topics_dev + a synchronise: the scoring stage alone (the row sums
                  of lambda and the word-topic kernel) from a gamma on the device, nothing copied

The two whole calls differ by the scoring stage AND by what they copy back (the statistics are K V 8
bytes), so the stage's own time is the third line.  The synthetic corpus is
trlda_amd.utils.synthetic's (Zipf words, Poisson lengths).

    python tools/wordtopics_rate.py [--configs k100_b200,k500_b512] [--calls N] [--top-n 1,3]

Run on the GPU box from the repo root; one JSON line per configuration and top_n.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (K, V, B)
    "k100_b200": (100, 7000, 200),
    "k500_b512": (500, 100000, 512),
}


def _timed(fn, calls):
    fn()                                             # warm-up
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--top-n", default="1,3")
    args = ap.parse_args()
    import trlda_amd
    from trlda_amd import _ffi
    from trlda_amd.documents import CSRDocuments, DeviceBatch
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils.synthetic import make_corpus

    L = _ffi.lib()
    for name in args.configs.split(","):
        K, V, B = CONFIGS[name]
        indptr, ids, cnts = make_corpus(B, V, seed=3)
        nnz = int(indptr[-1])
        trlda_amd.seed(1)
        model = OnlineLDA(num_words=V, num_topics=K, num_documents=10 * B, device=0)
        batch = DeviceBatch(CSRDocuments(indptr, ids, cnts), V, 0)
        g0 = np.asfortranarray(np.random.RandomState(2).gamma(1.0, 1.0, size=(K, B)) + 0.1)
        estep_med, estep_min = _timed(lambda: model.do_e_step(batch, latents=g0, max_iter=100), args.calls)
        gamma = np.asfortranarray(model.do_e_step(batch, latents=g0, max_iter=100)[0])
        for top_n in [int(t) for t in args.top_n.split(",")]:
            wt_med, wt_min = _timed(lambda: model.word_topics(batch, top_n=top_n, latents=g0, max_iter=100),
                                    args.calls)
            ptrs = [_ffi.vp() for _ in range(3)]
            for q, nbytes in zip(ptrs, (gamma.nbytes, nnz * top_n * 4, nnz * top_n * 8)):
                _ffi.check(L.trlda_dev_alloc(0, nbytes, C.byref(q)))
            _ffi.check(L.trlda_dev_upload(0, ptrs[0], gamma.ctypes.data, gamma.nbytes))

            def scoring():
                _ffi.check(L.trlda_model_word_topics_dev(model._handle, batch.handle, ptrs[0], top_n, ptrs[1],
                                                         ptrs[2]))
                _ffi.check(L.trlda_model_synchronize(model._handle))

            sc_med, sc_min = _timed(scoring, args.calls)
            for q in ptrs:
                L.trlda_dev_free(0, q)
            print(json.dumps({
                "config": name, "K": K, "V": V, "B": B, "entries": nnz, "top_n": top_n, "calls": args.calls,
                "word_topics_ms_median": round(wt_med * 1e3, 3), "word_topics_ms_min": round(wt_min * 1e3, 3),
                "do_e_step_ms_median": round(estep_med * 1e3, 3), "do_e_step_ms_min": round(estep_min * 1e3, 3),
                "difference_ms_median": round((wt_med - estep_med) * 1e3, 3),
                "scoring_ms_median": round(sc_med * 1e3, 3), "scoring_ms_min": round(sc_min * 1e3, 3),
                "lambda_column_bytes": nnz * K * 8, "lambda_table_bytes": K * V * 8,
                "scoring_GBps_columns": round(nnz * K * 8 / sc_med / 1e9, 2),
                "entries_per_s_scoring": round(nnz / sc_med)}), flush=True)
        batch.close()
        model.close()


if __name__ == "__main__":
    main()
