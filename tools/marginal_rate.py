"""Device time of LDA.document_log_likelihood (csrc/marginal_kernels.h) per call, per proposal:
200 documents of the bench's shape (K = 100, V = 7000, ~100 distinct words each), S = 256 samples.

The calls run in a child process under `rocprofv3 --kernel-trace --stats`; the kernel trace is read
back and the marginal kernel's dispatches are averaged (the first call of each proposal is left
out), next to the whole call's kernels and to the flop count S n_d K 2 of the dot products against
the fp64 vector peak bench.py quotes.

    python tools/marginal_rate.py [--calls N] [--samples S] [--out DIR]

Run from the repo root on a machine with the GPU; one JSON line.  With --out the directory keeps
rocprofv3's files (run_kernel_stats.csv is the one profiles/ holds).
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K, V, B, MEAN_UNIQUE = 100, 7000, 200, 100
FP64_PEAK_TFLOPS = 78.6                      # bench.py
KERNEL = "marginal_docs_kernel"


def child(calls, samples):
    import trlda_amd
    from trlda_amd import _ffi
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils.synthetic import make_corpus
    _ffi.require_gpu()
    docs = CSRDocuments(*make_corpus(B, V, seed=7, mean_unique=MEAN_UNIQUE))
    trlda_amd.seed(3)
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=B, alpha=.1, eta=.01, device=0)
    batch = m.upload(docs)
    g0 = np.asfortranarray(np.random.RandomState(1).gamma(100., 1. / 100., size=(K, B)))
    info = {"entries": int(docs.indptr[-1]), "tokens": int(docs.cnts.sum())}
    for proposal in ("vi", "prior"):
        ms = []
        for _ in range(calls + 1):
            t0 = time.perf_counter()
            ll, ess = m.document_log_likelihood(batch, num_samples=samples, proposal=proposal, return_ess=True,
                                                latents=g0 if proposal == "vi" else None)
            ms.append((time.perf_counter() - t0) * 1e3)
        info[proposal] = {"host_call_ms": float(np.median(ms[1:])), "loglik_per_token": float(ll.sum() / docs.cnts.sum()),
                          "median_ess": float(np.median(ess))}
    batch.close()
    m.close()
    print(json.dumps(info), flush=True)


def _trace(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel trace under %s" % out_dir)
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--out", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.calls, args.samples)
    out_dir = args.out or tempfile.mkdtemp(prefix="marginal_rate_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls),
           "--samples", str(args.samples)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-3000:] + p.stderr[-3000:])
        raise SystemExit(p.returncode)
    info = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    rows = _trace(out_dir)
    ends = [i for i, r in enumerate(rows) if KERNEL in r[2]]
    n = args.calls + 1
    assert len(ends) == 2 * n, (len(ends), n)
    out = {"K": K, "V": V, "B": B, "samples": args.samples, **info}
    flops = 2.0 * args.samples * info["entries"] * K
    for name, idx in (("vi", ends[1:n]), ("prior", ends[n + 1:])):
        kern = [rows[i][1] - rows[i][0] for i in idx]
        # the call's other kernels: those between the previous marginal kernel and this one
        rest = [sum(e - s for s, e, _ in rows[ends[ends.index(i) - 1] + 1:i]) for i in idx]
        us = float(np.mean(kern)) / 1e3
        out[name].update({"marginal_kernel_us": round(us, 1), "other_kernels_us": round(float(np.mean(rest)) / 1e3, 1),
                          "dot_product_tflops": round(flops / us / 1e6, 3),
                          "of_fp64_vector_peak": round(flops / us / 1e6 / FP64_PEAK_TFLOPS, 4)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
