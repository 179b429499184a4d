"""Device time of LDA.predictive_log_likelihood (csrc/heldout_kernels.h) per call, split into the
E-step on the observed parts and the held-out scoring kernel.

The calls run in a child process under `rocprofv3 --kernel-trace --stats`; the kernel trace is read
back and every call's dispatches -- those after the previous call's scoring kernel, up to and
including its own -- are summed by kernel.  The first call (allocations, code objects) is left out.
The E-step's preamble (row sums, exp E[log beta]) is reported apart from its document kernel.

    python tools/heldout_rate.py [--configs k100,k500] [--calls N] [--out DIR]

Run from the repo root on a machine with the GPU; one JSON line per configuration.
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

CONFIGS = {
    # name: (K, V, B, tokens per document, held-out fraction)
    "k100": (100, 7000, 2000, 100, 0.2),
    "k500": (500, 100000, 512, 100, 0.2),
}
HELDOUT = "heldout_docs_kernel"
PREAMBLE = ("rowsum", "exp_elog_beta", "topic_factors", "preamble_fused")


def child(name, calls):
    import trlda_amd
    from trlda_amd import _ffi
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils import split_documents
    _ffi.require_gpu()
    K, V, B, length, frac = CONFIGS[name]
    rng = np.random.RandomState(1)
    n = rng.poisson(length, size=B)
    indptr = np.concatenate([[0], np.cumsum(n)])
    docs = CSRDocuments(indptr, rng.randint(0, V, size=indptr[-1]), np.ones(indptr[-1]))
    trlda_amd.seed(3)
    observed, heldout = split_documents(docs, frac)
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=B, alpha=.1, eta=.01, device=0)
    m.lambdas = rng.gamma(1.0, 1.0, size=(K, V)) + 0.01
    ob, hb = m.upload(observed), m.upload(heldout)
    g0 = np.asfortranarray(rng.gamma(100., 1. / 100., size=(K, B)))
    ms = []
    for _ in range(calls + 1):
        t0 = time.perf_counter()
        score = m.predictive_log_likelihood(ob, hb, latents=g0)
        ms.append((time.perf_counter() - t0) * 1e3)
    ob.close()
    hb.close()
    m.close()
    print(json.dumps({"score": score, "host_call_ms": float(np.median(ms[1:])),
                      "heldout_tokens": int(heldout.csr.cnts.sum()),
                      "heldout_entries": int(heldout.csr.indptr[-1])}), flush=True)


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


def split_calls(rows):
    """per call after the first: {kernel name: ns}"""
    ends = [i for i, r in enumerate(rows) if HELDOUT in r[2]]
    calls = []
    for a, b in zip(ends, ends[1:]):
        per = {}
        for s, e, k in rows[a + 1:b + 1]:
            per[k] = per.get(k, 0) + (e - s)
        calls.append(per)
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.calls)
    if args.out is None:
        args.out = tempfile.mkdtemp(prefix="heldout_rate_")
    for name in args.configs.split(","):
        out_dir = os.path.join(args.out, name)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir,
               "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", name,
               "--calls", str(args.calls)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-3000:] + p.stderr[-3000:])
            raise SystemExit(p.returncode)
        info = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        calls = split_calls(_trace(out_dir))
        def mean_us(pred):
            return float(np.mean([sum(v for k, v in c.items() if pred(k)) for c in calls])) / 1e3
        kernels = sorted({k for c in calls for k in c})
        K, V, B, length, frac = CONFIGS[name]
        print(json.dumps({
            "config": name, "K": K, "V": V, "B": B, "tokens_per_doc": length, "heldout": frac,
            "calls_timed": len(calls), **info,
            "device_call_us": round(mean_us(lambda k: True), 2),
            "estep_us": round(mean_us(lambda k: HELDOUT not in k), 2),
            "estep_preamble_us": round(mean_us(lambda k: any(p in k for p in PREAMBLE)), 2),
            "heldout_kernel_us": round(mean_us(lambda k: HELDOUT in k), 2),
            "kernels_us": {k.split("(")[0][:60]: round(mean_us(lambda x, k=k: x == k), 2) for k in kernels},
        }), flush=True)


if __name__ == "__main__":
    main()
