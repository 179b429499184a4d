"""Device time of LDA.top_words and of the counting behind LDA.topic_coherence
(csrc/coherence_kernels.h) per call.

The calls run in a child process under `rocprofv3 --kernel-trace --stats`; the kernel trace is read
back and the dispatches of the configuration's kernels (the buffer fills between them included) are
summed and divided by the number of calls.  Every call does the same work, so the mean is the
per-call device time.

    python tools/coherence_rate.py [--configs top_k100,top_k500,...] [--calls N] [--out DIR]

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
    # name: (what, K, V, top_n, documents per batch, batches)
    "top_k100": ("top", 100, 7000, 10, 0, 0),
    "top_k500": ("top", 500, 100000, 10, 0, 0),
    "top_k500_n100": ("top", 500, 100000, 100, 0, 0),
    "count_b200": ("count", 100, 7000, 10, 200, 1),
    "count_b200_k500_n100": ("count", 500, 100000, 100, 200, 1),
    "count_stream": ("count", 100, 7000, 10, 1000, 40),
}
KERNELS = {"top": ("topn_",), "count": ("cooc_", "fillBuffer")}


def child(name, calls):
    from trlda_amd import _ffi
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils import make_corpus
    _ffi.require_gpu()
    what, K, V, n, B, batches = CONFIGS[name]
    rng = np.random.RandomState(1)
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.01, device=0)
    m.lambdas = rng.gamma(0.3, 1.0, size=(K, V)) + 0.01
    ms = []
    info = {}
    if what == "top":
        for _ in range(calls):
            t0 = time.perf_counter()
            m.top_words(n)
            ms.append((time.perf_counter() - t0) * 1e3)
    else:
        words = m.top_words(n)
        parts = [CSRDocuments(*make_corpus(B, V, seed=100 + i, mean_unique=60)) for i in range(batches)]
        dev = [m.upload(p) for p in parts]
        for _ in range(calls):
            t0 = time.perf_counter()
            coh = m.topic_coherence(iter(dev), words=words, measure="npmi")
            ms.append((time.perf_counter() - t0) * 1e3)
        for b in dev:
            b.close()
        info = {"documents": B * batches, "entries": int(sum(p.indptr[-1] for p in parts)),
                "distinct_words": int(len(np.unique(words))), "mean_npmi": float(np.nanmean(coh))}
    m.close()
    print(json.dumps({"host_call_ms": float(np.median(ms)), **info}), flush=True)


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
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.calls)
    if args.out is None:
        args.out = tempfile.mkdtemp(prefix="coherence_rate_")
    for name in args.configs.split(","):
        what, K, V, n, B, batches = CONFIGS[name]
        out_dir = os.path.join(args.out, name)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir,
               "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", name,
               "--calls", str(args.calls)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-3000:] + p.stderr[-3000:])
            raise SystemExit(p.returncode)
        info = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        rows = _trace(out_dir)
        if what == "count":                    # (what the child ran before: set-up, its top_words)
            rows = rows[max(i for i, r in enumerate(rows) if "topn_" in r[2]) + 1:]
        rows = [r for r in rows if any(k in r[2] for k in KERNELS[what])]
        per = {}
        for s, e, k in rows:
            key = k.split("(")[0][:60]
            per[key] = per.get(key, 0) + (e - s)
        print(json.dumps({
            "config": name, "what": what, "K": K, "V": V, "top_n": n, "docs_per_batch": B,
            "batches": batches, "calls": args.calls, **info,
            "device_call_us": round(sum(per.values()) / args.calls / 1e3, 2),
            "kernels_us": {k: round(v / args.calls / 1e3, 2) for k, v in sorted(per.items())},
        }), flush=True)


if __name__ == "__main__":
    main()
