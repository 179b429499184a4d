"""Device time of LDA.left_to_right (csrc/l2r_kernels.h) per call, with and without `resample`:
200 documents of the bench's shape (K = 100, V = 7000, ~100 distinct words each), R = 20 particles.

The calls run in a child process under `rocprofv3 --kernel-trace --stats`; the kernel trace is read
back and the document kernel's dispatches are averaged (the first call of each setting is left out),
next to the call's other kernels and to the number of histogram draws per call.

    python tools/l2r_rate.py [--calls N] [--particles R] [--out DIR]

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
KERNEL = "l2r_docs_kernel"
SETTINGS = (("resample", True), ("sequential", False))


def child(calls, particles):
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
    n = np.add.reduceat(np.append(docs.cnts, 0), docs.indptr[:-1]).astype(np.int64) * (np.diff(docs.indptr) > 0)
    info = {"entries": int(docs.indptr[-1]), "tokens": int(n.sum()), "longest": int(n.max()),
            "draws": {"resample": int((n * (n + 1) // 2).sum()) * particles, "sequential": int(n.sum()) * particles}}
    for name, resample in SETTINGS:
        ms = []
        for _ in range(calls + 1):
            t0 = time.perf_counter()
            ll, tokens = m.left_to_right(batch, num_particles=particles, resample=resample, return_tokens=True)
            ms.append((time.perf_counter() - t0) * 1e3)
        info[name] = {"host_call_ms": float(np.mean(ms[1:])), "loglik_per_token": float(ll.sum() / tokens.sum())}
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
    ap.add_argument("--particles", type=int, default=20)
    ap.add_argument("--out", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.calls, args.particles)
    out_dir = args.out or tempfile.mkdtemp(prefix="l2r_rate_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls),
           "--particles", str(args.particles)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-3000:] + p.stderr[-3000:])
        raise SystemExit(p.returncode)
    info = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    rows = _trace(out_dir)
    ends = [i for i, r in enumerate(rows) if KERNEL in r[2]]
    n = args.calls + 1
    assert len(ends) == 2 * n, (len(ends), n)                # (one group of documents per call at this shape)
    out = {"K": K, "V": V, "B": B, "particles": args.particles, **info}
    for name, idx in ((SETTINGS[0][0], ends[1:n]), (SETTINGS[1][0], ends[n + 1:])):
        kern = [rows[i][1] - rows[i][0] for i in idx]
        # the call's other kernels: those between the previous document kernel and this one (the
        # finish kernel of the call before among them, in place of this call's)
        rest = [sum(e - s for s, e, _ in rows[ends[ends.index(i) - 1] + 1:i]) for i in idx]
        us = float(np.mean(kern)) / 1e3
        out[name].update({"docs_kernel_us": round(us, 1), "other_kernels_us": round(float(np.mean(rest)) / 1e3, 1),
                          "ns_per_draw": round(us * 1e3 / info["draws"][name], 4)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
