"""Device time of LDA.similar_words per call (csrc/wordsim_kernels.h) beside LDA.recommend_gamma
(csrc/recommend_kernels.h) at the same K, V, B and top_n, on the same model in the same run: the same
V x B x K product on the matrix cores without the staging transform, so the ratio of the two query
kernels is what the multiply and the square root cost.

The calls run in a child process under `rocprofv3 --kernel-trace --stats`: `calls` warm-up calls and
`calls` calls of recommend_gamma(gamma, top_n), then of similar_words(words, top_n) under hellinger,
then under cosine.  The kernel trace is read back, cut into the three phases at the row sums in front
of each phase's first own kernel, and the dispatches of the last `calls` calls of each phase (the
buffer fills between them included) are summed and divided by the number of calls.

    python tools/wordsim_rate.py [--configs k100,k500] [--calls N] [--out DIR] [--write]

Run from the repo root on a machine with the GPU; one JSON line per configuration.  `--write` also
puts the lines into profiles/wordsim_rate.txt.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (K, V, B, top_n)
    "k100": (100, 7000, 128, 10),
    "k500": (500, 100000, 128, 10),
}
KERNELS = ("recommend_", "wordsim_", "relevance_coef", "rowsum_", "fillBuffer")


def child(name, calls):
    from trlda_amd import _ffi
    from trlda_amd.models import OnlineLDA
    _ffi.require_gpu()
    K, V, B, n = CONFIGS[name]
    rng = np.random.RandomState(1)
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.01, device=0)
    m.lambdas = rng.gamma(0.3, 1.0, size=(K, V)) + 0.01
    gamma = np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, B)) + 0.01)
    words = rng.randint(0, V, size=B)
    host = {}
    for what, call in (("recommend_gamma", lambda: m.recommend_gamma(gamma, n)),
                       ("similar_words_hellinger", lambda: m.similar_words(words, n)),
                       ("similar_words_cosine", lambda: m.similar_words(words, n, measure="cosine"))):
        ms = []
        for i in range(2 * calls):                       # (the first half warms up)
            t0 = time.perf_counter()
            call()
            if i >= calls:
                ms.append((time.perf_counter() - t0) * 1e3)
        host[what + "_host_ms"] = round(float(np.median(ms)), 3)
    m.close()
    print(json.dumps(host), flush=True)


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


def _calls(rows, own):
    """The phase's rows cut into calls: a call starts at the row sums in front of its `own` kernel."""
    starts, last_rowsum = [], None
    for i, r in enumerate(rows):
        if "rowsum_partial" in r[2]:
            last_rowsum = i
        elif own in r[2]:
            starts.append(last_rowsum)
    return starts


def _phase(rows, calls):
    per = {}
    for s, e, k in rows:
        key = k.split("(")[0][:60]
        per[key] = per.get(key, 0) + (e - s)
    return round(sum(per.values()) / calls / 1e3, 2), {k: round(v / calls / 1e3, 2) for k, v in sorted(per.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--write", action="store_true", help="also write profiles/wordsim_rate.txt")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.calls)
    made = args.out is None                   # (a temporary directory of our own is removed at the end)
    if made:
        args.out = tempfile.mkdtemp(prefix="wordsim_rate_")
    lines = []
    for name in args.configs.split(","):
        K, V, B, n = CONFIGS[name]
        out_dir = os.path.join(args.out, name)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir,
               "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", name,
               "--calls", str(args.calls)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-3000:] + p.stderr[-3000:])
            raise SystemExit(p.returncode)
        info = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        rows = [r for r in _trace(out_dir) if any(k in r[2] for k in KERNELS)]
        rec = _calls(rows, "recommend_rows")
        sim = _calls(rows, "wordsim_norm")                # hellinger, then cosine
        if len(rec) != 2 * args.calls or len(sim) != 4 * args.calls:
            raise SystemExit("expected %d + %d calls in the trace, found %d + %d"
                             % (2 * args.calls, 4 * args.calls, len(rec), len(sim)))
        c = args.calls
        r_us, r_k = _phase(rows[rec[c]:sim[0]], c)
        h_us, h_k = _phase(rows[sim[c]:sim[2 * c]], c)
        c_us, c_k = _phase(rows[sim[3 * c]:], c)
        query = lambda per: sum(v for k, v in per.items() if "query_kernel" in k)  # noqa: E731
        line = json.dumps({
            "config": name, "K": K, "V": V, "B": B, "top_n": n, "calls": c, **info,
            "recommend_gamma_us": r_us, "similar_words_hellinger_us": h_us, "similar_words_cosine_us": c_us,
            "hellinger_over_recommend": round(h_us / r_us, 2), "cosine_over_recommend": round(c_us / r_us, 2),
            "query_kernel_hellinger_over_recommend": round(query(h_k) / query(r_k), 2),
            "query_kernel_cosine_over_recommend": round(query(c_k) / query(r_k), 2),
            "mfma_flops": 2 * K * V * B, "lambda_read_us_at_4TBps": round(8.0 * K * V / 4e6, 2),
            "kernels_us": {"recommend_gamma": r_k, "similar_words_hellinger": h_k, "similar_words_cosine": c_k},
        })
        print(line, flush=True)
        lines.append(line)
    if args.write:
        with open(os.path.join(ROOT, "profiles", "wordsim_rate.txt"), "w") as fh:
            fh.write("# python tools/wordsim_rate.py --calls %d --write\n" % args.calls)
            fh.write("\n".join(lines) + "\n")
    if made:
        shutil.rmtree(args.out, ignore_errors=True)


if __name__ == "__main__":
    main()
