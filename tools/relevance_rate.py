"""Device time of LDA.relevant_words, LDA.word_statistics and LDA.top_words per call
(csrc/relevance_kernels.h, csrc/coherence_kernels.h), on the same model in the same run.

The calls run in a child process under `rocprofv3 --kernel-trace --stats`: `calls` calls of
top_words(10), then of word_statistics(), then of relevant_words(10).  The kernel trace is read back,
cut into the three phases at the first dispatch of each phase's own kernel, and the dispatches of
each phase (the buffer fills between them included) are summed and divided by the number of calls.

    python tools/relevance_rate.py [--configs k100,k500] [--calls N] [--out DIR] [--write]

Run from the repo root on a machine with the GPU; one JSON line per configuration.  `--write` also
puts the lines into profiles/relevance_rate.txt.
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
    # name: (K, V, top_n)
    "k100": (100, 7000, 10),
    "k500": (500, 100000, 10),
}
KERNELS = ("topn_", "relevance_", "rowsum_", "fillBuffer")


def child(name, calls):
    from trlda_amd import _ffi
    from trlda_amd.models import OnlineLDA
    _ffi.require_gpu()
    K, V, n = CONFIGS[name]
    rng = np.random.RandomState(1)
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.01, device=0)
    m.lambdas = rng.gamma(0.3, 1.0, size=(K, V)) + 0.01
    host = {}
    for what, call in (("top_words", lambda: m.top_words(n)), ("word_statistics", m.word_statistics),
                       ("relevant_words", lambda: m.relevant_words(n, 0.6))):
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            call()
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
    ap.add_argument("--write", action="store_true", help="also write profiles/relevance_rate.txt")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.calls)
    made = args.out is None                   # (a temporary directory of our own is removed at the end)
    if made:
        args.out = tempfile.mkdtemp(prefix="relevance_rate_")
    lines = []
    for name in args.configs.split(","):
        K, V, n = CONFIGS[name]
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
        # the phases: top_words from its first tile kernel, word_statistics from the first column
        # pass's row sums, relevant_words from the row sums of the call that runs the first
        # relevance_tile_kernel (what came before: the model's set-up)
        first_top = min(i for i, r in enumerate(rows) if "topn_tile" in r[2])
        first_col = min(i for i, r in enumerate(rows) if "relevance_column" in r[2])
        first_tile = min(i for i, r in enumerate(rows) if "relevance_tile" in r[2])
        start_stats = max(i for i in range(first_col) if "rowsum_partial" in rows[i][2])
        start_rel = max(i for i in range(first_tile) if "rowsum_partial" in rows[i][2])
        keep = lambda part: [r for r in part if any(k in r[2] for k in KERNELS)]  # noqa: E731
        top, top_k = _phase(keep(rows[first_top:start_stats]), args.calls)
        st, st_k = _phase(keep(rows[start_stats:start_rel]), args.calls)
        rel, rel_k = _phase(keep(rows[start_rel:]), args.calls)
        line = json.dumps({
            "config": name, "K": K, "V": V, "top_n": n, "calls": args.calls, **info,
            "top_words_us": top, "word_statistics_us": st, "relevant_words_us": rel,
            "relevant_over_top": round(rel / top, 2), "lambda_read_us_at_4TBps": round(8.0 * K * V / 4e6, 2),
            "kernels_us": {"top_words": top_k, "word_statistics": st_k, "relevant_words": rel_k},
        })
        print(line, flush=True)
        lines.append(line)
    if args.write:
        with open(os.path.join(ROOT, "profiles", "relevance_rate.txt"), "w") as fh:
            fh.write("# python tools/relevance_rate.py --calls %d --write\n" % args.calls)
            fh.write("\n".join(lines) + "\n")
    if made:
        shutil.rmtree(args.out, ignore_errors=True)


if __name__ == "__main__":
    main()
