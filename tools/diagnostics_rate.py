"""Device time of LDA.topic_word_diagnostics per call next to LDA.word_statistics and LDA.top_words,
and of LDA.topic_document_diagnostics_gamma next to LDA.topic_prevalence_gamma
(csrc/diagnostics_kernels.h, csrc/relevance_kernels.h, csrc/coherence_kernels.h), on the same model in
the same run.

The calls run in a child process under `rocprofv3 --kernel-trace --stats`: `calls` calls of
top_words(10), of word_statistics(), of topic_word_diagnostics(10), then per batch size B `calls` calls
of topic_prevalence_gamma and of topic_document_diagnostics_gamma on the same gamma and documents.  The
kernel trace is read back, cut into the phases at the first dispatch of each phase's own kernel, and
the dispatches of each phase (the buffer fills between them included) are summed and divided by the
number of calls.

    python tools/diagnostics_rate.py [--configs k100,k500] [--calls N] [--out DIR] [--write]

Run from the repo root on a machine with the GPU; one JSON line per configuration.  `--write` also
puts the lines into profiles/diagnostics_rate.txt.
"""
import argparse
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

from tools.relevance_rate import CONFIGS, _phase, _trace  # noqa: E402

BATCHES = (200, 1600)
KERNELS = ("topn_", "relevance_", "rowsum_", "diagnostics_", "prevalence_", "topicdiag_", "fillBuffer")


def child(name, calls):
    from trlda_amd import _ffi
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils.synthetic import make_corpus
    _ffi.require_gpu()
    K, V, n = CONFIGS[name]
    rng = np.random.RandomState(1)
    m = OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.01, device=0)
    m.lambdas = rng.gamma(0.3, 1.0, size=(K, V)) + 0.01
    host = {}

    def timed(what, call):
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        host[what + "_host_ms"] = round(float(np.median(ms)), 3)

    timed("top_words", lambda: m.top_words(n))
    timed("word_statistics", m.word_statistics)
    timed("topic_word_diagnostics", lambda: m.topic_word_diagnostics(n))
    for B in BATCHES:
        batch = m.upload(CSRDocuments(*make_corpus(B, V, seed=7, mean_unique=40)))
        gamma = np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, B)) + 0.01)
        timed("topic_prevalence_gamma_b%d" % B, lambda: m.topic_prevalence_gamma(gamma, batch))
        timed("topic_document_diagnostics_gamma_b%d" % B, lambda: m.topic_document_diagnostics_gamma(gamma, batch))
        batch.close()
    m.close()
    print(json.dumps(host), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--write", action="store_true", help="also write profiles/diagnostics_rate.txt")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.calls)
    made = args.out is None                   # (a temporary directory of our own is removed at the end)
    if made:
        args.out = tempfile.mkdtemp(prefix="diagnostics_rate_")
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
        rows = [r for r in _trace(out_dir) if any(k in r[2] for k in KERNELS)]

        def first(what, after=0):
            return min(i for i, r in enumerate(rows) if i >= after and what in r[2])

        # the phases: top_words from its first tile kernel; word_statistics from the row sums before
        # the first column pass; topic_word_diagnostics from the first tile kernel after that (its
        # top_words) to its last mean kernel; then per batch size the prevalence's and the
        # diagnostics' document kernels in turn (what came before: the model's set-up)
        cuts = [first("topn_tile")]
        first_col = first("relevance_column")
        cuts.append(max(i for i in range(first_col) if "rowsum_partial" in rows[i][2]))
        cuts.append(first("topn_tile", first_col))
        cuts.append(max(i for i, r in enumerate(rows) if "diagnostics_mean" in r[2]) + 1)
        for _ in BATCHES:
            cuts[-1] = first("prevalence_docs", cuts[-1])
            cuts.append(first("topicdiag_docs", cuts[-1]))
            cuts.append(cuts[-1])
        cuts[-1] = len(rows)
        names = ["top_words", "word_statistics", "topic_word_diagnostics"]
        for B in BATCHES:
            names += ["topic_prevalence_gamma_b%d" % B, "topic_document_diagnostics_gamma_b%d" % B]
        us, kernels = {}, {}
        for what, lo, hi in zip(names, cuts[:-1], cuts[1:]):
            us[what + "_us"], kernels[what] = _phase(rows[lo:hi], args.calls)
        extra = us["topic_word_diagnostics_us"] - us["top_words_us"] - us["word_statistics_us"]
        line = json.dumps({
            "config": name, "K": K, "V": V, "top_n": n, "calls": args.calls, **info, **us,
            "diagnostics_beyond_top_words_and_word_statistics_us": round(extra, 2),
            "lambda_read_us_at_4TBps": round(8.0 * K * V / 4e6, 2), "kernels_us": kernels,
        })
        print(line, flush=True)
        lines.append(line)
    if args.write:
        with open(os.path.join(ROOT, "profiles", "diagnostics_rate.txt"), "w") as fh:
            fh.write("# python tools/diagnostics_rate.py --calls %d --write\n" % args.calls)
            fh.write("\n".join(lines) + "\n")
    if made:
        shutil.rmtree(args.out, ignore_errors=True)


if __name__ == "__main__":
    main()
