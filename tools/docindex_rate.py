"""Cost of DocumentIndex.query_gamma (csrc/docindex_kernels.h) next to the same search written with
torch on the same rows: fp64 ``Q @ R.T`` over chunks of the index, ``torch.topk`` per chunk, then a
merge of the chunks' lists.

    query_gamma   whole calls (upload of gamma, rows of the queries, search, merge, download of the
                  B x top_n results; the call ends in a synchronise): host clock, median of --calls
    torch         the chunks' products, top-k and merge between two events on torch's stream

Both after a warm-up call.  Bytes and flops per call are computed from the shapes: the table is
N Kp 8 bytes, the product 2 N B Kp flops.

    python tools/docindex_rate.py [--configs k100,k500] [--calls N] [--out profiles/docindex_rate.txt]

Run on the GPU box from the repo root.  Every GPU step (a configuration's index and its two
timings) is a child process under its own `timeout`; after a step that fails nothing more is started.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (K, N, B, top_n)
    "k100": (100, 1000000, 200, 10),
    "k500": (500, 200000, 200, 10),
    "tiny": (20, 5000, 40, 10),          # rehearsal size
}
STEP_SECONDS = 240
ADD_CHUNK = 100000
TORCH_CHUNK = 65536


def _gammas(K, n, seed):
    rng = np.random.RandomState(seed)
    return np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, n)) + 0.01)


def step(name, calls):
    import torch
    from trlda_amd.models import OnlineLDA
    K, N, B, top_n = CONFIGS[name]
    Kp = (K + 3) // 4 * 4
    model = OnlineLDA.__new__(OnlineLDA)
    model._num_documents, model._update_count = 1000, 0
    model._ada_tau, model._ada_rho, model._ada_sq_norm = 1000., 1e-3, 1.
    model._setup(8, K, .1, .3, 0, _lambda=np.ones((K, 8), order="F"))
    index = model.document_index()
    index.reserve(N)
    for at in range(0, N, ADD_CHUNK):
        index.add_gamma(_gammas(K, min(ADD_CHUNK, N - at), 100 + at))
    gq = _gammas(K, B, 7)
    ids, sim = index.query_gamma(gq, top_n=top_n, return_similarity=True)        # warm-up
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        index.query_gamma(gq, top_n=top_n, return_similarity=True)
        times.append(time.perf_counter() - t0)
    ours = float(np.median(times))

    # the same search with torch on the device's own rows
    qix = model.document_index()
    qix.add_gamma(gq)
    Q = torch.from_numpy(qix.rows()).cuda()
    R = torch.empty((N, K), dtype=torch.float64, device="cuda")
    for at in range(0, N, ADD_CHUNK):
        n = min(ADD_CHUNK, N - at)
        R[at:at + n] = torch.from_numpy(index.rows(at, n)).cuda()

    def torch_search():
        vals, idx = [], []
        for at in range(0, N, TORCH_CHUNK):
            s = Q @ R[at:at + TORCH_CHUNK].T
            v, i = torch.topk(s, min(top_n, s.shape[1]), dim=1)
            vals.append(v)
            idx.append(i + at)
        v, i = torch.cat(vals, dim=1), torch.cat(idx, dim=1)
        best, pos = torch.topk(v, top_n, dim=1)
        return torch.gather(i, 1, pos), best

    t_ids, t_sim = torch_search()                                                # warm-up
    torch.cuda.synchronize()
    ttimes = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_search()
        e1.record()
        e1.synchronize()
        ttimes.append(e0.elapsed_time(e1) * 1e-3)
    theirs = float(np.median(ttimes))
    # (torch.topk does not order equal values by id: compare the similarities, and the ids where they differ)
    same_ids = float(np.mean(t_ids.cpu().numpy() == ids))
    sim_diff = float(np.max(np.abs(t_sim.cpu().numpy() - sim)))
    table_bytes, flops = N * Kp * 8, 2.0 * N * B * Kp
    print(json.dumps({
        "config": name, "K": K, "N": N, "B": B, "top_n": top_n, "calls": calls,
        "query_gamma_ms_median": round(ours * 1e3, 3), "query_gamma_ms_min": round(min(times) * 1e3, 3),
        "torch_ms_median": round(theirs * 1e3, 3), "torch_ms_min": round(min(ttimes) * 1e3, 3),
        "table_bytes": table_bytes, "flops": flops,
        "query_gamma_TFLOPs": round(flops / ours / 1e12, 2), "torch_TFLOPs": round(flops / theirs / 1e12, 2),
        "query_gamma_table_GBps": round(table_bytes / ours / 1e9, 1),
        "ids_equal_share": round(same_ids, 6), "max_abs_similarity_difference": sim_diff}), flush=True)
    model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="k100,k500")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "docindex_rate.txt"))
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.calls)
        return 0
    lines = []
    for name in args.configs.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", name,
               "--calls", str(args.calls)]
        done = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        sys.stdout.write(done.stdout)
        sys.stderr.write(done.stderr[-2000:])
        lines.append(done.stdout)
        if done.returncode != 0:                     # nothing more is started on the GPU after a failure
            lines.append("step %s ended with status %d\n" % (name, done.returncode))
            break
    with open(args.out, "w") as f:
        f.write("# python tools/docindex_rate.py --configs %s --calls %d\n" % (args.configs, args.calls))
        f.writelines(lines)
    return done.returncode


if __name__ == "__main__":
    sys.exit(main())
