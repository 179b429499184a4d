"""Cost of LDA.heldout_ranks_gamma (csrc/ranks_kernels.h) next to LDA.recommend_gamma(top_n=100) of the
same library at the same shape -- the same product behind the other epilogue, so the difference is
what counting costs -- and next to the same answer written with torch on the device: fp64
``theta @ beta`` (a B x V matrix), the seen words masked out, a compare-and-sum against each held-out
score.

    heldout_ranks_gamma   whole calls (upload of gamma, row sums of lambda, q rows, seen bits, the
    recommend_gamma       thresholds and the counting sweep / the ranked product and merge, download;
                          the call ends in a synchronise): host clock, median of --calls
    torch                 the product, the mask and the counts between two events on torch's stream

All after a warm-up call.  Every document has 30 seen and 20 held-out entries.  Flops per call are
computed from the shapes: the product 2 B V Kp, the thresholds' gather product 2 * 64 nnz Kp.

    python tools/ranks_rate.py [--configs k100,k500] [--calls N] [--out profiles/ranks_rate.txt]

Run on the GPU box from the repo root.  Every GPU step (a configuration's model and its three
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
    # name: (K, V, B)
    "k100": (100, 7000, 200),
    "k500": (500, 100000, 4096),
    "tiny": (20, 500, 40),               # rehearsal size
}
STEP_SECONDS = 600
SEEN_PER_DOC = 30
HELD_PER_DOC = 20


def step(name, calls):
    import torch
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.models import OnlineLDA
    K, V, B = CONFIGS[name]
    Kp = (K + 3) // 4 * 4
    rng = np.random.RandomState(5)
    lam_t = rng.gamma(2.0, 1.0, size=(V, K)) + 0.05              # word-major: lam_t.T is K x V column-major
    gamma = np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, B)) + 0.01)
    ids = rng.randint(0, V, size=B * SEEN_PER_DOC).astype(np.int32)      # (a repeated word counts once)
    held = rng.randint(0, V, size=B * HELD_PER_DOC).astype(np.int32)
    docs = CSRDocuments(np.arange(B + 1) * SEEN_PER_DOC, ids, np.ones_like(ids))
    hdocs = CSRDocuments(np.arange(B + 1) * HELD_PER_DOC, held, np.ones_like(held))
    model = OnlineLDA.__new__(OnlineLDA)
    model._num_documents, model._update_count = 1000, 0
    model._ada_tau, model._ada_rho, model._ada_sq_norm = 1000., 1e-3, 1.
    model._setup(V, K, .1, .3, 0, _lambda=lam_t.T)
    batch, hbatch = model.upload(docs), model.upload(hdocs)

    def clock(call):
        call()                                                   # warm-up
        times = []
        for _ in range(calls):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        return times

    indptr, words, ranks, cand = model.heldout_ranks_gamma(gamma, hbatch, docs=batch)
    t_ranks = clock(lambda: model.heldout_ranks_gamma(gamma, hbatch, docs=batch))
    t_rec = clock(lambda: model.recommend_gamma(gamma, top_n=100, docs=batch))
    batch.close()
    hbatch.close()
    model.close()

    # the same answer with torch
    lam_d = torch.from_numpy(lam_t).cuda()                       # V x K
    beta = (lam_d / lam_d.sum(dim=0)).T.contiguous()             # K x V
    g = torch.from_numpy(np.ascontiguousarray(gamma.T)).cuda()   # B x K
    theta = g / g.sum(dim=1, keepdim=True)
    rows = torch.from_numpy(np.repeat(np.arange(B), SEEN_PER_DOC)).cuda()
    cols = torch.from_numpy(ids.astype(np.int64)).cuda()
    held_d = torch.from_numpy(held.astype(np.int64).reshape(B, HELD_PER_DOC)).cuda()
    word = torch.arange(V, device="cuda")[None, :]
    doc = torch.arange(B, device="cuda")

    def torch_ranks():
        s = theta @ beta
        own = s[doc[:, None], held_d]                            # B x 20, before the mask
        s[rows, cols] = -float("inf")
        out = torch.empty((B, HELD_PER_DOC), dtype=torch.int64, device="cuda")
        for j in range(HELD_PER_DOC):
            v, h = own[:, j, None], held_d[:, j, None]
            out[:, j] = 1 + ((s > v) | ((s == v) & (word < h))).sum(dim=1)
        return out

    t_out = torch_ranks()                                        # warm-up
    torch.cuda.synchronize()
    ttimes = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_ranks()
        e1.record()
        e1.synchronize()
        ttimes.append(e0.elapsed_time(e1) * 1e-3)
    # (torch's scores have other bits: compare the ranks of the words both rank, entry by entry)
    t_out = t_out.cpu().numpy()
    same, total = 0, 0
    for d in range(B):
        mine = dict(zip(words[indptr[d]:indptr[d + 1]].tolist(), ranks[indptr[d]:indptr[d + 1]].tolist()))
        for j in range(HELD_PER_DOC):
            if int(held[d * HELD_PER_DOC + j]) in mine:
                total += 1
                same += mine[int(held[d * HELD_PER_DOC + j])] == int(t_out[d, j])
    ours, rec, theirs = float(np.median(t_ranks)), float(np.median(t_rec)), float(np.median(ttimes))
    nnz = B * HELD_PER_DOC
    flops, gather_flops = 2.0 * B * V * Kp, 2.0 * 64 * nnz * Kp
    print(json.dumps({
        "config": name, "K": K, "V": V, "B": B, "seen_per_document": SEEN_PER_DOC,
        "heldout_per_document": HELD_PER_DOC, "relevant_pairs": int(len(words)), "calls": calls,
        "heldout_ranks_gamma_ms_median": round(ours * 1e3, 3), "heldout_ranks_gamma_ms_min": round(min(t_ranks) * 1e3, 3),
        "recommend_gamma_top100_ms_median": round(rec * 1e3, 3), "recommend_gamma_top100_ms_min": round(min(t_rec) * 1e3, 3),
        "torch_ms_median": round(theirs * 1e3, 3), "torch_ms_min": round(min(ttimes) * 1e3, 3),
        "ranks_over_recommend": round(ours / rec, 3), "torch_over_ranks": round(theirs / ours, 3),
        "lambda_bytes": K * V * 8, "product_flops": flops, "gather_flops": gather_flops,
        "torch_matrix_bytes": B * V * 8, "heldout_ranks_gamma_TFLOPs": round(flops / ours / 1e12, 2),
        "ranks_equal_share": round(same / max(total, 1), 6)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="k100,k500")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranks_rate.txt"))
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
        f.write("# python tools/ranks_rate.py --configs %s --calls %d\n" % (args.configs, args.calls))
        f.writelines(lines)
    return done.returncode


if __name__ == "__main__":
    sys.exit(main())
