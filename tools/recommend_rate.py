"""Cost of LDA.recommend_gamma (csrc/recommend_kernels.h) next to the same answer written with torch
on the device: fp64 ``theta @ beta`` (a B x V matrix), the seen words masked out, ``torch.topk``.

    recommend_gamma   whole calls (upload of gamma, row sums of lambda, q rows, seen bits, the ranked
                      product, merge, download of the B x top_n results; the call ends in a
                      synchronise): host clock, median of --calls
    torch             the product, the mask and the top-k between two events on torch's stream

Both after a warm-up call.  Bytes and flops per call are computed from the shapes: lambda is
K V 8 bytes, the product 2 B V Kp flops, the B x V matrix torch forms B V 8 bytes.

    python tools/recommend_rate.py [--configs k100,k500] [--calls N] [--out profiles/recommend_rate.txt]

Run on the GPU box from the repo root.  Every GPU step (a configuration's model and its two timings)
is a child process under its own `timeout`; after a step that fails nothing more is started.
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
    # name: (K, V, B, top_n)
    "k100": (100, 7000, 200, 10),
    "k500": (500, 100000, 4096, 20),
    "tiny": (20, 500, 40, 10),           # rehearsal size
}
STEP_SECONDS = 600
SEEN_PER_DOC = 30


def step(name, calls):
    import torch
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.models import OnlineLDA
    K, V, B, top_n = CONFIGS[name]
    Kp = (K + 3) // 4 * 4
    rng = np.random.RandomState(5)
    lam_t = rng.gamma(2.0, 1.0, size=(V, K)) + 0.05              # word-major: lam_t.T is K x V column-major
    gamma = np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, B)) + 0.01)
    n_seen = min(SEEN_PER_DOC, V // 2)
    ids = rng.randint(0, V, size=B * n_seen).astype(np.int32)    # (a repeated word counts once)
    docs = CSRDocuments(np.arange(B + 1) * n_seen, ids, np.ones_like(ids))
    model = OnlineLDA.__new__(OnlineLDA)
    model._num_documents, model._update_count = 1000, 0
    model._ada_tau, model._ada_rho, model._ada_sq_norm = 1000., 1e-3, 1.
    model._setup(V, K, .1, .3, 0, _lambda=lam_t.T)
    batch = model.upload(docs)
    words, probs = model.recommend_gamma(gamma, top_n=top_n, docs=batch)         # warm-up
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        model.recommend_gamma(gamma, top_n=top_n, docs=batch)
        times.append(time.perf_counter() - t0)
    ours = float(np.median(times))
    batch.close()
    model.close()

    # the same answer with torch
    lam_d = torch.from_numpy(lam_t).cuda()                       # V x K
    beta = (lam_d / lam_d.sum(dim=0)).T.contiguous()             # K x V
    g = torch.from_numpy(np.ascontiguousarray(gamma.T)).cuda()   # B x K
    theta = g / g.sum(dim=1, keepdim=True)
    rows = torch.from_numpy(np.repeat(np.arange(B), n_seen)).cuda()
    cols = torch.from_numpy(ids.astype(np.int64)).cuda()

    def torch_recommend():
        s = theta @ beta
        s[rows, cols] = -float("inf")
        return torch.topk(s, top_n, dim=1)

    t_probs, t_words = torch_recommend()                         # warm-up
    torch.cuda.synchronize()
    ttimes = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_recommend()
        e1.record()
        e1.synchronize()
        ttimes.append(e0.elapsed_time(e1) * 1e-3)
    theirs = float(np.median(ttimes))
    # (torch.topk does not order equal values by id: compare the values, and the ids where they differ)
    same_ids = float(np.mean(t_words.cpu().numpy() == words))
    rel_diff = float(np.max(np.abs(t_probs.cpu().numpy() - probs) / probs))
    lambda_bytes, flops = K * V * 8, 2.0 * B * V * Kp
    print(json.dumps({
        "config": name, "K": K, "V": V, "B": B, "top_n": top_n, "seen_per_document": n_seen, "calls": calls,
        "recommend_gamma_ms_median": round(ours * 1e3, 3), "recommend_gamma_ms_min": round(min(times) * 1e3, 3),
        "torch_ms_median": round(theirs * 1e3, 3), "torch_ms_min": round(min(ttimes) * 1e3, 3),
        "lambda_bytes": lambda_bytes, "flops": flops, "torch_matrix_bytes": B * V * 8,
        "recommend_gamma_TFLOPs": round(flops / ours / 1e12, 2), "torch_TFLOPs": round(flops / theirs / 1e12, 2),
        "ids_equal_share": round(same_ids, 6), "max_rel_prob_difference": rel_diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="k100,k500")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend_rate.txt"))
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
        f.write("# python tools/recommend_rate.py --configs %s --calls %d\n" % (args.configs, args.calls))
        f.writelines(lines)
    return done.returncode


if __name__ == "__main__":
    sys.exit(main())
