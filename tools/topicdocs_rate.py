"""Cost of DocumentIndex.topic_documents and DocumentIndex.topic_covariance (csrc/topicdocs_kernels.h)
next to the same work written with torch on the same rows: theta = R * R, ``torch.topk`` of theta.T per
topic, and the centred fp64 product ``(theta - m).T @ (theta - m)``.

    topic_documents / topic_covariance   whole calls (every temporary allocated and freed, the kernels,
                                         the download of the small result; the call ends in a
                                         synchronise): host clock, median of --calls
    torch                                the same work between two events on torch's stream

Both after a warm-up call.  Bytes and flops per call are computed from the shapes: the table is
N Kp 8 bytes (read once by the selection; once by the mean and once per tile column by the scatter),
the scatter 2 N K^2 flops as a full product (the kernel forms the T (T + 1) / 2 tiles of 64 x 64 with
ti <= tj, T = ceil(K / 64)).

    python tools/topicdocs_rate.py [--configs k100,k500] [--calls N] [--out profiles/topicdocs_rate.txt]

Run on the GPU box from the repo root.  Every GPU step (a configuration's index and its timings) is
a child process under its own `timeout`; after a step that fails nothing more is started.
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
    # name: (K, N, top_n)
    "k100": (100, 1000000, 10),
    "k500": (500, 200000, 10),
    "tiny": (20, 5000, 10),              # rehearsal size
}
STEP_SECONDS = 240
ADD_CHUNK = 100000


def _gammas(K, n, seed):
    rng = np.random.RandomState(seed)
    return np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, n)) + 0.01)


def _host_median(call, calls):
    call()                                                                       # warm-up
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(min(times))


def step(name, calls):
    import torch
    from trlda_amd.models import OnlineLDA
    K, N, top_n = CONFIGS[name]
    Kp = (K + 3) // 4 * 4
    model = OnlineLDA.__new__(OnlineLDA)
    model._num_documents, model._update_count = 1000, 0
    model._ada_tau, model._ada_rho, model._ada_sq_norm = 1000., 1e-3, 1.
    model._setup(8, K, .1, .3, 0, _lambda=np.ones((K, 8), order="F"))
    index = model.document_index()
    index.reserve(N)
    for at in range(0, N, ADD_CHUNK):
        index.add_gamma(_gammas(K, min(ADD_CHUNK, N - at), 100 + at))
    docs_med, docs_min = _host_median(lambda: index.topic_documents(top_n, return_theta=True), calls)
    cov_med, cov_min = _host_median(lambda: index.topic_covariance(return_mean=True), calls)
    ids, theta = index.topic_documents(top_n, return_theta=True)
    cov, mean = index.topic_covariance(return_mean=True)

    # the same work with torch on the device's own rows
    R = torch.empty((N, K), dtype=torch.float64, device="cuda")
    for at in range(0, N, ADD_CHUNK):
        n = min(ADD_CHUNK, N - at)
        R[at:at + n] = torch.from_numpy(index.rows(at, n)).cuda()

    def torch_documents():
        return torch.topk((R * R).T, top_n, dim=1)

    def torch_covariance():
        t = R * R
        m = t.mean(dim=0)
        c = t - m
        return (c.T @ c) / (N - 1), m

    def device_median(call):
        call()                                                                   # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        return float(np.median(times)), float(min(times))

    tdocs_med, tdocs_min = device_median(torch_documents)
    tcov_med, tcov_min = device_median(torch_covariance)
    t_theta, t_ids = torch_documents()
    t_cov, _ = torch_covariance()
    # (torch.topk does not order equal values by id: compare the values, and the ids where they differ)
    same_ids = float(np.mean(t_ids.cpu().numpy() == ids))
    theta_diff = float(np.max(np.abs(t_theta.cpu().numpy() - theta)))
    cov_diff = float(np.max(np.abs(t_cov.cpu().numpy() - cov)))
    table_bytes, flops = N * Kp * 8, 2.0 * N * K * K
    print(json.dumps({
        "config": name, "K": K, "N": N, "top_n": top_n, "calls": calls,
        "topic_documents_ms_median": round(docs_med * 1e3, 3), "topic_documents_ms_min": round(docs_min * 1e3, 3),
        "torch_topk_ms_median": round(tdocs_med * 1e3, 3), "torch_topk_ms_min": round(tdocs_min * 1e3, 3),
        "topic_covariance_ms_median": round(cov_med * 1e3, 3), "topic_covariance_ms_min": round(cov_min * 1e3, 3),
        "torch_covariance_ms_median": round(tcov_med * 1e3, 3), "torch_covariance_ms_min": round(tcov_min * 1e3, 3),
        "table_bytes": table_bytes, "scatter_flops": flops,
        "topic_documents_table_GBps": round(table_bytes / docs_med / 1e9, 1),
        "topic_covariance_TFLOPs": round(flops / cov_med / 1e12, 2),
        "torch_covariance_TFLOPs": round(flops / tcov_med / 1e12, 2),
        "ids_equal_share": round(same_ids, 6), "max_abs_theta_difference": theta_diff,
        "max_abs_covariance_difference": cov_diff}), flush=True)
    model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="k100,k500")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topicdocs_rate.txt"))
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
        f.write("# python tools/topicdocs_rate.py --configs %s --calls %d\n" % (args.configs, args.calls))
        f.writelines(lines)
    return done.returncode


if __name__ == "__main__":
    sys.exit(main())
