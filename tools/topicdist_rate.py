"""Cost of LDA.topic_distances (csrc/topicdist_kernels.h) next to the Hellinger distance written with
torch on the device: ``P = L / L.sum(1)``, ``sqrt(P) @ sqrt(Q).T`` in fp64, the closing formula.

    topic_distances   whole calls for each measure (row statistics, product or Jensen-Shannon kernel,
                      combine, download of the K x K' matrix; the call ends in a synchronise): host
                      clock, median of --calls
    torch             normalisation, roots, product and closing formula between two events on torch's
                      stream, both lambdas already on the device

Both after a warm-up call.  Flops per call are 2 K K' V for the three products; Jensen-Shannon is
K K' V logarithms.

    python tools/topicdist_rate.py [--configs k500,k100] [--calls N] [--out profiles/topicdist_rate.txt]

Run on the GPU box from the repo root.  Every GPU step (a configuration's two models and its
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
    # name: (K, K', V)
    "k500": (500, 500, 100000),
    "k100": (100, 100, 7000),            # the headline shape of bench.py
    "tiny": (20, 24, 300),               # rehearsal size
}
MEASURES = ("hellinger", "cosine", "kl", "jensen_shannon")
STEP_SECONDS = 300


def _lambda(K, V, seed):
    rng = np.random.RandomState(seed)
    return np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, V)) * rng.uniform(0.5, 40, size=(K, 1)) + 0.01)


def _model(lam):
    from trlda_amd.models import OnlineLDA
    model = OnlineLDA.__new__(OnlineLDA)
    model._num_documents, model._update_count = 1000, 0
    model._ada_tau, model._ada_rho, model._ada_sq_norm = 1000., 1e-3, 1.
    model._setup(lam.shape[1], lam.shape[0], .1, .3, 0, _lambda=lam)
    return model


def step(name, calls):
    import torch
    K, K2, V = CONFIGS[name]
    lam, mu = _lambda(K, V, 1), _lambda(K2, V, 2)
    a, b = _model(lam), _model(mu)
    result = {"config": name, "K": K, "K2": K2, "V": V, "calls": calls, "flops": 2.0 * K * K2 * V}
    ours = None
    for measure in MEASURES:
        D = a.topic_distances(b, measure)                                        # warm-up
        times = []
        for _ in range(calls):
            t0 = time.perf_counter()
            a.topic_distances(b, measure)
            times.append(time.perf_counter() - t0)
        result[measure + "_ms_median"] = round(float(np.median(times)) * 1e3, 3)
        result[measure + "_ms_min"] = round(min(times) * 1e3, 3)
        if measure == "hellinger":
            ours = D
            result["hellinger_TFLOPs"] = round(result["flops"] / float(np.median(times)) / 1e12, 2)

    L, M = torch.from_numpy(np.ascontiguousarray(lam)).cuda(), torch.from_numpy(np.ascontiguousarray(mu)).cuda()

    def torch_hellinger():
        P, Q = L / L.sum(dim=1, keepdim=True), M / M.sum(dim=1, keepdim=True)
        return torch.sqrt(torch.clamp(1 - torch.sqrt(P) @ torch.sqrt(Q).T, min=0))

    theirs = torch_hellinger()                                                   # warm-up
    torch.cuda.synchronize()
    ttimes = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_hellinger()
        e1.record()
        e1.synchronize()
        ttimes.append(e0.elapsed_time(e1) * 1e-3)
    result["torch_hellinger_ms_median"] = round(float(np.median(ttimes)) * 1e3, 3)
    result["torch_hellinger_ms_min"] = round(min(ttimes) * 1e3, 3)
    result["torch_hellinger_TFLOPs"] = round(result["flops"] / float(np.median(ttimes)) / 1e12, 2)
    result["max_abs_difference_of_squares"] = float(np.max(np.abs(theirs.cpu().numpy() ** 2 - ours ** 2)))
    print(json.dumps(result), flush=True)
    b.close()
    a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="k500,k100")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topicdist_rate.txt"))
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
        f.write("# python tools/topicdist_rate.py --configs %s --calls %d\n" % (args.configs, args.calls))
        f.writelines(lines)
    return done.returncode


if __name__ == "__main__":
    sys.exit(main())
