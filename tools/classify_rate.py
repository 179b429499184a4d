"""Cost of the classifier of an indexed corpus (csrc/classify_kernels.h): one evaluation of
the loss and its gradient on the device, a whole ``DocumentIndex.fit_classifier``, and the same fit with
the same optimiser driven by a float64 NumPy statement of the objective on the host.

    evaluation        trlda_docindex_classify_eval with the labels already on the device (C x K doubles up,
                      the kernels, 1 + C x K doubles down, one synchronise): host clock, median of --calls
    fit_classifier    the whole call (labels and weights checked and uploaded, every evaluation, the scratch
                      freed): host clock, one call after a warm-up call
    numpy             lbfgs_minimize on ``fun(W)`` in float64 NumPy over the index's own theta^ on the host
                      (BLAS products, the host's threads): host clock, one call
    kernels           ``--stats CSV``: the device time of classify_forward_kernel and of
                      effects_products_kernel from a ``rocprofv3 --kernel-trace --stats`` run of
                      ``--step evals`` (a run of its own), each against its byte floor -- forward: the table
                      read once and R written once; cross product: the table and R read once -- as a share
                      of the HBM peak (8.0 TB/s)

    python tools/classify_rate.py [--config k100] [--calls N] [--out profiles/classify_rate.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/classify_rate.py --step evals
    python tools/classify_rate.py --stats DIR/.../..._kernel_stats.csv

Run on the GPU box from the repo root.  Every GPU step is a child process under its own `timeout`;
after a step that fails nothing more is started.
"""
import argparse
import csv
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
    # name: (K, N, C)
    "k100": (100, 1000000, 20),
    "tiny": (20, 5000, 4),                # rehearsal size
}
STEP_SECONDS = 400
ADD_CHUNK = 100000
HBM_PEAK = 8.0e12
L2, TOL = 1e-4, 1e-6                      # fit_classifier's defaults


def _gammas(K, n, seed):
    rng = np.random.RandomState(seed)
    return np.asfortranarray(rng.gamma(0.3, 1.0, size=(K, n)) + 0.01)


def _setup(name):
    from trlda_amd.models import OnlineLDA
    K, N, C = CONFIGS[name]
    model = OnlineLDA.__new__(OnlineLDA)
    model._num_documents, model._update_count = 1000, 0
    model._ada_tau, model._ada_rho, model._ada_sq_norm = 1000., 1e-3, 1.
    model._setup(8, K, .1, .3, 0, _lambda=np.ones((K, 8), order="F"))
    index = model.document_index()
    index.reserve(N)
    for at in range(0, N, ADD_CHUNK):
        index.add_gamma(_gammas(K, min(ADD_CHUNK, N - at), 100 + at))
    rng = np.random.RandomState(7)
    # labels that depend on theta through a hidden coefficient matrix, a tenth left out
    theta = np.empty((N, K))
    for at in range(0, N, ADD_CHUNK):
        n = min(ADD_CHUNK, N - at)
        r = index.rows(at, n)
        theta[at:at + n] = r * r
    true = rng.normal(size=(C, K)) * 8.0
    labels = np.argmax(theta.dot(true.T) + rng.gumbel(size=(N, C)), axis=1).astype(np.int32)
    labels[rng.permutation(N)[:N // 10]] = -1
    return model, index, theta, labels


def _numpy_fun(theta, labels, l2):
    keep = np.flatnonzero(labels >= 0)
    t, y = theta[keep], labels[keep]
    rows = np.arange(len(keep))
    omega = float(len(keep))

    def fun(W):
        z = t.dot(W.T)
        m = z.max(axis=1)
        e = np.exp(z - m[:, None])
        S = e.sum(axis=1)
        loss = float(((np.log(S) + m) - z[rows, y]).sum())
        r = e / S[:, None]
        r[rows, y] -= 1.0
        return loss / omega + 0.5 * l2 * float(np.sum(W * W)), r.T.dot(t) / omega + l2 * W
    return fun


def step_time(name, calls):
    from trlda_amd import _ffi
    from trlda_amd.index import lbfgs_minimize
    K, N, C = CONFIGS[name]
    model, index, theta, labels = _setup(name)
    lib, handle = _ffi.lib(), index._handle
    W = np.ascontiguousarray(np.random.RandomState(3).normal(size=(C, K)))
    omega, counts = np.zeros(1), np.zeros(C, dtype=np.int64)
    loss, grad = np.zeros(1), np.empty((C, K))
    _ffi.check(lib.trlda_docindex_classify_set(handle, labels.ctypes.data, C, None, omega.ctypes.data,
                                               counts.ctypes.data))
    times = []
    for i in range(calls + 1):                                                   # (the first: warm-up)
        t0 = time.perf_counter()
        _ffi.check(lib.trlda_docindex_classify_eval(handle, W.ctypes.data, loss.ctypes.data, grad.ctypes.data))
        times.append(time.perf_counter() - t0)
    _ffi.check(lib.trlda_docindex_classify_clear(handle))
    times = times[1:]
    index.fit_classifier(labels, num_classes=C, max_iter=2)                      # warm-up
    t0 = time.perf_counter()
    fit = index.fit_classifier(labels, num_classes=C)
    fit_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = lbfgs_minimize(_numpy_fun(theta, labels, L2), np.zeros((C, K)), max_iter=200, tol=TOL)
    host_s = time.perf_counter() - t0
    train = index.predict(fit["coef"])
    Kp, Cp = (K + 3) // 4 * 4, (C + 3) // 4 * 4
    print(json.dumps({
        "config": name, "K": K, "N": N, "C": C, "calls": calls,
        "eval_call_ms_median": round(float(np.median(times)) * 1e3, 3), "eval_call_ms_min": round(min(times) * 1e3, 3),
        "eval_flops": 4.0 * N * K * C, "table_bytes": N * Kp * 8, "R_bytes": N * Cp * 8,
        "fit_classifier_s": round(fit_s, 3), "fit_iterations": fit["iterations"], "fit_evaluations": fit["evaluations"],
        "fit_converged": fit["converged"], "fit_loss": fit["loss"],
        "numpy_fit_s": round(host_s, 3), "numpy_iterations": host["iterations"],
        "numpy_evaluations": host["evaluations"],
        "numpy_converged": host["converged"], "numpy_loss": host["loss"],
        "max_abs_coef_difference": float(np.max(np.abs(host["coef"] - fit["coef"]))),
        "training_accuracy": float(np.mean(train[labels >= 0] == labels[labels >= 0])),
        "host_threads": os.environ.get("OMP_NUM_THREADS", "unset")}), flush=True)
    model.close()


def step_evals(name, calls):
    """What the kernel trace is taken of: the labels set once, then `calls` evaluations."""
    from trlda_amd import _ffi
    K, N, C = CONFIGS[name]
    model, index, theta, labels = _setup(name)
    lib, handle = _ffi.lib(), index._handle
    W = np.ascontiguousarray(np.random.RandomState(3).normal(size=(C, K)))
    omega, counts = np.zeros(1), np.zeros(C, dtype=np.int64)
    loss, grad = np.zeros(1), np.empty((C, K))
    _ffi.check(lib.trlda_docindex_classify_set(handle, labels.ctypes.data, C, None, omega.ctypes.data,
                                               counts.ctypes.data))
    for _ in range(calls):
        _ffi.check(lib.trlda_docindex_classify_eval(handle, W.ctypes.data, loss.ctypes.data, grad.ctypes.data))
    _ffi.check(lib.trlda_docindex_classify_clear(handle))
    print("loss_sum %.17g after %d evaluations" % (loss[0], calls), flush=True)
    model.close()


def stats(path, name):
    """The two kernels of an evaluation in a rocprofv3 kernel_stats.csv against their byte floors."""
    K, N, C = CONFIGS[name]
    Kp, Cp = (K + 3) // 4 * 4, (C + 3) // 4 * 4
    floors = {"classify_forward_kernel": N * Kp * 8 + N * Cp * 8, "effects_products_kernel": N * Kp * 8 + N * Cp * 8}
    out = {"config": name, "K": K, "N": N, "C": C, "hbm_peak_Bps": HBM_PEAK}
    with open(path) as f:
        for row in csv.DictReader(f):
            for kernel, floor in floors.items():
                if kernel in row["Name"]:
                    mean_ns = float(row["AverageNs"])
                    out[kernel] = {"calls": int(row["Calls"]), "mean_us": round(mean_ns * 1e-3, 2),
                                   "floor_bytes": floor, "floor_us_at_peak": round(floor / HBM_PEAK * 1e6, 2),
                                   "GBps": round(floor / mean_ns, 1),
                                   "share_of_hbm_peak": round(floor / mean_ns * 1e9 / HBM_PEAK, 4)}
    print(json.dumps(out), flush=True)
    return 0 if all(k in out for k in floors) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="k100")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify_rate.txt"))
    ap.add_argument("--step", default=None, choices=["time", "evals"], help=argparse.SUPPRESS)
    ap.add_argument("--stats", default=None)
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats, args.config)
    if args.step:
        {"time": step_time, "evals": step_evals}[args.step](args.config, args.calls)
        return 0
    cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", "time",
           "--config", args.config, "--calls", str(args.calls)]
    done = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    sys.stdout.write(done.stdout)
    sys.stderr.write(done.stderr[-2000:])
    with open(args.out, "w") as f:
        f.write("# python tools/classify_rate.py --config %s --calls %d\n" % (args.config, args.calls))
        f.write(done.stdout)
        if done.returncode != 0:
            f.write("the step ended with status %d\n" % done.returncode)
    return done.returncode


if __name__ == "__main__":
    sys.exit(main())
