"""Cost of DocumentIndex.group_prevalence and DocumentIndex.topic_effects (csrc/effects_kernels.h) next to
the same work written with torch on the same rows: ``Z.T @ (W theta)`` with ``Z.T @ (W Z)``, and
``torch.linalg.lstsq`` of ``sqrt(W) theta`` on ``sqrt(W) Z``.

    group_prevalence / topic_effects     whole calls (the design and the weights checked, padded and uploaded,
                                         every temporary allocated and freed, the kernels, the download of
                                         the small results, the host's closing arithmetic; each library call
                                         ends in a synchronise): host clock, median of --calls
    products / residuals                 the two library calls of topic_effects on their own, likewise
    torch                                the same work between two events on torch's stream, the design
                                         and theta already on the device

Both after a warm-up call.  Bytes and flops per call are computed from the shapes: the table is
N Kp 8 bytes (read once per pass of the groups, once per row of cross tiles by the products, once by each
residual pass), the design N Pp 8 bytes (uploaded by each library call); the products 2 N P' (P' + K)
flops as full products (of the Gram matrix the T (T + 1) / 2 tile pairs with pi <= pj are formed), a
residual pass 2 N Pp K.

    python tools/effects_rate.py [--configs k100,k500] [--calls N] [--out profiles/effects_rate.txt]

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
    # name: (K, N, P' with the intercept, groups)
    "k100": (100, 1000000, 16, 50),
    "k500": (500, 200000, 64, 50),
    "tiny": (20, 5000, 4, 5),            # rehearsal size
}
STEP_SECONDS = 280
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
    from trlda_amd import _ffi
    from trlda_amd.models import OnlineLDA
    K, N, P, G = CONFIGS[name]
    Kp, Pp = (K + 3) // 4 * 4, (P + 3) // 4 * 4
    model = OnlineLDA.__new__(OnlineLDA)
    model._num_documents, model._update_count = 1000, 0
    model._ada_tau, model._ada_rho, model._ada_sq_norm = 1000., 1e-3, 1.
    model._setup(8, K, .1, .3, 0, _lambda=np.ones((K, 8), order="F"))
    index = model.document_index()
    index.reserve(N)
    for at in range(0, N, ADD_CHUNK):
        index.add_gamma(_gammas(K, min(ADD_CHUNK, N - at), 100 + at))
    rng = np.random.RandomState(7)
    labels = rng.randint(-1, G, size=N).astype(np.int32)
    w = rng.uniform(0.5, 30.0, size=N)
    X = rng.normal(size=(N, P - 1))
    Z = np.ascontiguousarray(np.hstack([np.ones((N, 1)), X]))
    lib, handle = _ffi.lib(), index._handle
    gram, cross, rss = np.empty((P, P)), np.empty((P, K)), np.empty(K)

    def products():
        _ffi.check(lib.trlda_docindex_regress_products(handle, Z.ctypes.data, P, w.ctypes.data, gram.ctypes.data,
                                                       cross.ctypes.data))

    fit = index.topic_effects(X, weights=w)
    rows = np.ascontiguousarray(fit["coef"].T)

    def residuals():
        _ffi.check(lib.trlda_docindex_regress_residuals(handle, Z.ctypes.data, P, w.ctypes.data, rows.ctypes.data,
                                                        rss.ctypes.data))

    grp_med, grp_min = _host_median(lambda: index.group_prevalence(labels, weights=w, return_variance=True), calls)
    gru_med, gru_min = _host_median(lambda: index.group_prevalence(labels), calls)
    eff_med, eff_min = _host_median(lambda: index.topic_effects(X, weights=w), calls)
    pro_med, pro_min = _host_median(products, calls)
    res_med, res_min = _host_median(residuals, calls)
    mean, counts = index.group_prevalence(labels, weights=w)

    # the same work with torch on the device's own rows
    R = torch.empty((N, K), dtype=torch.float64, device="cuda")
    for at in range(0, N, ADD_CHUNK):
        n = min(ADD_CHUNK, N - at)
        R[at:at + n] = torch.from_numpy(index.rows(at, n)).cuda()
    Zd, wd = torch.from_numpy(Z).cuda(), torch.from_numpy(w).cuda()

    def torch_products():
        t = R * R
        wz = wd[:, None] * Zd
        return wz.T @ Zd, wz.T @ t

    def torch_lstsq():
        s = torch.sqrt(wd)[:, None]
        return torch.linalg.lstsq(s * Zd, s * (R * R)).solution

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

    tpro_med, tpro_min = device_median(torch_products)
    tls_med, tls_min = device_median(torch_lstsq)
    t_gram, t_cross = torch_products()
    t_coef = torch_lstsq().cpu().numpy()
    table_bytes, design_bytes = N * Kp * 8, N * Pp * 8
    product_flops, residual_flops = 2.0 * N * P * (P + K), 2.0 * N * Pp * K
    print(json.dumps({
        "config": name, "K": K, "N": N, "P": P, "groups": G, "calls": calls,
        "group_prevalence_weighted_variance_ms_median": round(grp_med * 1e3, 3),
        "group_prevalence_weighted_variance_ms_min": round(grp_min * 1e3, 3),
        "group_prevalence_ms_median": round(gru_med * 1e3, 3), "group_prevalence_ms_min": round(gru_min * 1e3, 3),
        "topic_effects_ms_median": round(eff_med * 1e3, 3), "topic_effects_ms_min": round(eff_min * 1e3, 3),
        "products_call_ms_median": round(pro_med * 1e3, 3), "products_call_ms_min": round(pro_min * 1e3, 3),
        "residuals_call_ms_median": round(res_med * 1e3, 3), "residuals_call_ms_min": round(res_min * 1e3, 3),
        "torch_products_ms_median": round(tpro_med * 1e3, 3), "torch_products_ms_min": round(tpro_min * 1e3, 3),
        "torch_lstsq_ms_median": round(tls_med * 1e3, 3), "torch_lstsq_ms_min": round(tls_min * 1e3, 3),
        "table_bytes": table_bytes, "design_bytes": design_bytes, "product_flops": product_flops,
        "residual_flops": residual_flops,
        "group_prevalence_table_GBps": round(table_bytes / gru_med / 1e9, 1),
        "products_call_TFLOPs": round(product_flops / pro_med / 1e12, 3),
        "torch_products_TFLOPs": round(product_flops / tpro_med / 1e12, 3),
        "group_members": int(counts.sum()),
        "max_abs_gram_difference": float(np.max(np.abs(t_gram.cpu().numpy() - gram))),
        "max_abs_cross_difference": float(np.max(np.abs(t_cross.cpu().numpy() - cross))),
        "max_abs_coef_difference": float(np.max(np.abs(t_coef - fit["coef"])))}), flush=True)
    model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="k100,k500")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "effects_rate.txt"))
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
        f.write("# python tools/effects_rate.py --configs %s --calls %d\n" % (args.configs, args.calls))
        f.writelines(lines)
    return done.returncode


if __name__ == "__main__":
    sys.exit(main())
