"""Device time per call of trlda.utils' GPU paths: sample_dirichlet (csrc/dirichlet_kernels.h) in both
regimes, and polygamma (csrc/polygamma.h) on a device tensor and on an ndarray staged through a device
buffer.

The calls run in a child process under `rocprofv3 --kernel-trace --memory-copy-trace --stats`; the
traces are read back, the first call (allocations, code objects) is left out, and the rest are
averaged per kernel and for the host<->device copies.  The host's wall time per call is reported
beside them.

    python tools/utils_rate.py [--configs dir100,dir1e5,pg_tensor,pg_ndarray] [--calls N] [--out DIR]

Run from the repo root on a machine with the GPU; one JSON line per configuration.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    # name: what one call does
    "dir100": "sample_dirichlet(100, 10**6, .1)",
    "dir1e5": "sample_dirichlet(10**5, 100, .1)",
    "pg_tensor": "polygamma(1, x), x a 10**7-element float64 tensor on the GPU",
    "pg_ndarray": "polygamma(1, x), x a 10**7-element ndarray",
}
COUNT = 10 ** 7


def child(name, calls):
    import trlda
    from trlda_amd import _ffi
    from trlda.utils import polygamma, sample_dirichlet
    _ffi.require_gpu()
    trlda.seed(5)
    if name.startswith("dir"):
        m, n = (100, 10 ** 6) if name == "dir100" else (10 ** 5, 100)
        call = lambda: sample_dirichlet(m, n, .1)                     # noqa: E731
    elif name == "pg_ndarray":
        x = np.random.RandomState(1).uniform(0.01, 30.01, COUNT)
        call = lambda: polygamma(1, x)                                # noqa: E731
    else:
        import torch
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand(COUNT, device="cuda", dtype=torch.float64, generator=g) * 30.0 + 0.01

        def call():
            polygamma(1, x)
            torch.cuda.synchronize()
    ms = []
    for _ in range(calls + 1):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"host_call_ms": float(np.median(ms[1:]))}), flush=True)


def _rows(out_dir, kind, name_field):
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*%s.csv" % kind), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get(name_field, kind)))
    rows.sort()
    return rows


def per_call_us(rows, calls, keep=lambda k: True):
    """{name: mean us per call}, the first call's share of each name left out"""
    by = {}
    for s, e, k in rows:
        if keep(k):
            by.setdefault(k, []).append(e - s)
    out = {}
    for k, v in by.items():
        per = len(v) // (calls + 1)
        if per:
            out[k] = float(np.sum(v[per:])) / calls / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.calls)
    if args.out is None:
        args.out = tempfile.mkdtemp(prefix="utils_rate_")
    for name in args.configs.split(","):
        out_dir = os.path.join(args.out, name)
        cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv",
               "-d", out_dir, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", name,
               "--calls", str(args.calls)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-3000:] + p.stderr[-3000:])
            raise SystemExit(p.returncode)
        info = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        mine = lambda k: "dirichlet_" in k or "polygamma_kernel" in k          # noqa: E731
        kernels = per_call_us(_rows(out_dir, "kernel_trace", "Kernel_Name"), args.calls, mine)
        copies = per_call_us(_rows(out_dir, "memory_copy_trace", "Direction"), args.calls)
        if name == "pg_tensor":
            copies = {}                      # (the tensor's own set-up copies are not the call's)
        kernel_us = sum(kernels.values())
        copy_us = sum(copies.values())
        print(json.dumps({
            "config": name, "call": CONFIGS[name], "calls_timed": args.calls, **info,
            "kernel_us": round(kernel_us, 2), "copy_us": round(copy_us, 2),
            "device_call_us": round(kernel_us + copy_us, 2),
            "kernels_us": {k.split("(")[0][:60]: round(v, 2) for k, v in kernels.items()},
            "copies_us": {k: round(v, 2) for k, v in copies.items()},
        }), flush=True)


if __name__ == "__main__":
    main()
