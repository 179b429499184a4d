"""Throughput of LDA.sample (csrc/sample_kernels.h): tokens per second of whole calls and the time of
each phase -- the beta table, theta, the tokens, the download of the word ids -- in-process, after a
warm-up call.

The phases come from differences of synchronising calls of trlda_model_sample on device buffers:
B = 0 builds the table only; length 0 adds theta (every document empty); the full call adds the
tokens.  The download is one trlda_dev_download of the ids.  Each time is the median over --calls
calls of a host clock around the call, which ends in a device synchronise.

    python tools/sample_rate.py [--configs k100,k500] [--calls N]

Run on the GPU box from the repo root; one JSON line per configuration.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (K, V, B, length)
    "k100": (100, 7000, 100000, 100),           # 10^7 tokens
    "k500": (500, 100000, 10000, 200),          # 2 x 10^6 tokens over a 400 MB table
}


def _median_ms(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    from trlda_amd import _ffi
    from trlda_amd.models import OnlineLDA
    _ffi.require_gpu()
    L = _ffi.lib()
    for name in args.configs.split(","):
        K, V, B, length = CONFIGS[name]
        rng = np.random.RandomState(1)
        m = OnlineLDA(num_words=V, num_topics=K, num_documents=B, alpha=.1, eta=.01, device=0)
        m.lambdas = rng.gamma(1.0, 1.0, size=(K, V)) + 0.01
        key = 0x5EED5EED12345
        t0 = time.perf_counter()
        indptr = np.empty(B + 1, dtype=np.int32)
        _ffi.check(L.trlda_sample_lengths(B, float(length), key, indptr))
        lengths_ms = (time.perf_counter() - t0) * 1e3
        empty = np.zeros(B + 1, dtype=np.int32)
        nnz = int(indptr[-1])
        bufs = [_ffi.vp() for _ in range(4)]
        for p, nbytes in zip(bufs, ((B + 1) * 4, (B + 1) * 4, max(nnz, 1) * 4, K * B * 8)):
            _ffi.check(L.trlda_dev_alloc(0, nbytes, C.byref(p)))
        d_indptr, d_empty, d_ids, d_theta = bufs
        _ffi.check(L.trlda_dev_upload(0, d_indptr, indptr.ctypes.data, indptr.nbytes))
        _ffi.check(L.trlda_dev_upload(0, d_empty, empty.ctypes.data, empty.nbytes))
        ids = np.empty(max(nnz, 1), dtype=np.int32)

        def table():
            _ffi.check(L.trlda_model_sample(m._handle, 0, None, None, None, key))

        def theta():
            _ffi.check(L.trlda_model_sample(m._handle, B, d_empty, d_ids, d_theta, key))

        def full():
            _ffi.check(L.trlda_model_sample(m._handle, B, d_indptr, d_ids, d_theta, key))

        def download():
            _ffi.check(L.trlda_dev_download(0, ids.ctypes.data, d_ids, nnz * 4))

        full()                                                    # warm-up: allocations, code objects
        download()
        t_table = _median_ms(table, args.calls)
        t_theta = _median_ms(theta, args.calls)
        t_full = _median_ms(full, args.calls)
        t_down = _median_ms(download, args.calls)
        host_call = np.empty(nnz, dtype=np.int32)
        t0 = time.perf_counter()
        _ffi.check(L.trlda_model_sample_host(m._handle, B, indptr, host_call, None, key))
        host_ms = (time.perf_counter() - t0) * 1e3
        _ffi.check(L.trlda_dev_synchronize(0))
        for p in bufs:
            L.trlda_dev_free(0, p)
        m.close()
        print(json.dumps({
            "config": name, "K": K, "V": V, "B": B, "length": length, "tokens": nnz,
            "lengths_host_ms": round(lengths_ms, 3),
            "beta_table_ms": round(t_table, 3),
            "theta_ms": round(t_theta - t_table, 3),
            "tokens_ms": round(t_full - t_theta, 3),
            "download_ms": round(t_down, 3),
            "device_call_ms": round(t_full, 3),
            "host_call_ms": round(host_ms, 3),
            "tokens_per_s_device_call": round(nnz / (t_full * 1e-3), 1),
            "tokens_per_s_host_call": round(nnz / ((host_ms + lengths_ms) * 1e-3), 1),
        }), flush=True)


if __name__ == "__main__":
    main()
