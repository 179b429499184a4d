#!/usr/bin/env python3
"""Generate tests/golden/f15_users.npz from the REFERENCE's own user loader.

    python tests/golden/make_users_golden.py          # needs the reference's sources

The reference's ``load_users`` / ``load_users_as_dict`` (code/trlda/python/utils/load_users.py)
are plain Python; the module is loaded from where it lies, run on a ratings file this script
writes, and only its outputs are stored: per case the number of users of each batch, each user's
number of pairs, the flattened (item, rating) pairs and, for the dict form, the uids in the
batches' key order -- plus the ratings file itself, this script's own data.  Cases: the whole
file, fixed batch sizes, stochastic sizes under fixed NumPy seeds (rates small enough to draw
zeros), thresholds 0, 3 and 4; the file has a user whose ratings are all below 4 and a uid that
comes back after other users.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/code/trlda/python/utils/load_users.py"

# name, batch_size, stochastic, threshold, numpy seed
CASES = [("all_t4", None, False, 4, 0), ("all_t3", None, False, 3, 0), ("all_t0", None, False, 0, 0),
         ("b3_t4", 3, False, 4, 0), ("b4_t0", 4, False, 0, 0), ("b50_t3", 50, False, 3, 0),
         ("s2_t4_seed1", 2, True, 4, 1), ("s1_t0_seed2", 1, True, 0, 2), ("s1_t3_seed5", 1, True, 3, 5),
         ("s3_t0_seed7", 3, True, 0, 7)]


def ratings_text(rng):
    lines = []
    uids = [int(u) for u in rng.integers(1, 10 ** 7, size=20)]
    uids[7] = uids[2]                       # the same uid again, after other users
    for j, uid in enumerate(uids):
        n = int(rng.integers(1, 7))
        for _ in range(n):
            rating = 1 + int(rng.integers(0, 3)) if j == 11 else 1 + int(rng.integers(0, 5))
            lines.append("%d %d %d" % (uid, int(rng.integers(1, 500)), rating))
    return "\n".join(lines) + "\n"


def flatten(batches, as_dict):
    sizes = [len(b) for b in batches]
    users = [u for b in batches for u in (b.values() if isinstance(b, dict) else b)]
    keys = [k for b in batches if isinstance(b, dict) for k in b.keys()] if as_dict else []
    lens = [len(u) for u in users]
    pairs = np.array([t for u in users for t in u], dtype=np.int64).reshape(-1, 2)
    return (np.array(sizes, dtype=np.int64), np.array(lens, dtype=np.int64), pairs[:, 0].copy(),
            pairs[:, 1].copy(), np.array(keys, dtype=np.int64))


def main():
    if not os.path.exists(REF):
        sys.exit("reference not present: nothing generated")
    spec = importlib.util.spec_from_file_location("ref_load_users", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    text = ratings_text(np.random.Generator(np.random.PCG64(15)))
    path = os.path.join(HERE, "_users_ratings.tmp")
    with open(path, "w") as f:
        f.write(text)
    out = {"text": np.frombuffer(text.encode(), dtype=np.uint8)}
    try:
        for name, bs, st, th, seed in CASES:
            for form, fn in (("list", mod.load_users), ("dict", mod.load_users_as_dict)):
                np.random.seed(seed)
                res = fn(path, batch_size=bs, stochastic=st, threshold=th)
                batches = list(res) if bs else [res]
                for key, arr in zip(("sizes", "lens", "items", "ratings", "uids"),
                                    flatten(batches, form == "dict")):
                    out["%s_%s_%s" % (name, form, key)] = arr
    finally:
        os.remove(path)
    dst = os.path.join(HERE, "f15_users.npz")
    np.savez_compressed(dst, **out)
    print("f15_users.npz %d arrays, %.1f kB" % (len(out), os.path.getsize(dst) / 1e3))


if __name__ == "__main__":
    main()
