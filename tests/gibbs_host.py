"""NumPy restatement of the Gibbs sampler of csrc/gibbs_kernels.h (a helper module, not a test file).

It follows the header's contract step by step: Philox4x32-10 with the pinned counter layout, the
uniforms from its words, the init draws (one sequential sum over the topics per entry), the sweeps'
blocked per-lane prefix and 64-lane Hillis-Steele scan in the kernel's order of additions, and the
Marsaglia-Tsang gamma draws behind theta.  Given the same e table, alpha, documents, initial theta
and key it reproduces the kernel's topic counts and statistics exactly and theta to rounding.

Also: the exact posterior of one short document by enumeration of its topic assignments.
"""
import itertools
import math

import numpy as np

WAVE = 64
INIT_THETA, INIT_TOKEN, SWEEP, GAMMA_NORMAL, GAMMA_ACCEPT, GAMMA_BOOST = range(6)
GAMMA_TRIES = 64
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Random123's Philox4x32-10 on arrays of counter words; returns the four output words."""
    c = [np.asarray(x, dtype=np.uint64) & _LO for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _M0 * c[0]
        p1 = _M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _LO,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def uniform(lo, hi):
    """u = (x >> 11) 2^-53 in [0, 1), x = hi 2^32 + lo."""
    x = (np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def uniform_open(lo, hi):
    """u_open = ((x >> 12) + 0.5) 2^-52 in (0, 1)."""
    x = (np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)
    return ((x >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52


def split_key(key):
    return int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF


def wave_allsum(v):
    """The kernel's butterfly (xor 32, 16, .., 1) over 64 lane values; every lane's result."""
    v = np.array(v, dtype=np.float64)
    idx = np.arange(WAVE)
    off = 32
    while off:
        v = v + v[idx ^ off]
        off >>= 1
    return v[0]


def log_gamma(a, k, doc, key):
    """log of the Gamma(a) draws of topics k (arrays) of document `doc` (header: theta)."""
    k0, k1 = split_key(key)
    a = np.asarray(a, dtype=np.float64)
    k = np.asarray(k, dtype=np.uint64)
    out = np.full(a.shape, -np.inf)
    ok = (a > 0) & (a <= 1e300)
    boost = a < 1.0
    sh = np.where(boost, a + 1.0, a)
    d = sh - 1.0 / 3.0
    with np.errstate(divide="ignore", invalid="ignore"):
        c = 1.0 / np.sqrt(9.0 * d)
        lg = np.log(d)
        todo = ok.copy()
        for n in range(GAMMA_TRIES):
            if not todo.any():
                break
            w = philox4x32_10(k, doc, n, GAMMA_NORMAL, k0, k1)
            x = np.sqrt(-2.0 * np.log(uniform_open(w[0], w[1]))) * np.cos(6.283185307179586 * uniform(w[2], w[3]))
            v1 = 1.0 + c * x
            v = v1 * v1 * v1
            w = philox4x32_10(k, doc, n, GAMMA_ACCEPT, k0, k1)
            lu = np.log(uniform_open(w[0], w[1]))
            lv = np.log(v)
            acc = todo & (v1 > 0.0) & (lu < 0.5 * x * x + d - d * v + d * lv)
            lg = np.where(acc, np.log(d) + lv, lg)
            todo &= ~acc
        w = philox4x32_10(k, doc, 0, GAMMA_BOOST, k0, k1)
        lg = np.where(boost, lg + np.log(uniform_open(w[0], w[1])) / a, lg)
    return np.where(ok, lg, out)


def kpl_of(K):
    kpl = 1
    while kpl * WAVE < K:
        kpl *= 2
    return kpl


def _tally(stats, name):
    if stats is not None:
        stats[name] = stats.get(name, 0) + 1


def sweep_draw(e_pad, cnt_pad, u, kpl, stats=None):
    """One histogram draw in the kernel's order (e_pad, cnt_pad: 64 * kpl, topics >= K zero).
    Returns (topic, ok).  `stats` (a dict) counts the branches taken: 'draws', 'last_in_lane' and
    'last_overall' (the two fall-backs to the last topic with p > 0), 'zero_lane_below' (a lane
    whose weights are all 0 below the chosen lane) and 'zero_weight_pick' (the chosen topic's weight
    is not > 0: never, whatever the inputs)."""
    z, ok = _sweep_draw(e_pad, cnt_pad, u, kpl, stats)
    if ok and stats is not None:
        p = e_pad * cnt_pad
        _tally(stats, "draws")
        if not p[z] > 0.0:
            _tally(stats, "zero_weight_pick")
        live = (p.reshape(WAVE, kpl)[:z // kpl] > 0.0).any(axis=1)
        if live.any() and not live[int(np.argmax(live)):].all():
            _tally(stats, "zero_lane_below")               # between a live lane and the chosen one
    return z, ok


def _sweep_draw(e_pad, cnt_pad, u, kpl, stats):
    p = e_pad * cnt_pad
    q = np.cumsum(p.reshape(WAVE, kpl), axis=1)           # lane-local sequential prefix
    x = q[:, -1].copy()
    off = 1
    while off < WAVE:                                       # Hillis-Steele, offsets 1 .. 32
        y = np.empty_like(x)
        y[off:] = x[:-off]
        y[:off] = 0.0
        x = np.where(np.arange(WAVE) >= off, x + y, x)
        off <<= 1
    total = x[-1]
    if not (total > 0.0 and np.isfinite(total)):
        return -1, False
    r = u * total
    excl = np.concatenate(([0.0], x[:-1]))
    pr = p.reshape(WAVE, kpl)
    hit = np.nonzero(x > r)[0]
    if hit.size:
        L = int(hit[0])
        inl = np.nonzero(excl[L] + q[L] > r)[0]
        if inl.size:
            return L * kpl + int(inl[0]), True
        nz = np.nonzero(pr[L] > 0.0)[0]
        if nz.size:
            _tally(stats, "last_in_lane")
            return L * kpl + int(nz[-1]), True
    nz = np.nonzero(p > 0.0)[0]
    _tally(stats, "last_overall")
    return int(nz[-1]), True


def gibbs(e, alpha, indptr, ids, cnts, theta0, num_samples, burn_in, key, docs=None, stats=None):
    """The whole call: returns (theta K x B, counts K x V int64 summed over the samples,
    final topic counts K x B int64).  `docs`: only these documents (others left zero).  `stats`: a
    dict that counts the branches of the sweeps' draws (sweep_draw)."""
    e = np.asarray(e, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    K, V = e.shape
    B = len(indptr) - 1
    k0, k1 = split_key(key)
    kpl = kpl_of(K)
    theta = np.zeros((K, B))
    counts = np.zeros((K, V), dtype=np.int64)
    nfinal = np.zeros((K, B), dtype=np.int64)
    for d in (range(B) if docs is None else docs):
        if theta0 is not None:
            th = np.asarray(theta0, dtype=np.float64)[:, d].copy()
        else:
            w = philox4x32_10(np.arange(K), d, 0, INIT_THETA, k0, k1)
            x = -np.log(uniform_open(w[0], w[1]))
            part = np.zeros(WAVE)
            for k in range(K):
                part[k % WAVE] += x[k]
            th = x / wave_allsum(part)
        ents = [(int(ids[j]), max(int(cnts[j]), 0)) for j in range(indptr[d], indptr[d + 1])]
        z, words = [], []
        hist = np.zeros(K, dtype=np.int64)
        t = 0
        for wid, c in ents:
            if c == 0:
                continue
            p = e[:, wid] * th
            P = np.cumsum(p)
            tot = P[-1]
            ok = tot > 0.0 and np.isfinite(tot)
            if not ok:
                raise RuntimeError("Something went wrong while sampling from histogram.")
            w = philox4x32_10(np.arange(t, t + c), d, 0, INIT_TOKEN, k0, k1)
            r = uniform(w[0], w[1]) * tot
            nz = np.nonzero(p > 0.0)[0]
            last = int(nz[-1]) if nz.size else 0
            for i in range(c):
                above = np.nonzero(P > r[i])[0]
                zz = int(above[0]) if above.size else last
                z.append(zz)
                words.append(wid)
                hist[zz] += 1
            t += c
        cnt = np.zeros(WAVE * kpl)
        cnt[:K] = alpha + hist.astype(np.float64)
        ntok = len(z)
        for s in range(num_samples + burn_in):
            if ntok == 0:
                break
            w = philox4x32_10(np.arange(ntok), d, s, SWEEP, k0, k1)
            us = uniform(w[0], w[1])
            ti = 0
            for wid, c in ents:
                if c == 0:
                    continue
                e_pad = np.zeros(WAVE * kpl)
                e_pad[:K] = e[:, wid]
                for _ in range(c):
                    cnt[z[ti]] -= 1.0
                    zz, ok = sweep_draw(e_pad, cnt, us[ti], kpl, stats)
                    if not ok:
                        raise RuntimeError("Something went wrong while sampling from histogram.")
                    cnt[zz] += 1.0
                    z[ti] = zz
                    ti += 1
            if s >= burn_in:
                np.add.at(counts, (np.array(z), np.array(words)), 1)
        nfinal[:, d] = np.bincount(np.array(z, dtype=np.int64), minlength=K) if ntok else 0
        lg = log_gamma(cnt[:K], np.arange(K), d, key)
        lanes = np.full(WAVE * kpl, -np.inf)
        lanes[:K] = lg
        ex = np.exp(lanes - lanes.max())
        part = np.cumsum(ex.reshape(WAVE, kpl), axis=1)[:, -1]
        theta[:, d] = ex[:K] / wave_allsum(part)
    return theta, counts, nfinal


# ---- the exact posterior of one document ------------------------------------------------
def exact_posterior(e, alpha, words):
    """Enumerate the K^n topic assignments z of a document whose tokens have word ids `words`:
    p(z) ~ prod_i e[z_i, w_i] * prod_k Gamma(alpha_k + n_k) (the collapsed joint whose full
    conditionals are e[k, w] (alpha_k + n_k^-i)).  Returns (E[token counts per (topic, word)]
    K x V, E[theta] = E[(alpha + n) / (sum alpha + n)])."""
    e = np.asarray(e, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    K, V = e.shape
    n_tok = len(words)
    states = np.array(list(itertools.product(range(K), repeat=n_tok)), dtype=np.int64)
    logp = np.zeros(len(states))
    for i, w in enumerate(words):
        logp += np.log(e[states[:, i], w])
    n = np.stack([(states == k).sum(axis=1) for k in range(K)], axis=1)
    logp += np.array([sum(math.lgamma(alpha[k] + n[s, k]) for k in range(K)) for s in range(len(states))])
    p = np.exp(logp - logp.max())
    p /= p.sum()
    ecounts = np.zeros((K, V))
    for i, w in enumerate(words):
        for k in range(K):
            ecounts[k, w] += p[states[:, i] == k].sum()
    etheta = ((alpha[None, :] + n) / (alpha.sum() + n_tok) * p[:, None]).sum(axis=0)
    return ecounts, etheta


def sweep_stationary(e, alpha, words):
    """Brute force: the stationary distribution of one systematic-scan sweep of the collapsed
    sampler (the product of the per-token transition matrices over all K^n states), by power
    iteration.  Returns the probabilities in the order of itertools.product."""
    e = np.asarray(e, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    K = e.shape[0]
    n_tok = len(words)
    states = list(itertools.product(range(K), repeat=n_tok))
    index = {s: i for i, s in enumerate(states)}
    S = len(states)
    T = np.eye(S)
    for i, w in enumerate(words):
        Ti = np.zeros((S, S))
        for s in states:
            n = np.bincount(np.array(s), minlength=K).astype(np.float64)
            n[s[i]] -= 1.0
            cond = e[:, w] * (alpha + n)
            cond /= cond.sum()
            for k in range(K):
                t = list(s)
                t[i] = k
                Ti[index[s], index[tuple(t)]] += cond[k]
        T = T @ Ti
    pi = np.full(S, 1.0 / S)
    for _ in range(2000):
        pi = pi @ T
    return pi / pi.sum()
