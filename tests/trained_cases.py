"""The case table of the trained-model tests (test infrastructure): tests/test_gpu_trained_inputs.py
runs these inputs through the sampling and scoring entry points, tests/test_trained_inputs_host.py
proves on the restatements alone that they can fail a wrong kernel.  Both take every (K, V, eta, seed,
key, swap pair) from here; tests/golden/make_trained_table_golden.py takes the Gibbs cases' lambda.

Inputs: trained_case -- what a model this library trains looks like.  lambda = eta + S with S sparse
non-negative integer counts: every topic owns a few words (counts over 1 .. 1e4), about V / 20 stop
words (at most 20) carry 1e3 .. 1e5 in every topic, the last two words are unseen (eta in every topic), every row
sum lies in [1e4, 1e6].  With those row sums the table the samplers read,
e = exp(psi(lambda) - psi(rowsum)), is at the entries that hold eta

    eta = 0.3      ~ 1e-6    the control
    eta = 0.01     ~ 1e-49   normal, tiny
    eta = 1.4e-3   ~ 1e-316  subnormal (psi(1.4e-3) = -714.86; psi(rowsum) in [9.2, 13.8])
    eta = 1e-3     0         exactly (psi(1e-3) = -1000.6: below exp_nonpos's clamp at -800, and the true
                             value, below 1e-439, rounds to 0 as well)

alpha is log-spaced over [2e-3, 4] in a random topic order (helpers.asymmetric_case's), so that a
kernel reading alpha at a wrong topic index computes other numbers.

Seeds, keys and swap pairs are chosen, not arbitrary (find_pairs and find_fallback_key are how):
  - a swap pair is the first of its pattern (pair_patterns), in order of decreasing ratio of the two
    alphas, whose swap changes the restatement's result;
  - the 'last topic with p > 0' fall-back of the histogram draw needs r = u * total to round up to
    total: u >= 1 - 2^-53 for a total with 53 bits, but u >= 1 - 1 / (2 T) for a subnormal total of T
    units of 2^-1074.  The document made of one token of an unseen word at eta = 1.4e-3, K = 3 has
    T ~ 2e8 (all three weights subnormal); FALLBACK_KEY is the first key of find_fallback_key's search
    under which one of its sweeps draws such a u, with a factor 4 to spare so that a table that
    differs in its last unit reaches the branch too.
"""
from collections import namedtuple

import numpy as np

ETAS = (0.3, 0.01, 1.4e-3, 1e-3)
REGIME = {0.3: "control", 0.01: "tiny", 1.4e-3: "subnormal", 1e-3: "zero"}
V = 120
WAVE = 64


def trained_case(K, V, eta, seed):
    """-> lambda (K x V, F-order), alpha (K), docs, docs_unseen.  `docs`: six documents as lists of
    (word, count) whose words some topic owns -- a short one, an empty one, one with a duplicate id and
    a zero count, one of about 300 tokens, one of stop words only, one of a single token.
    `docs_unseen`: the same, but the first also holds an unseen word and the last is one token of the
    other unseen word.  The same (K, V, seed) give the same S, alpha and documents for every eta."""
    K, V = int(K), int(V)
    rng = np.random.RandomState(int(seed))
    S = np.zeros((K, V))
    seen = V - 2
    stop = np.sort(rng.choice(seen, min(max(1, V // 20), 20), replace=False))   # (20 at most: the row sums)
    S[:, stop] = np.rint(10. ** rng.uniform(3., 5., (K, len(stop))))
    S[:, stop[0]] = np.rint(10. ** rng.uniform(4., 5., K))                 # every row sum >= 1e4
    rest = np.setdiff1d(np.arange(seen), stop)
    for k in range(K):
        own = rng.choice(rest, 3 + rng.randint(4), replace=False)
        S[k, own] = np.rint(10. ** rng.uniform(0., 4., len(own)))
    lam = np.asfortranarray(eta + S)
    rs = lam.sum(axis=1)
    assert rs.min() >= 1e4 and rs.max() <= 1e6 and not S[:, seen:].any()
    alpha = np.logspace(np.log10(2e-3), np.log10(4.), K)[rng.permutation(K)]
    owned = np.nonzero((S > 0).any(axis=0))[0]
    plain = np.setdiff1d(owned, stop)

    def entries(words, lo, hi):
        return [(int(w), int(c)) for w, c in zip(words, rng.randint(lo, hi, len(words)))]

    dup = entries(rng.choice(plain, 4, replace=False), 1, 4)
    docs = [entries(rng.choice(owned, 5, replace=False), 1, 4),
            [],
            [dup[0], (dup[0][0], 1), (dup[1][0], 0), dup[2], dup[3]],
            entries(rng.choice(owned, 100), 1, 6),                          # 100 entries, ~300 tokens
            entries(stop[:3], 1, 3),
            [(int(rng.choice(plain)), 1)]]
    unseen = [list(d) for d in docs]
    unseen[0] = unseen[0] + [(V - 1, 2)]
    unseen[5] = [(V - 2, 1)]
    return lam, alpha, docs, unseen


def csr(docs):
    indptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int32)
    ids = np.array([w for d in docs for w, _ in d], dtype=np.int32)
    cnts = np.array([c for d in docs for _, c in d], dtype=np.int32)
    return indptr, ids, cnts


def words_of(docs):
    return sorted({w for d in docs for w, _ in d})


def host_table(lam, psi=None):
    """e = exp(psi(lambda) - psi(rowsum(lambda))), K x V, with scipy's digamma (or `psi`)."""
    if psi is None:
        from scipy.special import digamma as psi
    else:
        psi = np.vectorize(psi, otypes=[np.float64])
    lam = np.asarray(lam, dtype=np.float64)
    with np.errstate(under="ignore"):
        return np.asfortranarray(np.exp(psi(lam) - psi(lam.sum(axis=1))[:, None]))


def theta0(K, B, seed):
    return np.asfortranarray(np.random.RandomState(1000 + int(seed)).dirichlet(np.ones(int(K)), size=int(B)).T)


def swapped(alpha, pair):
    a = np.array(alpha, copy=True)
    i, j = pair
    a[i], a[j] = alpha[j], alpha[i]
    return a


def kpl_of(K):
    kpl = 1
    while kpl * WAVE < K:
        kpl *= 2
    return kpl


def pair_patterns(entry, K):
    """Pairs of topics whose alpha a wrongly indexed kernel would confuse.  The Gibbs family (gibbs,
    cvb0, l2r) holds topics l KPL .. l KPL + KPL - 1 in lane l: k and k + 1 inside a lane, k and
    k + KPL in neighbouring lanes (KPL = 1: the same pairs, one pattern).  The others hold topic k in
    lane k mod 64: k and k + 1, k and k + 64."""
    if entry in ("gibbs", "cvb0", "l2r"):
        kpl = kpl_of(K)
        if kpl == 1:
            return [[(k, k + 1) for k in range(K - 1)]]
        return [[(k, k + 1) for k in range(K - 1) if k // kpl == (k + 1) // kpl],
                [(k, k + kpl) for k in range(K - kpl)]]
    out = [[(k, k + 1) for k in range(K - 1)]]
    if K > 64:
        out.append([(k, k + 64) for k in range(K - 64)])
    return out


def find_pairs(entry, K, alpha, differs, tries=8):
    """Per pattern the first pair, in order of decreasing ratio of its alphas, for which
    differs(swapped alpha) holds (at most `tries` pairs are tried; None if none does)."""
    out = []
    for pattern in pair_patterns(entry, K):
        ranked = sorted(pattern, key=lambda p: -abs(np.log(alpha[p[0]] / alpha[p[1]])))
        out.append(next((p for p in ranked[:tries] if differs(swapped(alpha, p))), None))
    return tuple(out)


# --------------------------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------------------------
# entry point -> its K values: the Gibbs family at KPL 1, 2, 4, 16; elsewhere the K at which the entry
# point's own GPU test file switches variant (at most four)
KS = {
    "gibbs": (3, 65, 200, 1000),
    "cvb0": (3, 65, 130, 1024),
    "l2r": (3, 65, 100, 1024),
    "marginal": (3, 100, 600, 2304),
    "heldout": (7, 129, 600, 1000),
    "wordtopics": (3, 65, 513, 2276),
    "sample": (3, 100, 1500),
}
SEED = 1                       # one model per K: the same S, alpha and documents for every eta
NS, BI = 1, 2                  # the chains' num_samples, burn_in
CVB0_ITER, CVB0_THRESHOLD = 7, 0.0
L2R_PARTICLES, L2R_LONG = 2, 131
MARGINAL_SAMPLES = 8
FALLBACK_K, FALLBACK_ETA = 3, 1.4e-3
FALLBACK_NS, FALLBACK_BI = 3, 7

Case = namedtuple("Case", "entry K V eta seed pairs")

# (entry, K) -> swap pairs, one per pattern: the first that changes the result at every eta
# (find_pairs; tests/test_trained_inputs_host.py verifies each)
_PAIRS = {
    ("cvb0", 3): ((1, 2),),
    ("cvb0", 65): ((12, 13), (35, 37)),
    ("cvb0", 130): ((13, 14), (125, 129)),
    ("cvb0", 1024): ((221, 222), (23, 39)),
    ("gibbs", 3): ((1, 2),),
    ("gibbs", 65): ((12, 13), (35, 37)),
    ("gibbs", 200): ((196, 197), (172, 176)),
    ("gibbs", 1000): ((660, 661), (12, 28)),
    ("heldout", 7): ((4, 5),),
    ("heldout", 129): ((126, 127), (6, 70)),
    ("heldout", 600): ((213, 214), (283, 347)),
    ("heldout", 1000): ((111, 112), (123, 187)),
    ("l2r", 3): ((1, 2),),
    ("l2r", 65): ((12, 13), (35, 37)),
    ("l2r", 100): ((34, 35), (35, 37)),
    ("l2r", 1024): ((221, 222), (23, 39)),
    ("marginal", 3): ((1, 2),),
    ("marginal", 100): ((19, 20), (7, 71)),
    ("marginal", 600): ((213, 214), (283, 347)),
    ("marginal", 2304): ((1057, 1058), (2037, 2101)),
    ("wordtopics", 3): ((1, 2),),
    ("wordtopics", 65): ((49, 50), (0, 64)),
    ("wordtopics", 513): ((403, 404), (5, 69)),
    ("wordtopics", 2276): ((567, 568), (503, 567)),
}
FALLBACK_KEY = 0x1560A454        # find_fallback_key: the first from 1 on; T = 1.96e8 units


def key_of(c):
    """The key of a case's chain."""
    return 0x0123456789ABCDEF + 1000 * c.K + int(round(1e4 * c.eta))


def make_cases():
    return [Case(entry, K, V, eta, SEED, _PAIRS.get((entry, K), ()))
            for entry in ("gibbs", "cvb0", "l2r", "marginal", "heldout", "wordtopics", "sample")
            for K in KS[entry] for eta in ETAS]


CASES = make_cases()


def cases(entry):
    return [c for c in CASES if c.entry == entry]


def case_id(c):
    return "%s-K%d-%s" % (c.entry, c.K, REGIME[c.eta])


def build(c):
    return trained_case(c.K, c.V, c.eta, c.seed)


def table_cases():
    """The cases of the golden table: the Gibbs cases and K = 65 at V = 2000 (63 row-sum blocks where
    V = 120 has 4: the partial sums of exp_elog_beta_kernel in another shape)."""
    return cases("gibbs") + [Case("gibbs", 65, 2000, 0.01, SEED, ())]


def table_docs(c):
    """The batch of the table test: the short, the duplicate-id, the stop-word and the one-token
    document -- with the unseen words wherever the chain survives them (every eta but 1e-3)."""
    _, _, docs, unseen = build(c)
    src = docs if c.eta == 1e-3 else unseen
    return [src[0], docs[2], docs[4], src[5]]


def table_columns(c):
    """The golden table's columns: table_docs' words and the two unseen words, whatever eta."""
    _, _, docs, unseen = build(c)
    return words_of([unseen[0], docs[2], docs[4], unseen[5], docs[5]])


def l2r_docs(docs):
    """left_to_right redraws the whole prefix at every position: its long document is cut to
    L2R_LONG tokens (tests/test_gpu_l2r.py's length: three chunks of the lanes)."""
    out, left = [list(d) for d in docs], L2R_LONG
    long = []
    for w, c in out[3]:
        c = min(c, left)
        if c:
            long.append((w, c))
        left -= c
    out[3] = long
    return out


def find_fallback_key(lam, alpha, doc_index, sweeps, start=1, chunk=1 << 20, spare=4.):
    """The first key >= start under which a sweep of the one-token document `doc_index` draws
    u >= 1 - 1 / (2 spare T), T the document's histogram total in units of 2^-1074."""
    from gibbs_host import SWEEP
    e = host_table(lam)[:, lam.shape[1] - 2]
    T = float(np.sum(e * alpha)) / 2. ** -1074
    bound = 1. - 1. / (2. * spare * T)
    key = start
    while True:
        keys = np.arange(key, key + chunk, dtype=np.uint64)
        for s in range(sweeps):
            u = _philox_keys(0, doc_index, s, SWEEP, keys)
            hit = np.nonzero(u >= bound)[0]
            if hit.size:
                return int(keys[hit[0]]), T
        key += chunk


def _philox_keys(c0, c1, c2, c3, keys):
    """uniform() of the Philox block of one counter under many keys (keys < 2^32: k1 = 0)."""
    M0, M1, LO = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    c = [np.full(keys.shape, x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k0 = keys & LO
    k1 = keys >> np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & LO, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & LO]
        k0 = (k0 + np.uint64(0x9E3779B9)) & LO
        k1 = (k1 + np.uint64(0xBB67AE85)) & LO
    x = (c[1] << np.uint64(32)) | c[0]
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
