"""The case table of the topic-asymmetry tests (test infrastructure): tests/test_gpu_topic_asymmetry.py
runs these inputs through every document-kernel path, tests/test_asymmetric_inputs_host.py proves on
the oracle alone that they can fail a wrong kernel.  Both take every (K, V, lens, seed) from here.

Inputs: helpers.asymmetric_case -- peaked lambda and a per-topic alpha over three decades, so that a
kernel reading alpha (lda.cpp:194) or a topic factor at a wrong topic index computes another gamma
and, in the waves that only form the stop test's sum |gamma - last| (lda.cpp:202), stops a document
at another iteration.

Seeds, thresholds and swap pairs are chosen, not arbitrary.  Each case has the largest threshold of
1e-3, 1e-4, .. 1e-7 and then the first seed from 1 on for which the three conditions of
tests/test_asymmetric_inputs_host.py hold with no document excluded: a batch with a near tie at the
threshold, or none of whose documents runs to the iteration cap (few topics, or thousands of which
most stay at alpha: the MEAN change is small), was passed over.  Its swap pairs were found by trying,
per pattern (pair_patterns), the pairs in order of decreasing ratio of their alphas and keeping the
first that changes a document's iteration count.  Batches of one shape share their seed: lambda and
alpha are drawn first, so they are the same model."""
import math
from collections import namedtuple

import numpy as np

from helpers import asymmetric_case

MAX_ITER = 60
# no document's iteration count may change when the threshold moves by this much either way: 1e-6
# relative at the usual 1e-3, and the same ABSOLUTE band below it -- what another summation order
# does to sum |gamma - last| does not shrink with the threshold
TIE_BAND = 1e-9

Case = namedtuple("Case", "group K V lens seed zero_counts max_iter threshold pairs")

# every tier of the K <= 128 launch in one batch (tests/test_gpu_parity.py, test_document_length_boundaries)
TIERED_LENS = [1, 2, 63, 64, 65, 127, 128, 129, 137, 144, 145, 192, 193, 257, 400, 700, 1300]
# nothing beyond 128 words: estep_docs_reg_kernel; lengths around its waves' 16-word shares
REG128_LENS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 126, 127, 128, 128]
# the longest at 144: the variant with 18 words per wave
REG144_LENS = [0, 1, 17, 18, 19, 35, 36, 37, 126, 127, 128, 129, 130, 137, 144]
WIDE_LENS = [0, 1, 8, 9, 80, 81, 161, 257, 420, 700]
GENERAL_LENS = [1, 64, 130, 300]
# a wave per document, eight documents per workgroup (three workgroups), behind one document that
# keeps a workgroup of its own
SMALL_LENS = [200, 1, 2, 31, 33, 62, 63, 64, 65, 66, 100, 126, 127, 128, 128, 64, 5, 17, 96, 120]


def stream_lens(B, long_lens=()):
    """B document lengths in 1..128, the first ones replaced by `long_lens`"""
    lens = np.random.RandomState(B).randint(1, 129, size=B)
    lens[:len(long_lens)] = long_lens
    return [int(n) for n in lens]


# group -> V, lens (by K and batch number), zero counts, max_iter
def _shape(group, K, n):
    if group == "tiered":
        return 3000, TIERED_LENS, False, MAX_ITER
    if group == "reg128":
        return 600, REG128_LENS, False, MAX_ITER
    if group == "reg144":
        return 600, REG144_LENS, True, MAX_ITER
    if group == "wide":
        return 1500, WIDE_LENS, True, MAX_ITER
    if group == "general":
        return 700, GENERAL_LENS, True, MAX_ITER
    if group == "small":
        # (two topics settle by a decade every iteration or two: no document of forty seeds was still
        # moving after 40 iterations at any threshold the tie band allows, so the cap that binds is 10)
        return 600, SMALL_LENS, False, MAX_ITER if K > 2 else 10
    # streams: two batches per shape, the second with the 144-word variant, the LDS tail and split
    # documents in its launch; update loops (max_iter_inference = 20): merged launches at K = 64, the
    # big-table path at K = 333
    V, B = {64: (900, 90), 128: (3000, 64), 333: (13000, 40)}[K]
    lens = stream_lens(B - 7, (129, 140, 150, 200, 400)) if n else stream_lens(B)
    return V, lens, False, MAX_ITER if group == "stream" else 20


# (group, K, batch number, seed, threshold, swap pairs)
_CHOSEN = [
    ("tiered", 7, 0, 12, 1e-6, ((0, 1),)),
    ("tiered", 100, 0, 1, 1e-3, ((76, 77), (32, 96))),
    ("tiered", 128, 0, 1, 1e-3, ((16, 17), (17, 81))),
    ("reg128", 7, 0, 35, 1e-5, ((2, 3),)),
    ("reg128", 100, 0, 1, 1e-3, ((58, 59), (17, 81))),
    ("reg128", 128, 0, 1, 1e-3, ((17, 18), (40, 104))),
    ("reg144", 7, 0, 28, 1e-7, ((3, 4),)),
    ("reg144", 100, 0, 1, 1e-3, ((58, 59), (17, 81))),
    ("reg144", 128, 0, 1, 1e-3, ((17, 18), (40, 104))),
    ("wide", 64, 0, 1, 1e-3, ((26, 27),)),
    ("wide", 65, 0, 2, 1e-3, ((41, 42), (0, 64))),
    ("wide", 128, 0, 1, 1e-3, ((96, 97), (12, 76))),
    ("wide", 129, 0, 1, 1e-3, ((27, 28), (13, 77), (68, 128))),
    ("wide", 192, 0, 1, 1e-3, ((86, 87), (27, 91), (87, 156))),
    ("wide", 256, 0, 1, 1e-3, ((117, 118), (101, 165), (170, 224))),
    ("wide", 257, 0, 1, 1e-3, ((107, 108), (67, 131))),
    ("wide", 320, 0, 1, 1e-3, ((10, 11), (115, 179))),
    ("wide", 448, 0, 1, 1e-3, ((77, 78), (40, 104))),
    ("wide", 512, 0, 1, 1e-3, ((109, 110), (31, 95))),
    ("general", 513, 0, 6, 1e-3, ((218, 219), (58, 122))),
    ("general", 1000, 0, 10, 1e-4, ((164, 165), (138, 202))),
    ("general", 2276, 0, 12, 1e-7, ((2010, 2011), (553, 617))),
    ("small", 2, 0, 1, 1e-3, ((0, 1),)),
    ("small", 10, 0, 2, 1e-3, ((2, 3),)),
    ("small", 31, 0, 1, 1e-3, ((3, 4),)),
    ("small", 32, 0, 1, 1e-3, ((15, 16),)),
    ("stream", 64, 0, 1, 1e-3, ((43, 44),)),
    ("stream", 64, 1, 1, 1e-3, ((43, 44),)),
    ("stream", 128, 0, 1, 1e-3, ((16, 17), (17, 81))),
    ("stream", 128, 1, 1, 1e-3, ((16, 17), (17, 81))),
    ("update", 64, 0, 1, 1e-3, ((43, 44),)),
    ("update", 333, 0, 1, 1e-3, ((3, 4), (85, 149))),
]


def make_case(group, K, n, seed, threshold, pairs):
    V, lens, zero, max_iter = _shape(group, K, n)
    return Case(group, K, V, tuple(lens), seed, zero, max_iter, threshold, tuple(pairs))


CASES = [make_case(*row) for row in _CHOSEN]


def cases(group):
    return [c for c in CASES if c.group == group]


def case_id(c):
    return "%s-K%d-B%d" % (c.group, c.K, len(c.lens))


def build(c):
    return asymmetric_case(c.K, c.V, c.lens, c.seed, zero_counts=c.zero_counts)


def pair_patterns(K):
    """Pairs of topics whose alpha a wrongly indexed kernel would confuse: k and k + 1 (neighbours in a
    wave, in an LDS row), k and k + 64 (the same lane of the next wave / the next topic slot) and,
    for 128 < K <= 256, pairs astride the first topic of the last 64-topic slot, where the mirror
    waves of the single-orientation kernel begin."""
    out = [[(k, k + 1) for k in range(K - 1)]]
    if K > 64:
        out.append([(k, k + 64) for k in range(K - 64)])
    if 128 < K <= 256:
        b = 64 * int(math.ceil(K / 64.)) - 64
        out.append([(i, j) for i in range(b - 64, b) for j in range(b, K)])
    return out


def warm_start(oracle, c, nthreads=8):
    """the case's inputs with gamma0 replaced by the gamma its E-step ends with -- how the E-steps of an
    update loop with init_gamma=False start.  Documents that had converged now stop after ONE
    iteration, and only if the first iteration's sum |gamma - gamma0| is right: the mirror waves of
    csrc/estep_wide.h carry their own last gamma from then on, so a wrong alpha there cancels in
    every later difference and shows in the first alone."""
    lam, alpha, ip, ids, cnts, g0 = build(c)
    g = oracle.estep(lam, alpha, ip, ids, cnts, g0, c.max_iter, c.threshold, nthreads=nthreads)[0]
    return lam, alpha, ip, ids, cnts, np.asfortranarray(g)


def host_conditions(oracle, c, nthreads=8, warm=False):
    """What makes the case able to fail a wrong kernel, measured on the oracle alone:
    `iters`, and the iteration counts at threshold -+ TIE_BAND; per swap pair the largest relative
    move of a gamma entry and the number of documents whose iteration count changes."""
    lam, alpha, ip, ids, cnts, g0 = warm_start(oracle, c, nthreads) if warm else build(c)

    def run(a, thr=c.threshold):
        return oracle.estep(lam, a, ip, ids, cnts, g0, c.max_iter, thr, nthreads=nthreads)

    g, _, it = run(alpha)
    lo = run(alpha, c.threshold - TIE_BAND)[2]
    hi = run(alpha, c.threshold + TIE_BAND)[2]
    swaps = []
    for i, j in c.pairs:
        a2 = alpha.copy()
        a2[i], a2[j] = alpha[j], alpha[i]
        g2, _, it2 = run(a2)
        swaps.append(((i, j), float(np.max(np.abs(g2 - g) / np.abs(g))), int((it2 != it).sum())))
    return dict(iters=it, iters_lo=lo, iters_hi=hi, swaps=swaps)


def stop_test_is_live(r, max_iter):
    it = r["iters"]
    return bool(np.array_equal(r["iters_lo"], it) and np.array_equal(r["iters_hi"], it) and
                len(set(it.tolist())) >= 3 and (it < max_iter).any() and (it == max_iter).any())
