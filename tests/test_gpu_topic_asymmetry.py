"""Every document-kernel path with inputs that tell the topics apart: a per-topic alpha over three
decades (reference src/lda.cpp:194 adds alpha_k, a K-vector) and peaked, trained-looking topics
(helpers.asymmetric_case), where the shape tests use the scalar alpha = .1 and lambda = 1 +- 0.1.

With every alpha_k equal a kernel may read alpha, or a topic factor, at a wrong topic index and
nothing changes.  The sharpest case are the waves that recompute gamma only to form sum |gamma - last|
for the stop test (lda.cpp:202; csrc/estep_kernels.h waves 6 and 7, csrc/estep_wide.h mirror waves):
a wrong alpha there leaves every iteration's gamma right and only moves the iteration at which a
document stops -- so every case here compares the per-document iteration counts for equality, on
inputs that tests/test_asymmetric_inputs_host.py shows have no near tie at the threshold and do
change a count when two such alphas are swapped.  Cases: tests/asymmetric_cases.py.

Each case: gamma per document and the statistics against oracle.estep at TIGHT_RTOL (1e-8 for
atomically added statistics, as everywhere), identical iteration counts, and that the intended path
ran.

One case is held to another bar for its statistics, ORACLE_LIMITED below: there the fp64 oracle
itself is further than 1e-9 from the same fixed point in extended precision (estep_longdouble)."""
import numpy as np
import pytest

import asymmetric_cases as ac
from helpers import TIGHT_RTOL, relerr
from test_gpu_deferred import Slots
from test_gpu_lanes import ahead

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(hip_lib):
    from trlda_amd import _ffi
    assert _ffi.device_count() >= 1, "GPU tests need a visible MI355X"
    return hip_lib


@pytest.fixture(scope="module")
def expected(oracle):
    """(inputs, oracle results + the bar for the statistics) of a case at an iteration limit: computed
    once, read-only"""
    memo = {}

    def get(c, max_iter, warm=False):
        if warm:
            return get_warm(c)
        if (c, max_iter) not in memo:
            inp = ac.build(c)
            lam, alpha, ip, ids, cnts, g0 = inp
            want = oracle.estep(lam, alpha, ip, ids, cnts, g0, max_iter, c.threshold, nthreads=8)
            for x in inp + want:
                x.setflags(write=False)
            bar = TIGHT_RTOL
            if ac.case_id(c) in ORACLE_LIMITED and max_iter == c.max_iter:
                own = oracle_distance(inp, want, max_iter, c.threshold)[1]
                assert 10. * own > TIGHT_RTOL, own       # (else the case belongs with the others)
                bar = min(10. * own, 1e-8)
            memo[c, max_iter] = (inp, want + (bar,))
        return memo[c, max_iter]

    def get_warm(c):
        if (c, "warm") not in memo:
            inp = ac.warm_start(oracle, c)
            want = oracle.estep(*inp, c.max_iter, c.threshold, nthreads=8)
            for x in inp + want:
                x.setflags(write=False)
            memo[c, "warm"] = (inp, want + (TIGHT_RTOL,))
        return memo[c, "warm"]
    return get


LD = np.longdouble
PSI_SERIES = [LD(1) / 12, -LD(691) / 32760, LD(1) / 132, -LD(1) / 240, LD(1) / 252, -LD(1) / 120, LD(1) / 12]


def psi_longdouble(x):
    """digamma of positive arguments the way oracle/cpu_ref.c forms it (the recurrence up to 10, then
    the asymptotic series; digamma.cpp:158-171), in extended precision"""
    s, w = np.array(x, dtype=LD), np.zeros(np.shape(x), dtype=LD)
    for _ in range(10):
        low = s < 10
        w = w + np.where(low, 1 / np.where(low, s, 1), 0)
        s = s + low
    z = 1 / (s * s)
    p = PSI_SERIES[0]
    for coeff in PSI_SERIES[1:]:
        p = p * z + coeff
    return np.log(s) - LD(.5) / s - z * p - w


def estep_longdouble(lam, alpha, ip, ids, cnts, g0, max_iter, threshold):
    """LDA::updateVariablesVI (lda.cpp:160-220) restated in np.longdouble, on the CPU: what the fp64
    oracle's own rounding is measured against.  -> gamma, statistics, iteration counts"""
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is no wider than double here"
    lam, alpha = lam.astype(LD), alpha.astype(LD)
    K, V = lam.shape
    eeb = np.exp(psi_longdouble(lam) - psi_longdouble(lam.sum(axis=1))[:, None])
    gamma, sstats, iters = g0.astype(LD), np.zeros((K, V), dtype=LD), np.zeros(len(ip) - 1, np.int32)
    for d in range(len(ip) - 1):
        w, cnt = ids[ip[d]:ip[d + 1]], cnts[ip[d]:ip[d + 1]].astype(LD)
        beta, g = eeb[:, w], gamma[:, d]
        epg = np.exp(psi_longdouble(g))
        phinorm = epg @ beta + LD(1e-100)
        while iters[d] < max_iter:
            last = g
            g = alpha + epg * (beta @ (cnt / phinorm))
            epg = np.exp(psi_longdouble(g))
            phinorm = epg @ beta + LD(1e-100)
            iters[d] += 1
            if np.abs(last - g).sum() / K < threshold:
                break
        gamma[:, d] = g
        np.add.at(sstats, (slice(None), w), np.outer(epg, cnt / phinorm))
    return gamma, sstats * eeb, iters


def oracle_distance(inp, want, max_iter, threshold):
    """how far the fp64 oracle's gamma and statistics are from estep_longdouble's (relative, worst entry)"""
    gl, sl, itl = estep_longdouble(*inp, max_iter, threshold)
    go, so, ito = want
    assert np.array_equal(itl, ito)
    nz = so > 0
    return float(np.max(np.abs(go - gl) / gl)), float(np.max(np.abs(so[nz] - sl[nz]) / sl[nz]))


# Cases whose statistics the fp64 oracle itself does not have to 1e-9 at the full iteration limit.
# Measured on the MI355X, tiered-K128-B17 at max_iter 60: statistics 1.30e-9 .. 1.36e-9 from the oracle
# on EVERY path (tiered launch with and without split documents, both preambles, the general kernel),
# gamma 6.4e-11, iteration counts equal; and on the CPU the oracle is 1.22e-9 (gamma 5.8e-11) from
# estep_longdouble: documents that are still moving after 60 iterations carry every rounding
# difference along.  The device adds up in another order than the oracle, so the bar there is ten
# times the oracle's own distance, measured when the test runs -- and never above the 1e-8 of the
# atomic mode.  (Next in line, all inside 1e-9: stream-K128-B57 2.2e-10, stream-K64-B83 7.3e-11.)
ORACLE_LIMITED = {"tiered-K128-B17"}


def make_model(c, lam, alpha, D=10000):
    from trlda_amd.models import OnlineLDA
    m = OnlineLDA(num_words=c.V, num_topics=c.K, num_documents=D, alpha=alpha, eta=.3)
    m.lambdas = lam
    assert np.array_equal(m.alpha.ravel(), alpha)
    return m


def documents(inp):
    from trlda_amd.documents import CSRDocuments
    return CSRDocuments(inp[2], inp[3], inp[4])


def kernel(hip, m):
    return hip.trlda_model_last_doc_kernel(m._handle).decode()


def check(c, got, want, what, atomic=False):
    """gamma per document, statistics and iteration counts of one run against the oracle's: the
    figures are printed, what misses its bar is returned (a test runs all its variants, then asserts
    that nothing missed)"""
    (g, s, it), (go, so, ito, bar) = got, want
    per_doc = np.max(np.abs(g - go) / np.abs(go), axis=0) if g.size else np.zeros(1)
    nz = so > 0
    err_s = relerr(s[nz], so[nz])
    off = np.nonzero(np.asarray(it) != ito)[0]
    print("%s %s: gamma %.2e sstats %.2e" % (ac.case_id(c), what, per_doc.max(), err_s))
    missed = []
    if off.size:
        missed.append("%s: iteration counts of documents %s (%s words): %s, oracle %s" % (
            what, off.tolist(), [c.lens[d] for d in off], np.asarray(it)[off].tolist(), ito[off].tolist()))
    if not per_doc.max() < TIGHT_RTOL:
        missed.append("%s: gamma %.2e at the document of %d words" % (what, per_doc.max(),
                                                                     c.lens[int(np.argmax(per_doc))]))
    if not err_s < (1e-8 if atomic else bar):
        missed.append("%s: statistics %.2e (bar %.2e)" % (what, err_s, 1e-8 if atomic else bar))
    if not np.array_equal(s == 0, so == 0):
        missed.append("%s: zeros of the statistics" % what)
    for line in missed:
        print("MISSED " + ac.case_id(c) + " " + line)
    return missed


def iteration_limits(c):
    return (1, c.max_iter)


@pytest.mark.parametrize("c", ac.cases("tiered"), ids=ac.case_id)
def test_tiered_launch(hip, expected, c):
    """128 words in registers, the 144-word variant, the LDS tail up to 192, the single orientation
    beyond (LDS rows at 257 / 400, streamed rows at 700 / 1300) in ONE launch: split documents on and
    off, fused and two-kernel preamble, both statistics modes; then everything through the general
    kernel."""
    want_wgs = sum(-(-n // 128) - 1 for n in c.lens if 192 < n <= 2048)
    inp = ac.build(c)
    m = make_model(c, inp[0], inp[1])
    missed = []
    batch = m.upload(documents(inp))
    for max_iter in iteration_limits(c):
        inp, want = expected(c, max_iter)
        assert hip.trlda_model_set_doc_kernel(m._handle, 0) == 0
        for mode in (0, 1):
            for split_docs in (1, 0):
                for two_kernel in (0, 1):
                    hip.trlda_model_set_sstats_mode(m._handle, mode)
                    assert hip.trlda_model_set_split_docs(m._handle, split_docs) == 0
                    assert hip.trlda_model_set_split_preamble(m._handle, two_kernel) == 0
                    got = m.update_variables(batch, latents=inp[5], max_iter=max_iter, threshold=c.threshold,
                                             return_iterations=True)
                    assert kernel(hip, m) == "estep_docs_tiered_kernel"
                    assert hip.trlda_model_last_split_workgroups(m._handle) == (want_wgs if split_docs else 0)
                    assert hip.trlda_model_last_preamble_fused(m._handle) == 1 - two_kernel
                    missed += check(c, got, want, "max_iter %d mode %d split %d two-kernel preamble %d" % (
                        max_iter, mode, split_docs, two_kernel), atomic=mode == 1)
        hip.trlda_model_set_split_preamble(m._handle, 0)
        hip.trlda_model_set_split_docs(m._handle, 1)
        assert hip.trlda_model_set_doc_kernel(m._handle, 1) == 0          # TRLDA_DOCS_GENERAL
        for mode in (0, 1):
            hip.trlda_model_set_sstats_mode(m._handle, mode)
            got = m.update_variables(batch, latents=inp[5], max_iter=max_iter, threshold=c.threshold,
                                     return_iterations=True)
            assert kernel(hip, m) == "estep_docs_kernel"
            missed += check(c, got, want, "general kernel, max_iter %d mode %d" % (max_iter, mode), atomic=mode == 1)
    m.close()
    assert not missed, missed


@pytest.mark.parametrize("c", ac.cases("reg128") + ac.cases("reg144"), ids=ac.case_id)
def test_register_kernel(hip, expected, c):
    """No document over 128 words: estep_docs_reg_kernel, whose waves 6 and 7 form the stop test's sum
    from alpha_l[ka]; the longest at 144 words: the variant with 18 words per wave (a tiered launch).
    Both statistics modes, fused and two-kernel preamble."""
    inp = ac.build(c)
    m = make_model(c, inp[0], inp[1])
    missed = []
    batch = m.upload(documents(inp))
    for max_iter in iteration_limits(c):
        inp, want = expected(c, max_iter)
        for mode in (0, 1):
            for two_kernel in (0, 1):
                hip.trlda_model_set_sstats_mode(m._handle, mode)
                assert hip.trlda_model_set_split_preamble(m._handle, two_kernel) == 0
                got = m.update_variables(batch, latents=inp[5], max_iter=max_iter, threshold=c.threshold,
                                         return_iterations=True)
                assert kernel(hip, m) == ("estep_docs_reg_kernel" if max(c.lens) <= 128
                                          else "estep_docs_tiered_kernel")
                assert hip.trlda_model_last_split_workgroups(m._handle) == 0
                assert hip.trlda_model_last_preamble_fused(m._handle) == 1 - two_kernel
                missed += check(c, got, want, "max_iter %d mode %d two-kernel preamble %d" % (max_iter, mode, two_kernel),
                      atomic=mode == 1)
    m.close()
    assert not missed, missed


@pytest.mark.parametrize("c", ac.cases("wide"), ids=ac.case_id)
def test_single_orientation_kernel(hip, expected, c):
    """estep_docs_wide_kernel forced for every document, every slot count ceil(K / 64) = 1..8 and
    both sides of the 256-topic limit of its mirror waves (a.alpha[km], stop test only); from a random
    gamma0 and from a converged one."""
    inp = ac.build(c)
    m = make_model(c, inp[0], inp[1])
    missed = []
    batch = m.upload(documents(inp))
    assert hip.trlda_model_set_doc_kernel(m._handle, 2) == 0              # TRLDA_DOCS_WIDE
    for max_iter in iteration_limits(c):
        inp, want = expected(c, max_iter)
        for mode in (0, 1):
            hip.trlda_model_set_sstats_mode(m._handle, mode)
            got = m.update_variables(batch, latents=inp[5], max_iter=max_iter, threshold=c.threshold,
                                     return_iterations=True)
            assert kernel(hip, m) == "estep_docs_wide_kernel"
            missed += check(c, got, want, "max_iter %d mode %d" % (max_iter, mode), atomic=mode == 1)
    # from the gamma the E-step above ends with (an update loop's init_gamma=False): the documents that
    # had converged stop after one iteration -- if the FIRST sum |gamma - gamma0| is right, the only
    # one in which the mirror waves' alpha does not cancel (asymmetric_cases.warm_start)
    inp, want = expected(c, c.max_iter, warm=True)
    assert (want[2] == 1).any() and (want[2] > 1).any()
    for mode in (0, 1):
        hip.trlda_model_set_sstats_mode(m._handle, mode)
        got = m.update_variables(batch, latents=inp[5], max_iter=c.max_iter, threshold=c.threshold,
                                 return_iterations=True)
        assert kernel(hip, m) == "estep_docs_wide_kernel"
        missed += check(c, got, want, "warm start, mode %d" % mode, atomic=mode == 1)
    m.close()
    assert not missed, missed


@pytest.mark.parametrize("c", ac.cases("general"), ids=ac.case_id)
def test_general_kernel_above_512_topics(hip, expected, c):
    """estep_docs_kernel (a.alpha[k] in its LDS-tile and its streamed loop), the workgroup size left
    to the library, 64 and 1024 threads."""
    inp = ac.build(c)
    m = make_model(c, inp[0], inp[1])
    missed = []
    batch = m.upload(documents(inp))
    for max_iter in iteration_limits(c):
        inp, want = expected(c, max_iter)
        for threads in (0, 64, 1024):
            assert hip.trlda_model_set_doc_threads(m._handle, threads) == 0
            for mode in (0, 1):
                hip.trlda_model_set_sstats_mode(m._handle, mode)
                got = m.update_variables(batch, latents=inp[5], max_iter=max_iter, threshold=c.threshold,
                                         return_iterations=True)
                assert kernel(hip, m) == "estep_docs_kernel"
                missed += check(c, got, want, "max_iter %d threads %d mode %d" % (max_iter, threads, mode), atomic=mode == 1)
    m.close()
    assert not missed, missed


@pytest.mark.parametrize("c", ac.cases("small"), ids=ac.case_id)
def test_a_wave_per_document(hip, expected, c):
    """estep_docs_small_body forced (a.alpha[kc]): eight documents per workgroup, lengths around the
    64- and 128-word limits of a wave's passes, behind one 200-word document that keeps a workgroup
    of its own; fused and two-kernel preamble."""
    from trlda_amd import _ffi
    inp = ac.build(c)
    m = make_model(c, inp[0], inp[1])
    missed = []
    batch = m.upload(documents(inp))
    _ffi.check(hip.trlda_model_set_doc_kernel(m._handle, 3))               # TRLDA_DOCS_SMALL
    for max_iter in iteration_limits(c):
        inp, want = expected(c, max_iter)
        for two_kernel in (0, 1):
            assert hip.trlda_model_set_split_preamble(m._handle, two_kernel) == 0
            got = m.update_variables(batch, latents=inp[5], max_iter=max_iter, threshold=c.threshold,
                                     return_iterations=True)
            assert "small" in kernel(hip, m), kernel(hip, m)
            assert hip.trlda_model_last_preamble_fused(m._handle) == 1 - two_kernel
            missed += check(c, got, want, "max_iter %d two-kernel preamble %d" % (max_iter, two_kernel))
    m.close()
    assert not missed, missed


def run_stream(hip, c, lam, alpha, csrs, g0s, order, lanes, deferred, announce, max_iter):
    """the calls `order` of a stream of E-steps through trlda_model_estep_io_ahead, every call with
    output arrays of its own -> every call's (gamma, statistics, iterations), the steps that went
    through the lanes and trlda_model_last_deferred after every call"""
    from trlda_amd import _ffi
    m = make_model(c, lam, alpha)
    dev = [m.upload(x) for x in csrs]
    slots = [Slots(hip, c.K, c.V, csrs[i], g0s[i]) for i in order]
    devs = [dev[i] for i in order]
    _ffi.check(hip.trlda_model_set_deferred_stats(m._handle, deferred))
    _ffi.check(hip.trlda_model_set_stream_lanes(m._handle, lanes))
    flags = []
    for n in range(len(order)):
        ahead(hip, m, devs, slots, n, announce, max_iter)
        flags.append(hip.trlda_model_last_deferred(m._handle))
    through = hip.trlda_model_lane_steps(m._handle)
    _ffi.check(hip.trlda_model_synchronize(m._handle))
    res = [s.read() for s in slots]
    for s in slots:
        s.free()
    m.close()
    return res, through, flags


@pytest.mark.parametrize("K", [64, 128])
def test_merged_deferred_and_two_lane_streams(hip, expected, K):
    """(K, V, B) = (64, 900, 90) and (128, 3000, 64), two batches each (the second a tiered launch with
    split documents): the statistics as workgroups of the document launch (merged level 2), deferred
    into the next call's launch with two stream lanes and with one, and the plain kernels -- bitwise
    equal to each other, and equal to the oracle."""
    pair = [c for c in ac.cases("stream") if c.K == K]
    assert len(pair) == 2 and pair[0].threshold == pair[1].threshold == 1e-3     # (estep_io_ahead in `ahead`)
    ins = [expected(c, ac.MAX_ITER)[0] for c in pair]
    wants = [expected(c, ac.MAX_ITER)[1] for c in pair]
    lam, alpha = ins[0][0], ins[0][1]
    assert np.array_equal(ins[1][0], lam) and np.array_equal(ins[1][1], alpha)   # one model
    csrs = [documents(i) for i in ins]
    g0s = [i[5] for i in ins]
    c = pair[0]
    order = [0, 1, 0, 1]
    plain, through, flags = run_stream(hip, c, lam, alpha, csrs, g0s, order, lanes=1, deferred=0, announce=0,
                                       max_iter=ac.MAX_ITER)
    assert through == 0 and flags == [0] * len(order)
    one, through, flags = run_stream(hip, c, lam, alpha, csrs, g0s, order, lanes=1, deferred=1, announce=2,
                                     max_iter=ac.MAX_ITER)
    # (every call left its statistics to the next launch; which launches carried them depends on
    # whether the announced batch's index was there in time -- tests/test_gpu_deferred.py)
    assert through == 0 and all(f & 1 for f in flags), flags
    two, through, _ = run_stream(hip, c, lam, alpha, csrs, g0s, order, lanes=2, deferred=1, announce=2,
                                 max_iter=ac.MAX_ITER)
    assert through == len(order)
    m = make_model(c, lam, alpha)
    merged = []
    for level in (2, 0):
        assert hip.trlda_model_set_merged_launch(m._handle, level) == 0
        for i in (0, 1):
            merged.append(m.update_variables(csrs[i], latents=g0s[i], max_iter=ac.MAX_ITER, threshold=1e-3,
                                             return_iterations=True))
            assert hip.trlda_model_last_merged(m._handle) == (level == 2)
            assert kernel(hip, m) == ("estep_docs_tiered_kernel" if i else "estep_docs_reg_kernel")
            assert hip.trlda_model_last_split_workgroups(m._handle) == (4 if i else 0)   # 200 and 400 words
    m.close()
    missed = []
    for n, i in enumerate(order):
        missed += check(pair[i], plain[n], wants[i], "plain stream, call %d" % n)
        for name, other in (("deferred", one[n]), ("two lanes", two[n]), ("merged", merged[i]),
                            ("update_variables", merged[2 + i])):
            for q, array in enumerate(("gamma", "statistics", "iteration counts")):
                if not np.array_equal(other[q], plain[n][q]):
                    missed.append("call %d: %s of the %s form differ from the plain stream's" % (n, array, name))
    assert not missed, missed


@pytest.mark.parametrize("c", ac.cases("update"), ids=ac.case_id)
def test_update_loops(hip, oracle, c):
    """OnlineLDA.update_parameters with a vector alpha and a trust-region loop of three E-steps against
    oracle.online_update_parameters, at the bar tests/test_gpu_update_loop.py
    (test_fused_update_equals_plain_sequence) sets for the fused trajectory against the oracle:
    (64, 900, 90) through merged launches, (333, 13000, 40) through the big-table path (the single-
    orientation kernel, exp(psi(lambda)) left behind by the M-step)."""
    import trlda_amd
    D = 50000
    lam, alpha, ip, ids, cnts, _ = ac.build(c)
    m = make_model(c, lam, alpha, D=D)
    trlda_amd.seed(21)
    rho = m.update_parameters(documents((lam, alpha, ip, ids, cnts)), max_iter_tr=3, max_iter_inference=c.max_iter)
    big = c.K * c.V >= 1 << 22
    assert hip.trlda_model_last_merged(m._handle) == (0 if big else 1)
    assert kernel(hip, m) == ("estep_docs_wide_kernel" if big else "estep_docs_reg_kernel")
    got = np.array(m.lambdas)
    m.close()
    oracle.seed(21)
    rho_o, lam_o, _, _ = oracle.online_update_parameters(lam, alpha, .3, D, ip, ids, cnts, 0, max_iter_tr=3,
                                                         max_iter_inference=c.max_iter)
    print("%s: lambda %.2e" % (ac.case_id(c), relerr(got, lam_o)))
    assert rho == rho_o
    assert relerr(got, lam_o) < TIGHT_RTOL
