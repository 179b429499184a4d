"""The inputs of tests/test_gpu_topic_asymmetry.py can fail a wrong kernel: three properties of the
oracle alone (oracle/cpu_ref.c, LDA::updateVariablesVI, reference src/lda.cpp:160-220), for every
case of tests/asymmetric_cases.py -- the table the GPU module runs.

(a) No near ties: no document's iteration count changes when the threshold moves by 1e-6 relative
    either way, so a device that sums in another order stops every document where the oracle does
    and a different count is a finding, not rounding.
(b) The stop test is live: at least three distinct counts, a document below the cap and one at it.
(c) The inputs discriminate: swapping alpha between two topics a wrongly indexed kernel would
    confuse (asymmetric_cases.swap_pairs) moves a gamma entry by more than 1e-3 relative AND changes
    a document's iteration count -- the mirror waves' alpha only shows in the counts.

And the bars: the fp64 oracle against the same fixed point in np.longdouble (estep_longdouble of the
GPU module).  Ten times the oracle's own distance is inside TIGHT_RTOL for every case but those the
GPU module lists as ORACLE_LIMITED, which do need their own bar."""
import numpy as np
import pytest

import asymmetric_cases as ac


@pytest.fixture(scope="module")
def measured(oracle):
    memo = {}

    def get(c):
        if c not in memo:
            memo[c] = ac.host_conditions(oracle, c)
        return memo[c]
    return get


CASES = ac.CASES


@pytest.mark.parametrize("c", CASES, ids=ac.case_id)
def test_no_document_is_near_a_tie_at_the_threshold(measured, c):
    r = measured(c)
    assert np.array_equal(r["iters_lo"], r["iters"]), np.nonzero(r["iters_lo"] != r["iters"])[0]
    assert np.array_equal(r["iters_hi"], r["iters"]), np.nonzero(r["iters_hi"] != r["iters"])[0]


@pytest.mark.parametrize("c", CASES, ids=ac.case_id)
def test_the_stop_test_is_live(measured, c):
    it = measured(c)["iters"]
    assert len(set(it.tolist())) >= 3, sorted(set(it.tolist()))
    assert (it < c.max_iter).any() and (it == c.max_iter).any(), sorted(set(it.tolist()))


@pytest.mark.parametrize("c", CASES, ids=ac.case_id)
def test_swapped_alphas_move_gamma_and_an_iteration_count(measured, c):
    swaps = measured(c)["swaps"]
    patterns = ac.pair_patterns(c.K)
    assert len(swaps) == len(patterns) == 1 + (c.K > 64) + (128 < c.K <= 256)
    for ((i, j), move, changed), pattern in zip(swaps, patterns):
        assert (i, j) in pattern, (i, j)
        assert move > 1e-3, ((i, j), move)
        assert changed >= 1, ((i, j), changed)


def test_the_builder_is_what_it_says():
    """peaked lambda (entries over five decades), alpha log-spaced over [2e-3, 4] in a shuffled
    order, counts 1..4 (0 only when asked for), distinct ids per document, reproducible"""
    from helpers import asymmetric_case
    lens = [0, 1, 40, 300]
    lam, alpha, ip, ids, cnts, g0 = asymmetric_case(20, 300, lens, 5)
    assert lam.flags.f_contiguous and g0.flags.f_contiguous
    assert lam.shape == (20, 300) and g0.shape == (20, 4) and alpha.shape == (20,)
    assert lam.min() >= .01 and lam.max() / lam.min() > 1e5
    assert np.allclose(np.sort(alpha), np.logspace(np.log10(2e-3), np.log10(4.), 20), rtol=1e-14)
    assert not np.array_equal(alpha, np.sort(alpha))
    assert list(np.diff(ip)) == lens and ip.dtype == ids.dtype == cnts.dtype == np.int32
    assert cnts.min() >= 1 and cnts.max() <= 4
    for d in range(len(lens)):
        assert len(set(ids[ip[d]:ip[d + 1]].tolist())) == lens[d]
    again = asymmetric_case(20, 300, lens, 5)
    assert all(np.array_equal(x, y) for x, y in zip(again, (lam, alpha, ip, ids, cnts, g0)))
    z = asymmetric_case(20, 300, lens, 5, zero_counts=True)[4]
    assert 0 < (z == 0).sum() < len(z) // 4 and np.array_equal(z[z > 0], cnts[z > 0])


@pytest.mark.parametrize("c", [c for c in ac.CASES if c.group != "update" and c.K <= 512], ids=ac.case_id)
def test_the_oracle_against_the_long_double_restatement(oracle, c):
    """the same iteration counts; gamma and statistics ten times closer than the GPU tests' bar, except
    the statistics of the cases held to ten times the oracle's own distance"""
    from helpers import TIGHT_RTOL
    from test_gpu_topic_asymmetry import ORACLE_LIMITED, oracle_distance
    inp = ac.build(c)
    want = oracle.estep(*inp, c.max_iter, c.threshold, nthreads=8)
    own_g, own_s = oracle_distance(inp, want, c.max_iter, c.threshold)       # (asserts the counts)
    assert 10. * own_g < TIGHT_RTOL, own_g
    if ac.case_id(c) in ORACLE_LIMITED:
        assert TIGHT_RTOL < 10. * own_s < 1e-7, own_s
    else:
        assert 10. * own_s < TIGHT_RTOL, own_s


def test_every_oracle_limited_case_exists():
    from test_gpu_topic_asymmetry import ORACLE_LIMITED
    assert ORACLE_LIMITED <= {ac.case_id(c) for c in ac.CASES}


@pytest.mark.parametrize("c", ac.cases("wide"), ids=ac.case_id)
def test_warm_started_cases_stop_at_the_first_iteration_or_not_at_all_early(oracle, c):
    """asymmetric_cases.warm_start: no near tie, documents that stop after one iteration beside
    documents that go on, and every swap pair changes a count -- through the first iteration's
    sum |gamma - gamma0|, the one place where the alpha of the single-orientation kernel's mirror
    waves shows."""
    r = ac.host_conditions(oracle, c, warm=True)
    it = r["iters"]
    assert np.array_equal(r["iters_lo"], it) and np.array_equal(r["iters_hi"], it)
    assert (it == 1).any() and (it > 1).any(), it
    for (i, j), move, changed in r["swaps"]:
        assert move > 1e-3 and changed >= 1, ((i, j), move, changed)
