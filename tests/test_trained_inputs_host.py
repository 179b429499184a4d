"""The inputs of tests/test_gpu_trained_inputs.py can fail a wrong kernel: properties of the
restatements alone (gibbs_host, cvb0_host, l2r_host, marginal_host, heldout_host, wordtopics_host; the table from
scipy's digamma), for every case of tests/trained_cases.py -- the table the GPU module runs.

(a) The table regimes are what they are named: over the words of a case's chain the smallest e is
    normal and below 1e-40 at eta = 0.01, at least one is subnormal and non-zero at 1.4e-3, and at 1e-3
    a column holds exact zeros beside a positive entry.
(b) The fall-backs of the histogram draw are reached: over the table's Gibbs chains the restatement
    counts at least one draw that ends in 'last topic with p > 0' and at least one with a lane whose
    weights are all zero between a live lane and the chosen one; no draw ever picks a topic whose
    weight is not > 0.  Counted when the table was made, of 34 872 draws: last topic with p > 0 overall
    1 (the chain of trained_cases.FALLBACK_KEY; the rounding of u * total cannot reach it anywhere else,
    and the in-lane form needs r inside one rounding of a lane's sum: 0), an all-zero lane between a
    live lane and the chosen one 4 495.
(c) alpha is live: with alpha swapped between two topics a wrongly indexed kernel would confuse
    (trained_cases.pair_patterns) the chain gives other statistics, CVB0 another theta, and
    left_to_right, document_log_likelihood and predictive_log_likelihood another log-likelihood and
    word_topics another leading probability (by more than 1e-9 relative).
(d) The failure case fails: with an unseen word at eta = 1e-3 gibbs_host.gibbs meets a histogram whose
    total is 0.
"""
import numpy as np
import pytest

import cvb0_host
import gibbs_host
import heldout_host
import l2r_host
import marginal_host
import trained_cases as tc
import wordtopics_host

_MEMO = {}


def inputs(c):
    """(lambda, alpha, docs, docs_unseen, table) of a case, built once."""
    key = (c.K, c.V, c.eta, c.seed)
    if key not in _MEMO:
        lam, alpha, docs, unseen = tc.build(c)
        _MEMO[key] = (lam, alpha, docs, unseen, tc.host_table(lam))
    return _MEMO[key]


def chain(c, alpha, e=None, theta0=None, docs=None, key=None, ns=tc.NS, bi=tc.BI, stats=None):
    lam, _, d, _, table = inputs(c)
    indptr, ids, cnts = tc.csr(d if docs is None else docs)
    return gibbs_host.gibbs(table if e is None else e, alpha, indptr, ids, cnts, theta0, ns, bi,
                            tc.key_of(c) if key is None else key, stats=stats)


def result(oracle, c, alpha):
    """What the restatement of the case's entry point gives under `alpha`: the array that must move
    when alpha is read at a wrong index."""
    lam, _, docs, unseen, table = inputs(c)
    if c.entry == "gibbs":
        return chain(c, alpha)[1].astype(np.float64)
    if c.entry == "cvb0":
        indptr, ids, cnts = tc.csr(docs)
        return cvb0_host.cvb0(table, alpha, indptr, ids, cnts, None, tc.CVB0_ITER, tc.CVB0_THRESHOLD)[0]
    if c.entry == "l2r":
        indptr, ids, cnts = tc.csr(tc.l2r_docs(docs))
        return l2r_host.left_to_right(indptr, ids, cnts, lam, alpha, tc.key_of(c), tc.L2R_PARTICLES,
                                      False)[0]["particle"]
    if c.entry == "marginal":
        indptr, ids, cnts = tc.csr(docs)
        return marginal_host.document_loglik(indptr, ids, cnts, lam, alpha, tc.key_of(c),
                                             tc.MARGINAL_SAMPLES)[0]
    if c.entry == "heldout":
        indptr, ids, cnts = tc.csr(docs)
        g0 = np.asfortranarray(np.random.RandomState(c.K).gamma(1., 1., (c.K, len(docs))) + .1)
        gamma = oracle.estep(lam, alpha, indptr, ids, cnts, g0, 20, 1e-3, nthreads=8)[0]
        return heldout_host.score(*tc.csr(unseen), gamma, lam)[0]
    if c.entry == "wordtopics":
        indptr, ids, cnts = tc.csr(docs)
        g0 = np.asfortranarray(np.random.RandomState(c.K).gamma(1., 1., (c.K, len(docs))) + .1)
        gamma = oracle.estep(lam, alpha, indptr, ids, cnts, g0, 20, 1e-3, nthreads=8)[0]
        with np.errstate(under="ignore"):
            return wordtopics_host.word_topics(indptr, ids, gamma, lam, 1)[2]
    raise ValueError(c.entry)


def moved(a, b):
    """the largest relative move between two results"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-300)))


GIBBS = tc.cases("gibbs")
ALPHA_LIVE = [c for c in tc.CASES if c.entry != "sample"]          # (sample's theta ~ Dir(alpha): test_gpu_sample)


@pytest.mark.parametrize("c", GIBBS, ids=tc.case_id)
def test_the_table_regimes_are_what_they_are_named(c):
    lam, alpha, docs, unseen, e = inputs(c)
    words = tc.words_of(docs)
    assert not set(words) & {c.V - 1, c.V - 2} and set(tc.words_of(unseen)) >= {c.V - 1, c.V - 2}
    cols = e[:, words]
    tiny = np.finfo(np.float64).tiny
    assert not np.isnan(cols).any() and (cols >= 0).all()
    if c.eta == 0.3:
        assert cols.min() >= 1e-10
    elif c.eta == 0.01:
        assert tiny <= cols.min() < 1e-40, cols.min()
    elif c.eta == 1.4e-3:
        assert ((cols > 0) & (cols < tiny)).any() and (cols > 0).all(), cols.min()
        assert ((e[:, c.V - 2:] > 0) & (e[:, c.V - 2:] < tiny)).all()          # the unseen words: all of it
    else:
        both = ((cols == 0).any(axis=0) & (cols > 0).any(axis=0))
        assert both.any()
        assert (cols > 0).any(axis=0).all()                  # every word of a chain has a live topic
        assert not e[:, c.V - 2:].any()                      # the unseen words have none


def test_the_generator_is_what_it_says():
    for K in (3, 200):
        a = tc.trained_case(K, tc.V, 0.01, 4)
        b = tc.trained_case(K, tc.V, 1e-3, 4)
        lam, alpha, docs, unseen = a
        assert lam.flags.f_contiguous and lam.shape == (K, tc.V) and alpha.shape == (K,)
        S = lam - 0.01
        assert np.array_equal(np.rint(S), np.round(S, 6)) and (np.rint(S) >= 0).all()
        assert np.array_equal(np.rint(S), np.rint(b[0] - 1e-3))            # the same counts for every eta
        assert np.array_equal(alpha, b[1]) and docs == b[2] and unseen == b[3]
        S = np.rint(S)
        stop = (S >= 1e3).all(axis=0)
        assert stop.sum() == tc.V // 20 and S[:, stop].max() <= 1e5
        own = (S > 0) & ~stop[None, :]
        assert (own.sum(axis=1) >= 3).all() and S[own].max() <= 1e4 and S[own].min() >= 1
        assert not S[:, -2:].any()
        assert (S == 0).mean() > 0.8                          # sparse
        rs = lam.sum(axis=1)
        assert rs.min() >= 1e4 and rs.max() <= 1e6
        assert np.allclose(np.sort(alpha), np.logspace(np.log10(2e-3), np.log10(4.), K), rtol=1e-14)
        assert len(docs) == 6 and docs[1] == []
        ids2 = [w for w, _ in docs[2]]
        assert len(set(ids2)) < len(ids2) and 0 in [n for _, n in docs[2]]
        assert 250 <= sum(n for _, n in docs[3]) <= 350
        assert all((S[:, w] > 0).any() for d in docs for w, _ in d)
        assert (tc.V - 1, 2) in unseen[0] and unseen[5] == [(tc.V - 2, 1)]
    big = tc.build(tc.table_cases()[-1])[0]
    assert big.shape[1] == 2000 and 1e4 <= big.sum(axis=1).min() and big.sum(axis=1).max() <= 1e6


def fallback_case():
    return next(c for c in GIBBS if c.K == tc.FALLBACK_K and c.eta == tc.FALLBACK_ETA)


def test_the_fallbacks_of_the_draw_are_reached():
    total = {}
    for c in GIBBS:
        lam, alpha, docs, unseen, e = inputs(c)
        for theta0 in (tc.theta0(c.K, len(docs), c.seed), None):
            chain(c, alpha, theta0=theta0, stats=total)
    c = fallback_case()
    lam, alpha, docs, unseen, e = inputs(c)
    one = {}
    chain(c, alpha, theta0=tc.theta0(c.K, len(docs), c.seed), docs=unseen, key=tc.FALLBACK_KEY,
          ns=tc.FALLBACK_NS, bi=tc.FALLBACK_BI, stats=one)
    for name, n in one.items():
        total[name] = total.get(name, 0) + n
    print("draws %d: last topic with p > 0 in the lane %d, overall %d; a zero lane below the chosen one %d" %
          (total["draws"], total.get("last_in_lane", 0), total.get("last_overall", 0),
           total.get("zero_lane_below", 0)))
    assert total.get("last_in_lane", 0) + total.get("last_overall", 0) >= 1
    assert one.get("last_overall", 0) >= 1                   # where it was put
    assert total.get("zero_lane_below", 0) >= 1
    assert total.get("zero_weight_pick", 0) == 0


@pytest.mark.parametrize("c", ALPHA_LIVE, ids=tc.case_id)
def test_swapped_alphas_give_another_result(oracle, c):
    lam, alpha, docs, unseen, e = inputs(c)
    patterns = tc.pair_patterns(c.entry, c.K)
    assert len(c.pairs) == len(patterns)
    base = result(oracle, c, alpha)
    assert np.all(np.isfinite(base))
    for pair, pattern in zip(c.pairs, patterns):
        assert pair in pattern, pair
        other = result(oracle, c, tc.swapped(alpha, pair))
        if c.entry == "gibbs":
            assert not np.array_equal(base, other), pair
        else:
            assert moved(base, other) > 1e-9, (pair, moved(base, other))


@pytest.mark.parametrize("K", tc.KS["gibbs"])
def test_the_failure_case_fails(K):
    c = next(x for x in GIBBS if x.K == K and x.eta == 1e-3)
    lam, alpha, docs, unseen, e = inputs(c)
    for theta0 in (tc.theta0(c.K, len(docs), c.seed), None):
        with pytest.raises(RuntimeError, match="Something went wrong while sampling from histogram."):
            chain(c, alpha, theta0=theta0, docs=unseen)
    # and it is the unseen words' doing: each of the two documents that hold one fails alone
    indptr, ids, cnts = tc.csr(unseen)
    for d in (0, 5):
        with pytest.raises(RuntimeError, match="sampling from histogram"):
            gibbs_host.gibbs(e, alpha, indptr, ids, cnts, None, tc.NS, tc.BI, tc.key_of(c), docs=[d])
    gibbs_host.gibbs(e, alpha, indptr, ids, cnts, None, tc.NS, tc.BI, tc.key_of(c), docs=[1, 2, 3, 4])
