"""CPU checks of the word similarities: the restatement (tests/wordsim_host.py) against a brute-force
float128 loop and on hand cases, what the library and ``LDA.similar_words`` / ``words_near`` /
``word_topic_proportions`` answer before any GPU work, and the kernels' resources read off the code
object."""
import math

import numpy as np
import pytest

import wordsim_host as wh

LD = np.longdouble


# -- the restatement ------------------------------------------------------------------------------
def _brute(lam, measure, weights):
    """s(q, w) for all pairs by scalar longdouble loops straight from the definitions."""
    K, V = lam.shape
    R = [sum(LD(lam[k, v]) for v in range(V)) for k in range(K)]
    if weights is None:
        tot = sum(R)
        pi = [R[k] / tot for k in range(K)]
    else:
        tot = sum(LD(x) for x in weights)
        pi = [LD(weights[k]) / tot for k in range(K)]
    a = [[pi[k] / R[k] * LD(lam[k, w]) for k in range(K)] for w in range(V)]
    rows = []
    for w in range(V):
        if measure == "hellinger":
            p = sum(a[w])
            rows.append([np.sqrt(x / p) for x in a[w]])
        else:
            n = np.sqrt(sum(x * x for x in a[w]))
            rows.append([x / n for x in a[w]])
    s = np.empty((V, V), dtype=LD)
    for q in range(V):
        for w in range(V):
            s[q, w] = sum(rows[q][k] * rows[w][k] for k in range(K))
    return s, a


@pytest.mark.parametrize("measure", ["hellinger", "cosine"])
@pytest.mark.parametrize("given", [False, True])
def test_restatement_against_brute_force(measure, given):
    K, V = 3, 7
    rng = np.random.RandomState(11)
    lam = rng.gamma(0.3, 1.0, size=(K, V)) + 0.01
    weights = rng.gamma(2.0, 1.0, K) + 0.1 if given else None
    want, a = _brute(lam, measure, weights)
    r = wh.rows(lam, measure, weights)
    got = wh.similarities(r, r)
    assert float(np.max(np.abs(got - want))) <= 1e-17
    assert float(np.max(np.abs(np.diag(got) - 1))) <= 1e-17          # unit rows
    p = wh.proportions(lam, weights)
    for w in range(V):
        tot = sum(a[w])
        assert max(abs(float(p[k, w] - a[w][k] / tot)) for k in range(K)) <= 1e-18
    assert float(np.max(np.abs(p.sum(axis=0) - 1))) <= 1e-18
    assert np.array_equal(wh.proportions(lam, weights, words=[5, 0, 5]), p[:, [5, 0, 5]])
    # the search: the self pair leaves by id, the order is (s descending, id ascending)
    ids, s, gap = wh.search(r[[2, 6]], r, 4, self_ids=[2, 6])
    for b, q in enumerate((2, 6)):
        cand = [w for w in range(V) if w != q]
        order = sorted(cand, key=lambda w: (-want[q, w], w))
        assert list(ids[b]) == order[:4] and ids.dtype == np.int32
        assert float(np.max(np.abs(s[b] - want[q, order[:4]]))) <= 1e-17
    both = [sorted((float(want[q, w]) for w in range(V) if w != q), reverse=True)[:5] for q in (2, 6)]
    assert abs(gap - min(x - y for row in both for x, y in zip(row[:-1], row[1:]))) <= 1e-16
    ids, s, _ = wh.search(r[[2]], r, 3)
    assert ids[0, 0] == 2                                            # nothing left out: the word itself first


def test_equal_columns_tie_and_rank_by_id():
    """Word 4 copies word 1 and word 5 is 4 x word 1: equal p(k | w), s = 1 against each other; a
    query's list holds the equal columns next to each other in id order, and only the query leaves."""
    rng = np.random.RandomState(2)
    lam = rng.gamma(0.3, 1.0, size=(4, 6)) + 0.01
    lam[:, 4] = lam[:, 1]
    lam[:, 5] = 4.0 * lam[:, 1]
    for measure in ("hellinger", "cosine"):
        r = wh.rows(lam, measure)
        assert np.array_equal(r[1], r[4])
        ids, s, gap = wh.search(r[[1, 4]], r, 3, self_ids=[1, 4])
        assert list(ids[0][:2]) == [4, 5] and list(ids[1][:2]) == [1, 5]
        assert s[0, 0] == s[1, 0] and abs(float(s[0, 1]) - 1) <= 1e-18
        assert wh.distance(np.array([1.0 + 1e-16, 1.0, 0.75]), measure)[0] == 0.0
    p = wh.proportions(lam)
    assert float(np.max(np.abs(p[:, 5] - p[:, 1]))) <= 1e-19
    assert wh.distance(np.array([0.75]), "hellinger")[0] == 0.5 and wh.distance(np.array([0.75]), "cosine")[0] == 0.25


def test_given_weights_change_the_answer():
    """Two topics.  Word 0 lives in topic 0 and a little in topic 1.  Candidate 1 is pure topic 0 up
    to a trace, candidate 2 is even.  With weights on topic 0, word 0's p(k | w) is near (1, 0): 1 is
    nearer; with weights on topic 1 it is pulled to the even side: 2 is nearer."""
    lam = np.array([[8.0, 9.0, 1.0], [1.0, 0.01, 1.0]])
    for measure in ("hellinger", "cosine"):
        first = {}
        for name, w in (("zero", [100.0, 1.0]), ("one", [1.0, 100.0])):
            r = wh.rows(lam, measure, w)
            ids, _, gap = wh.search(r[[0]], r, 2, self_ids=[0])
            first[name] = int(ids[0, 0])
            assert gap > 1e-3
        assert first == {"zero": 1, "one": 2}, (measure, first)


def test_the_bound_is_a_function_of_the_shape():
    for measure in ("hellinger", "cosine"):
        assert wh.sim_bound(1, measure) < wh.sim_bound(100, measure) < wh.sim_bound(2276, measure)
        assert wh.sim_bound(100, measure, V=300) > wh.sim_bound(100, measure, V=0)
        assert wh.sim_bound(100, measure, V=300, given=False) < wh.sim_bound(100, measure, V=300)
        for K, V in ((2276, 300), (100, 2100)):          # three orders below the gap floor of the GPU tests
            assert wh.sim_bound(K, measure, V=V) <= 1e-3 * 1e-9
    assert wh.sim_bound(100, "hellinger", V=300) == (2 * 302 + 100 + 28 + 8) * wh.U
    assert wh.sim_bound(100, "cosine", V=300) == (4 * 302 + 100 + 28 + 7) * wh.U
    with pytest.raises(ValueError):
        wh.sim_bound(3, "euclid")


# -- the library ----------------------------------------------------------------------------------
def _bare(K, V):
    """An LDA that has no device side: whatever it raises, it raises before any GPU work."""
    from trlda_amd.models import LDA
    m = LDA.__new__(LDA)
    m._handle, m._K, m._V, m._device = None, K, V, 0
    return m


def test_argument_errors_come_before_any_gpu_work():
    import trlda.models
    from trlda_amd.models import LDA
    assert trlda.models.LDA is LDA
    for name in ("similar_words", "words_near", "word_topic_proportions"):
        assert callable(getattr(LDA, name)) and "DESIGN.md 3.28" in getattr(LDA, name).__doc__
    m = _bare(3, 200)
    for top_n in (0, -1, 101):
        with pytest.raises(RuntimeError, match="top_n"):
            m.similar_words([1], top_n=top_n)
        with pytest.raises(RuntimeError, match="top_n"):
            m.words_near(np.ones(3), top_n=top_n)
    small = _bare(3, 7)
    with pytest.raises(RuntimeError, match="top_n"):
        small.similar_words([1], top_n=7)                 # V - 1 = 6 candidates
    with pytest.raises(RuntimeError, match="top_n"):
        small.similar_words([1], top_n=8, exclude_self=False)
    with pytest.raises(RuntimeError, match="top_n"):
        small.words_near(np.ones(3), top_n=8)
    with pytest.raises(TypeError):
        m.similar_words([1], top_n=2.5)
    # measure: the names and errors of the document index
    with pytest.raises(TypeError, match="measure"):
        m.similar_words([1], measure=0)
    with pytest.raises(ValueError, match="Unknown measure"):
        m.similar_words([1], measure="euclid")
    with pytest.raises(ValueError, match="Unknown measure"):
        m.words_near(np.ones(3), measure="euclid")
    # word ids
    for bad in (1.5, [1, 2.0], "word", [None], np.array([1.0, 2.0])):
        with pytest.raises(TypeError):
            m.similar_words(bad)
        with pytest.raises(TypeError):
            m.word_topic_proportions(bad)
    for bad in (-1, 200, [0, 199, 200], np.array([3, -2])):
        with pytest.raises(RuntimeError, match="[Ww]ord id"):
            m.similar_words(bad)
        with pytest.raises(RuntimeError, match="[Ww]ord id"):
            m.word_topic_proportions(bad)
    # weights
    for pi in (np.ones(4), np.r_[1.0, 1.0, 0.0], np.r_[1.0, np.nan, 1.0], np.r_[1.0, np.inf, 1.0], np.r_[1.0, -1.0, 1.0]):
        with pytest.raises(RuntimeError, match="topic_weights"):
            m.similar_words([1], topic_weights=pi)
        with pytest.raises(RuntimeError, match="topic_weights"):
            m.words_near(np.ones(3), topic_weights=pi)
        with pytest.raises(RuntimeError, match="topic_weights"):
            m.word_topic_proportions([1], topic_weights=pi)
    # proportions: shape, type, finite and positive
    for bad in (np.ones((4, 2)), np.ones((2, 3, 1)), np.ones(4)):
        with pytest.raises(RuntimeError, match="wrong dimensionality"):
            m.words_near(bad)
    with pytest.raises(TypeError):
        m.words_near("theta")
    for bad in (0.0, -1.0, np.inf, np.nan):
        spoiled = np.ones((3, 2))
        spoiled[2, 1] = bad
        with pytest.raises(RuntimeError, match="finite and positive"):
            m.words_near(spoiled)
    # nothing to do needs no device either
    ids, dist = m.similar_words([], top_n=4)
    assert ids.shape == dist.shape == (0, 4) and ids.dtype == np.int32 and dist.dtype == np.float64
    ids, dist = m.words_near(np.empty((3, 0)), top_n=4)
    assert ids.shape == dist.shape == (0, 4)
    p = m.word_topic_proportions([])
    assert p.shape == (3, 0) and p.flags.f_contiguous and p.dtype == np.float64


def test_wordsim_entry_points_are_exported(hip_lib):
    from trlda_amd import _ffi
    for name in ("trlda_model_similar_words", "trlda_model_similar_words_rows",
                 "trlda_model_word_topic_proportions", "trlda_model_set_wordsim_slab_words"):
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    # (no model: the argument check answers before any device is touched)
    assert hip_lib.trlda_model_similar_words(None, None, 1, 1, 0, None, 1, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_model_similar_words_rows(None, None, 1, 1, 0, None, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_model_word_topic_proportions(None, None, 1, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_model_set_wordsim_slab_words(None, 16) == _ffi.ERR_ARG


def test_wordsim_kernels_do_not_spill(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    mine = {k: v for k, v in res.items() if "wordsim_" in k}
    assert len(mine) == 5, sorted(mine)                  # norm, rows, props, query<1>, query<2>
    for part in ("wordsim_norm_kernel", "wordsim_rows_kernel", "wordsim_props_kernel",
                 "wordsim_query_kernelILi1E", "wordsim_query_kernelILi2E"):
        assert sum(part in k for k in mine) == 1, (part, sorted(mine))
    for name, f in mine.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_spill_count"] == 0, (name, f)
        if "query" in name:
            assert f["vgpr_count"] <= 256, (name, f)     # two waves per SIMD, both widths


def test_query_lds_fits():
    """docindex_query_lds plus the scales and ids, as csrc/wordsim_kernels.h sizes it: within 160 KiB
    at the largest top_n of either width."""
    def lds(sw, top_n):
        return (64 * sw + 64) * 34 * 8 + 64 * sw * top_n * 12 + (64 + 64 * sw) * 8 + 64 * sw * 4
    assert lds(1, 100) <= 160 * 1024 and lds(2, 32) <= 160 * 1024
    assert lds(2, 100) > 160 * 1024                      # why the wide tile stops at top_n = 32
    assert math.ceil(lds(1, 100) / 1024) == 111
