"""CPU checks of the topic distances: the restatement (tests/topicdist_host.py) against by-hand values
on a K = 2, K' = 3, V = 3 case, the greedy matching's tie order, and what the library and
``LDA.topic_distances`` / ``LDA.match_topics`` answer before any GPU work."""
import numpy as np
import pytest

import topicdist_host as th

LN2, LN3 = np.log(2.0), np.log(3.0)
# p_0 = (1/4, 1/2, 1/4), p_1 = (1/4, 1/4, 1/2)
LAM = np.array([[1.0, 2.0, 1.0],
                [1.0, 1.0, 2.0]])
# q_0 = p_0 (twice lambda_0), q_1 = (1/8, 1/8, 3/4), q_2 = (1/2, 1/4, 1/4)
MU = np.array([[2.0, 4.0, 2.0],
               [1.0, 1.0, 6.0],
               [2.0, 1.0, 1.0]])
TOL = 1e-15


@pytest.fixture(scope="module")
def hand():
    return th.distances(LAM, MU)


def test_topics_by_hand():
    assert np.array_equal(th.topics(LAM).astype(np.float64), [[.25, .5, .25], [.25, .25, .5]])
    assert np.array_equal(th.topics(MU).astype(np.float64), [[.25, .5, .25], [.125, .125, .75], [.5, .25, .25]])


def test_hellinger_by_hand(hand):
    D, bc = hand["hellinger"]
    assert D.shape == (2, 3) and D.dtype == np.longdouble
    want = np.sqrt(1 / 32.) + 0.25 + np.sqrt(3.) / 4              # (0, 1)
    assert abs(float(bc[0, 1]) - want) <= TOL and abs(float(D[0, 1]) - np.sqrt(1 - want)) <= TOL
    want = np.sqrt(1 / 8.) + 0.25 + np.sqrt(1 / 8.)               # (1, 2)
    assert abs(float(bc[1, 2]) - want) <= TOL
    # by the other form: H^2 = 1/2 sum (sqrt p - sqrt q)^2
    p, q = th.topics(LAM), th.topics(MU)
    for i in range(2):
        for j in range(3):
            h2 = 0.5 * float(((np.sqrt(p[i]) - np.sqrt(q[j])) ** 2).sum())
            assert abs(float(D[i, j]) ** 2 - h2) <= TOL


def test_cosine_by_hand(hand):
    D, (c, num, n_p, n_q) = hand["cosine"]
    assert abs(float(num[0, 2]) - 0.3125) <= TOL and abs(float(n_p[0]) ** 2 - 0.375) <= TOL
    assert abs(float(c[0, 2]) - 5. / 6) <= TOL and abs(float(D[0, 2]) - 1. / 6) <= TOL
    # (1, 1): (1/32 + 1/32 + 3/8) / (sqrt(3/8) sqrt(19/32))
    assert abs(float(c[1, 1]) - (7. / 16) / np.sqrt(3. / 8 * 19. / 32)) <= TOL
    assert np.all(D >= 0) and np.all(D <= 1)


def test_kl_by_hand_and_asymmetric(hand):
    D, A = hand["kl"]
    assert abs(float(D[0, 2]) - 0.25 * LN2) <= TOL
    assert abs(float(D[0, 1]) - (1.25 * LN2 - 0.25 * LN3)) <= TOL
    back = th.distances(MU, LAM)["kl"][0]                         # q first
    assert abs(float(back[1, 0]) - (-0.375 * LN2 + 0.75 * LN3)) <= TOL
    assert abs(float(back[1, 0]) - float(D[0, 1])) > 0.02         # asymmetric: 0.5640 against 0.5918
    assert np.all(D >= 0) and np.all(A >= np.abs(D))
    # A of (0, 2): (|lambda log lambda| + |lambda log mu|) / S + |log S| + |log T|, S = T = 4
    want = (2 * LN2 + (LN2 + 0 + 0)) / 4 + 2 * LN2 + 2 * LN2
    assert abs(float(A[0, 2]) - want) <= 4 * TOL


def test_jensen_shannon_by_hand(hand):
    D, A = hand["jensen_shannon"]
    hm = -(0.75 * np.log(0.375) + 0.25 * np.log(0.25))            # (0, 2): m = (3/8, 3/8, 1/4)
    assert abs(float(D[0, 2]) - (hm - 1.5 * LN2)) <= TOL          # H(p_0) = H(q_2) = 3/2 ln 2
    assert abs(float(A[0, 2]) - (hm + 1.5 * LN2)) <= TOL
    assert np.all(D >= -TOL) and np.all(D <= LN2)
    # disjoint supports reach ln 2 (nearly: the restatement needs positive entries)
    far = th.distances([[1.0, 1e-30]], [[1e-30, 1.0]])["jensen_shannon"][0]
    assert abs(far[0, 0] - np.log(np.longdouble(2))) <= 1e-17
    # symmetric in the two topics
    assert abs(float(th.distances(MU, LAM)["jensen_shannon"][0][2, 0]) - float(D[0, 2])) <= TOL


def test_identical_topics_give_zero(hand):
    for measure in th.MEASURES:
        assert abs(float(hand[measure][0][0, 0])) <= TOL, measure     # q_0 = p_0
        own = th.distances(LAM, LAM)[measure][0]
        assert np.all(np.abs(np.diag(own).astype(np.float64)) <= TOL)
        assert float(own[0, 1]) > 0.01


def test_greedy_match_tie_order_and_leftover_rows():
    from trlda_amd.models import _greedy_match
    D = np.array([[0.5, 0.2, 0.2],
                  [0.2, 0.2, 0.9],
                  [0.2, 0.7, 0.1]])
    # 0.1 -> (2, 2); of the 0.2s, in (i, j) order: (0, 1) is first; (0, 2) has lost its column and row;
    # (1, 0) is next
    for fn in (th.greedy_match, _greedy_match):
        match, dist = fn(D)
        assert match.dtype == np.int64 and dist.dtype == np.float64
        assert list(match) == [1, 0, 2] and list(dist) == [0.2, 0.2, 0.1]
        # equal entries everywhere: the identity, by (i, j)
        match, dist = fn(np.full((3, 4), 0.25))
        assert list(match) == [0, 1, 2] and list(dist) == [0.25] * 3
        # K > K': the rows left over
        match, dist = fn(np.array([[0.3], [0.1], [0.3]]))
        assert list(match) == [-1, 0, -1] and list(dist) == [np.inf, 0.1, np.inf]
        match, dist = fn(np.array([[0.4, 0.3], [0.1, 0.3], [0.1, 0.2], [0.05, 0.9]]))
        assert list(match) == [-1, -1, 1, 0] and list(dist) == [np.inf, np.inf, 0.2, 0.05]


def test_min_gap():
    assert th.min_gap(np.array([[0.5, 0.25], [0.125, 0.75]])) == 0.125
    assert th.min_gap(np.array([[0.5, 0.25], [0.5, 0.75]])) == 0.0
    assert th.min_gap(np.array([[0.5]])) == float("inf")


# -- the library ----------------------------------------------------------------------------------
def _shell(K=2, V=5):
    """An LDA that has no device side: every check below is answered before one would be needed."""
    from trlda_amd.models import LDA
    m = LDA.__new__(LDA)
    m._handle = None
    m._K, m._V, m._device = K, V, 0
    return m


def test_measure_errors_come_before_the_model_is_looked_at():
    from trlda_amd.models import LDA, _topic_measure
    m = LDA.__new__(LDA)
    m._handle = None                                     # (no K, V or device either)
    for call in (m.topic_distances, m.match_topics):
        with pytest.raises(ValueError):
            call(None, measure="jensen-shannon")
        with pytest.raises(ValueError):
            call(None, measure="")
        for bad in (None, 0, b"kl", ["hellinger"]):
            with pytest.raises(TypeError):
                call(None, measure=bad)
    assert _topic_measure("Hellinger") == 0 and _topic_measure("COSINE") == 1 and _topic_measure("Kl") == 2
    assert _topic_measure("jensen_shannon") == _topic_measure("JS") == _topic_measure("Jensen_Shannon") == 3


def test_other_errors_come_before_any_gpu_work():
    m = _shell(K=2, V=5)
    for bad in ("a model", b"bytes", 3, 2.5, {"a": 1}, object()):
        with pytest.raises(TypeError):
            m.topic_distances(bad)
        with pytest.raises(TypeError):
            m.match_topics(bad)
    with pytest.raises(ValueError):
        m.topic_distances(_shell(K=3, V=6))              # another number of words
    other = _shell(K=3, V=5)
    other._device = 1
    with pytest.raises(ValueError):
        m.topic_distances(other)                         # another device
    good = np.ones((3, 5))
    for bad in (np.ones(5), np.ones((3, 4)), np.ones((2, 3, 5)), np.ones((0, 5))):
        with pytest.raises(ValueError):
            m.topic_distances(bad)
    for value in (0.0, -1.0, np.nan, np.inf):
        arr = good.copy()
        arr[2, 4] = value
        with pytest.raises(ValueError):
            m.topic_distances(arr)
        with pytest.raises(ValueError):
            m.match_topics(arr.tolist())
    with pytest.raises(ValueError):
        m.match_topics(None)
    # what passes the checks reaches the model, which is closed
    for ok in (None, m, good, good.tolist(), _shell(K=3, V=5)):
        with pytest.raises(RuntimeError):
            m.topic_distances(ok)


def test_topicdist_entry_points_are_exported(hip_lib):
    from trlda_amd import _ffi
    for name in ("trlda_model_topic_distances", "trlda_model_set_topicdist_chunk"):
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    # (no model: the argument check answers before any device is touched)
    assert hip_lib.trlda_model_topic_distances(None, None, None, 1, 0, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_model_set_topicdist_chunk(None, 0) == _ffi.ERR_ARG


def test_topicdist_kernels_do_not_spill(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    mine = {k: v for k, v in res.items() if "topicdist_" in k}
    # stats, stats_sum, product<0>, product<1>, product<2>, js, finish
    assert len(mine) == 7, sorted(mine)
    assert sum("product" in k for k in mine) == 3
    for name, f in mine.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_spill_count"] == 0, (name, f)
        assert f["sgpr_spill_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] <= 64 * 1024, (name, f)
