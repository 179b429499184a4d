"""CPU checks of the per-word topic posteriors: the restatement (tests/wordtopics_host.py) against a
literal triple loop, its rows, tie order and gap report, and the library's new entry points and
kernel."""
import numpy as np
from scipy.special import psi

import wordtopics_host


LAM = np.array([[0.7, 2.0, 0.3, 1.1, 4.0],
                [1.5, 0.2, 2.5, 0.9, 0.4],
                [0.6, 0.6, 1.0, 3.0, 0.8]])
GAMMA = np.array([[0.9, 2.5],
                  [3.1, 0.4],
                  [1.2, 1.7]])
INDPTR, IDS, CNTS = [0, 3, 7], [4, 0, 2, 1, 1, 3, 0], [2, 1, 0, 5, 1, 1, 3]


def test_against_the_triple_loop():
    K, V = LAM.shape
    phi = wordtopics_host.posterior(INDPTR, IDS, GAMMA, LAM)
    assert phi.shape == (7, K)
    p = 0
    for d in range(2):
        for j in range(INDPTR[d], INDPTR[d + 1]):
            s = []
            for k in range(K):
                rs = sum(LAM[k, v] for v in range(V))
                s.append(np.exp(psi(GAMMA[k, d]) - psi(rs)) * np.exp(psi(LAM[k, IDS[j]])))
            z = sum(s)
            for k in range(K):
                assert abs(phi[p, k] - s[k] / z) <= 4e-16 * s[k] / z
            p += 1
    # the counts play no part: entries 3 and 4 are the same word of the same document
    assert np.array_equal(phi[3], phi[4])


def test_rows_sum_to_one_and_are_ranked():
    K = LAM.shape[0]
    phi, topics, probs, gap = wordtopics_host.word_topics(INDPTR, IDS, GAMMA, LAM, K)
    assert topics.dtype == np.int32 and topics.shape == probs.shape == (7, K)
    assert np.all(np.abs(probs.sum(axis=1) - 1) <= 4 * K * np.finfo(float).eps)
    assert np.all(np.diff(probs, axis=1) <= 0)
    assert np.array_equal(np.sort(topics, axis=1), np.tile(np.arange(K), (7, 1)))
    assert np.array_equal(np.take_along_axis(phi, topics.astype(np.int64), axis=1), probs)
    _, t1, p1, _ = wordtopics_host.word_topics(INDPTR, IDS, GAMMA, LAM, 1)
    assert np.array_equal(t1[:, 0], np.argmax(phi, axis=1)) and np.array_equal(p1, probs[:, :1])


def test_equal_values_go_by_smaller_id():
    phi = np.array([[0.25, 0.5, 0.25, 0.0],
                    [0.25, 0.25, 0.25, 0.25],
                    [0.1, 0.2, 0.3, 0.4]])
    assert np.array_equal(wordtopics_host.rank(phi), [[1, 0, 2, 3], [0, 1, 2, 3], [3, 2, 1, 0]])
    # two topics with identical lambda rows and identical gamma: the same phi, the smaller id first
    lam = LAM[[0, 1, 0]]
    gamma = GAMMA[[0, 1, 0]]
    _, topics, probs, gap = wordtopics_host.word_topics(INDPTR, IDS, gamma, lam, 3)
    for p in range(7):
        at0, at2 = list(topics[p]).index(0), list(topics[p]).index(2)
        assert at2 == at0 + 1 and probs[p, at0] == probs[p, at2]
    assert np.all(gap == 0)


def test_gap_report():
    ranked = np.array([[0.5, 0.25, 0.125, 0.125],
                       [0.4, 0.4, 0.1, 0.1],
                       [0.625, 0.125, 0.125, 0.125]])
    assert np.array_equal(wordtopics_host.gaps(ranked, 1), [0.5, 0.0, 0.8])
    assert np.array_equal(wordtopics_host.gaps(ranked, 2), [0.5, 0.0, 0.0])
    assert np.array_equal(wordtopics_host.gaps(ranked, 3), [0.0, 0.0, 0.0])
    assert np.array_equal(wordtopics_host.gaps(ranked, 4), wordtopics_host.gaps(ranked, 3))   # all K
    assert np.all(np.isinf(wordtopics_host.gaps(ranked[:, :1], 1)))
    # the report of word_topics is that of its own ranked rows
    phi, _, _, gap = wordtopics_host.word_topics(INDPTR, IDS, GAMMA, LAM, 1)
    top2 = -np.sort(-phi, axis=1)[:, :2]
    assert np.array_equal(gap, (top2[:, 0] - top2[:, 1]) / top2[:, 0]) and np.all(gap > 0)


# -- the library ----------------------------------------------------------------------------------
def test_word_topics_entry_points_are_exported(hip_lib):
    from trlda_amd import _ffi
    from trlda_amd.models import LDA
    for name in ("trlda_model_word_topics", "trlda_model_word_topics_dev"):
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    # (no model: the argument check answers before any device is touched)
    assert hip_lib.trlda_model_word_topics(None, None, None, 1, 10, 1e-3, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_model_word_topics_dev(None, None, None, 1, None, None) == _ffi.ERR_ARG
    assert callable(LDA.word_topics)


def test_word_topics_kernel_does_not_spill(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    mine = {k: v for k, v in res.items() if "word_topics_kernel" in k}
    assert len(mine) == 9, sorted(mine)                          # KPL = 1 .. 8 and the form that keeps nothing
    for name, f in mine.items():
        # (16 bytes: the frame of psi.h's out-of-line rare branch, as in exp_elog_beta_kernel)
        assert f["private_segment_fixed_size"] <= 16, (name, f)
        assert f["vgpr_spill_count"] == 0, (name, f)
        assert f["vgpr_count"] <= 128, (name, f)                 # four waves per SIMD
        assert f["group_segment_fixed_size"] == 0, (name, f)     # the K factors are the only LDS, all dynamic
