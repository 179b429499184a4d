"""CPU checks of topic coherence: the restatement's known answers and conventions, the library's
host arithmetic on given counts, and the library's new entry points and kernels."""
import math

import numpy as np
import pytest

import coherence_host as ch

# five documents over V = 6 (d3 empty): D(0) = D(1) = 3, D(2) = D(3) = 2, D(0,1) = D(1,2) = 2,
# D(0,2) = D(0,3) = D(1,3) = D(2,3) = 1, M = 5
HAND = ([0, 3, 5, 7, 7, 10], [0, 1, 2, 0, 1, 0, 3, 1, 2, 3], [1] * 10)


def _hand(words):
    return ch.counts(ch.presence(*HAND, V=6), words)


def test_hand_computed_values():
    df, co, M = _hand([[0, 1, 2], [3, 0, 1]])
    assert M == 5
    assert df.tolist() == [[3, 3, 2], [2, 3, 3]]
    assert co[0].tolist() == [[3, 2, 1], [2, 3, 2], [1, 2, 2]]
    # UMass: log((D(v_m, v_l) + 1) / D(v_l)) over (m, l) = (1, 0), (2, 0), (2, 1)
    assert ch.umass(df, co)[0] == pytest.approx((0 + math.log(2 / 3) + 0) / 3, rel=1e-14)
    assert ch.umass(df, co)[1] == 0.0
    want0 = (math.log(10 / 9) / math.log(5 / 2) + math.log(5 / 6) / math.log(5)
             + math.log(5 / 3) / math.log(5 / 2)) / 3
    want1 = (2 * math.log(5 / 6) / math.log(5) + math.log(10 / 9) / math.log(5 / 2)) / 3
    npmi = ch.npmi(df, co, M)
    assert npmi[0] == pytest.approx(want0, rel=1e-14)
    assert npmi[1] == pytest.approx(want1, rel=1e-14)
    assert npmi[0] == pytest.approx(0.18639870, abs=1e-8)
    assert npmi[1] == pytest.approx(-0.03719320, abs=1e-8)


def test_npmi_extremes():
    # words 4 and 5 never meet: -1; words 0 and 1 in every document: +1
    indptr, ids = [0, 3, 6, 8], [0, 1, 4, 0, 1, 5, 1, 0]
    P = ch.presence(indptr, ids, np.ones(len(ids)), 6)
    df, co, M = ch.counts(P, [[4, 5], [0, 1]])
    assert ch.npmi(df, co, M).tolist() == [-1.0, 1.0]


def test_umass_drops_pairs_of_absent_words():
    df, co, M = _hand([[5, 0, 1]])
    assert ch.umass(df, co)[0] == math.log((2 + 1) / 3)   # only (m, l) = (2, 1) is left
    df, co, M = _hand([[5, 0], [4, 5]])
    u = ch.umass(df, co)
    assert math.isnan(u[0]) and math.isnan(u[1])          # no pair left
    assert ch.npmi(df, co, M).tolist() == [-1.0, -1.0]


def test_duplicates_and_non_positive_counts_create_no_presence():
    indptr = [0, 3, 6]
    ids = [0, 0, 1, 2, 3, 0]
    cnts = [2, 3, 0, 1, -1, 0]
    P = ch.presence(indptr, ids, cnts, 4)
    assert P.tolist() == [[True, False, False, False], [False, False, True, False]]


def test_empty_documents_count_in_m():
    base = ch.counts(ch.presence(*HAND, V=6), [[0, 1, 2]])
    more = ch.presence(HAND[0] + [10, 10], HAND[1], HAND[2], 6)
    grown = ch.counts(more, [[0, 1, 2]])
    assert grown[2] == base[2] + 2
    assert np.array_equal(grown[0], base[0]) and np.array_equal(grown[1], base[1])
    assert ch.npmi(*grown)[0] != ch.npmi(*base)[0]
    assert ch.umass(grown[0], grown[1])[0] == ch.umass(base[0], base[1])[0]


def test_top_words_restatement_breaks_ties_by_id():
    lam = np.array([[1.0, 3.0, 3.0, 2.0, np.nan], [0.0, -0.0, 5.0, -1.0, 5.0]])
    assert ch.top_words(lam, 5).tolist() == [[1, 2, 3, 0, 4], [2, 4, 0, 1, 3]]


@pytest.mark.parametrize("measure", ["umass", "npmi"])
def test_library_host_arithmetic_matches_the_restatement(measure):
    from trlda_amd.models import _coherence
    rng = np.random.RandomState(3)
    B, V = 300, 40
    P = rng.rand(B, V) < rng.rand(V) * 0.5
    P[:, 7] = False                                   # an absent word
    P[:, 8] = True                                    # a word in every document
    words = np.stack([rng.permutation(V)[:12] for _ in range(9)])
    words[0, :3] = [7, 8, 1]
    df, co, M = ch.counts(P, words)
    got = _coherence(measure, df, co, M)
    want = ch.coherence(measure, df, co, M)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=1e-12, atol=0)


def test_library_host_arithmetic_conventions():
    from trlda_amd.models import _coherence
    df, co, M = _hand([[5, 0], [4, 5]])
    u = _coherence("umass", df, co, M)
    assert math.isnan(u[0]) and math.isnan(u[1])
    assert _coherence("npmi", df, co, M).tolist() == [-1.0, -1.0]
    df, co, M = _hand([[5, 0, 1]])
    assert _coherence("umass", df, co, M)[0] == math.log(1.0)


def test_coherence_methods_are_on_every_model():
    from trlda_amd.models import LDA, OnlineLDA, BatchLDA, CumulativeLDA
    import trlda.models
    for cls in (OnlineLDA, BatchLDA, CumulativeLDA, trlda.models.OnlineLDA):
        assert cls.top_words is LDA.top_words
        assert cls.topic_coherence is LDA.topic_coherence


# -- the library ----------------------------------------------------------------------------------
NEW = ("trlda_model_top_words", "trlda_cooc_create", "trlda_cooc_add", "trlda_cooc_read",
       "trlda_cooc_destroy")


def test_coherence_entry_points_are_exported(hip_lib):
    import ctypes as C
    from trlda_amd import _ffi
    for name in NEW:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
    # (no model: the argument checks answer before any device is touched)
    assert hip_lib.trlda_model_top_words(None, 5, np.zeros(5, dtype=np.int32)) == _ffi.ERR_ARG
    out = _ffi.vp()
    words = np.arange(4, dtype=np.int32)
    assert hip_lib.trlda_cooc_create(None, words, 2, 2, C.byref(out)) == _ffi.ERR_ARG
    assert not out.value
    assert hip_lib.trlda_cooc_add(None, None) == _ffi.ERR_ARG
    n = C.c_int64(0)
    assert hip_lib.trlda_cooc_read(None, np.zeros(4, dtype=np.int64), np.zeros(8, dtype=np.int64),
                                   C.byref(n)) == _ffi.ERR_ARG
    assert hip_lib.trlda_cooc_destroy(None) == _ffi.OK


def test_coherence_kernels_use_no_scratch(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    names = ("topn_tile_kernel", "topn_merge_kernel", "cooc_bits_kernel", "cooc_df_kernel",
             "cooc_pairs_kernel")
    for kern in names:
        found = {k: v for k, v in res.items() if kern in k}
        assert len(found) == 1, (kern, sorted(found))
        for name, f in found.items():
            assert f["private_segment_fixed_size"] == 0, (name, f)
            assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
            assert f["vgpr_count"] <= 96, (name, f)
