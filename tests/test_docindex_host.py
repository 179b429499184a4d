"""CPU checks of the document index: the restatement (tests/docindex_host.py) against brute-force
definitions on a 5-document K = 3 case, its tie order and near-tie report, and what the library and
``DocumentIndex`` answer before any GPU work."""
import numpy as np
import pytest

import docindex_host as dh

# five documents, K = 3 (columns are documents); document 3 is twice document 0, so theta_3 = theta_0
GAMMA = np.array([[1.0, 0.5, 4.0, 2.0, 0.2],
                  [2.0, 0.5, 1.0, 4.0, 0.2],
                  [1.0, 3.0, 1.0, 2.0, 3.6]])
THETA = GAMMA / GAMMA.sum(axis=0)


def test_theta_by_hand():
    assert np.allclose(THETA[:, 0], [0.25, 0.5, 0.25], rtol=0, atol=1e-16)
    assert np.allclose(THETA[:, 1], [0.125, 0.125, 0.75], rtol=0, atol=1e-16)
    assert np.allclose(THETA[:, 4], [0.05, 0.05, 0.9], rtol=0, atol=1e-16)
    assert np.array_equal(THETA[:, 3], THETA[:, 0])


def test_hellinger_against_the_definition():
    """Hellinger^2 = 1/2 sum (sqrt p - sqrt q)^2 = 1 - s."""
    r = dh.rows(GAMMA, "hellinger")
    assert r.shape == (5, 3)
    s = dh.similarities(r, r)
    for a in range(5):
        for b in range(5):
            h2 = 0.5 * sum((np.sqrt(THETA[k, a]) - np.sqrt(THETA[k, b])) ** 2 for k in range(3))
            assert abs(float(s[a, b]) - (1.0 - h2)) <= 4e-16
            assert abs(dh.distance(s, "hellinger")[a, b] ** 2 - h2) <= 4e-16
    # by hand: documents 0 and 1: sqrt(1/32) + sqrt(1/16) + sqrt(3/16)
    assert abs(float(s[0, 1]) - (np.sqrt(1 / 32.) + 0.25 + np.sqrt(3.) / 4)) <= 4e-16
    assert np.all(np.abs(np.diag(s).astype(np.float64) - 1) <= 4e-16)


def test_cosine_against_the_definition():
    r = dh.rows(GAMMA, "cosine")
    s = dh.similarities(r, r)
    for a in range(5):
        for b in range(5):
            want = np.dot(THETA[:, a], THETA[:, b]) / (np.linalg.norm(THETA[:, a]) * np.linalg.norm(THETA[:, b]))
            assert abs(float(s[a, b]) - want) <= 4e-16
            assert abs(dh.distance(s, "cosine")[a, b] - max(0.0, 1 - want)) <= 4e-16
    # by hand: documents 0 and 2: (1/4 * 2/3 + 1/2 * 1/6 + 1/4 * 1/6) / (sqrt(3/8) sqrt(1/2))
    assert abs(float(s[0, 2]) - (7. / 24) / np.sqrt(3. / 16)) <= 4e-16
    with pytest.raises(ValueError):
        dh.rows(GAMMA, "manhattan")


def test_equal_values_go_by_smaller_id():
    s = np.array([[0.25, 0.5, 0.25, 0.0],
                  [0.25, 0.25, 0.25, 0.25],
                  [0.1, 0.2, 0.3, 0.4]])
    assert np.array_equal(dh.rank(s), [[1, 0, 2, 3], [0, 1, 2, 3], [3, 2, 1, 0]])
    # documents 0 and 3 have the same theta: the same rows, the same s, the smaller id first
    for measure in ("hellinger", "cosine"):
        r = dh.rows(GAMMA, measure)
        assert np.array_equal(r[0], r[3])
        ids, s_top, gap = dh.search(r, r, 5)
        for q in range(5):
            at0, at3 = list(ids[q]).index(0), list(ids[q]).index(3)
            assert at3 == at0 + 1 and s_top[q, at0] == s_top[q, at3]
        assert np.all(gap == 0)
        assert ids[0, 0] == 0 and ids[3, 0] == 0 and ids[1, 0] == 1       # itself, or its smallest duplicate


def test_gap_report():
    ranked = np.array([[0.5, 0.25, 0.125, 0.125],
                       [0.5, 0.5, 0.25, 0.125],
                       [1.0, 0.5, 0.375, 0.25]])
    assert np.array_equal(dh.gaps(ranked, 1), [0.25, 0.0, 0.5])
    assert np.array_equal(dh.gaps(ranked, 2), [0.125, 0.0, 0.125])
    assert np.array_equal(dh.gaps(ranked, 3), [0.0, 0.0, 0.125])
    assert np.array_equal(dh.gaps(ranked, 4), dh.gaps(ranked, 3))           # all N
    assert np.all(np.isinf(dh.gaps(ranked[:, :1], 1)))
    # the report of search is that of its own ranked similarities
    r = dh.rows(GAMMA[:, [0, 1, 2, 4]], "hellinger")
    ids, s_top, gap = dh.search(r, r, 1)
    full = -np.sort(-dh.similarities(r, r).astype(np.float64), axis=1)
    assert np.allclose(gap, full[:, 0] - full[:, 1], rtol=0, atol=1e-16) and np.all(gap > 0)
    assert np.array_equal(ids[:, 0], np.arange(4))


# -- the library ----------------------------------------------------------------------------------
def test_measure_errors_come_before_any_gpu_work():
    """The measure is checked first: a wrong one raises on a machine without a GPU, and with a
    model that would not do either."""
    import trlda_amd
    from trlda_amd import DocumentIndex
    from trlda_amd.models import LDA
    assert trlda_amd.DocumentIndex is DocumentIndex and callable(LDA.document_index)
    with pytest.raises(ValueError):
        DocumentIndex(None, measure="jensen-shannon")
    with pytest.raises(ValueError):
        DocumentIndex(None, measure="")
    for bad in (None, 0, b"cosine", ["hellinger"]):
        with pytest.raises(TypeError):
            DocumentIndex(None, measure=bad)
    # (LDA.document_index hands the measure on before it looks at the model)
    m = LDA.__new__(LDA)
    m._handle = None
    with pytest.raises(ValueError):
        m.document_index("euclid")
    with pytest.raises(TypeError):
        m.document_index(3)
    from trlda_amd.index import _measure
    assert _measure("Hellinger") == _measure("HELLINGER") == 0 and _measure("CoSine") == 1
    import trlda_amd.models
    assert not hasattr(trlda_amd.models, "DocumentIndex")


def test_docindex_entry_points_are_exported(hip_lib):
    from trlda_amd import _ffi
    names = ["trlda_docindex_" + n for n in ("create", "reserve", "add", "add_gamma", "add_gamma_dev", "size",
                                             "query", "query_gamma", "read_rows", "set_slab_rows", "destroy")]
    for name in names:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
    # (no index: the argument check answers before any device is touched)
    assert hip_lib.trlda_docindex_add(None, None, None, 10, 1e-3) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_add_gamma(None, None, 1) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_add_gamma_dev(None, None, 1) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_query(None, None, None, 10, 1e-3, 1, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_query_gamma(None, None, 1, 1, None, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_read_rows(None, 0, 0, None) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_reserve(None, 1) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_set_slab_rows(None, 16) == _ffi.ERR_ARG
    assert hip_lib.trlda_docindex_size(None) == 0
    assert hip_lib.trlda_docindex_destroy(None) == _ffi.OK


def test_docindex_kernels_do_not_spill(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    mine = {k: v for k, v in res.items() if "docindex_" in k}
    assert len(mine) == 4, sorted(mine)                  # rows, query<1>, query<2>, merge
    for name, f in mine.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_spill_count"] == 0, (name, f)
        if "query" in name:
            assert f["vgpr_count"] <= 256, (name, f)     # two waves per SIMD
