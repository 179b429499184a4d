"""CPU checks of the held-out predictive log-likelihood: the restatement's known answers,
trlda_amd.utils.split_documents, and the library's new entry point and kernel."""
import numpy as np
import pytest

import heldout_host


def _csr(rng, B, V, mean):
    n = rng.poisson(mean, size=B)
    indptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return indptr, rng.randint(0, V, size=indptr[-1]), rng.randint(1, 6, size=indptr[-1])


@pytest.mark.parametrize("K", [1, 5])
def test_identical_topics_give_the_unigram_score(K):
    rng = np.random.RandomState(K)
    V, B = 300, 20
    row = rng.gamma(0.5, 1.0, size=V) + 1e-3
    lam = np.tile(row, (K, 1))
    gamma = rng.gamma(1.0, 3.0, size=(K, B))          # any gamma
    indptr, ids, cnts = _csr(rng, B, V, 15)
    loglik, tokens = heldout_host.score(indptr, ids, cnts, gamma, lam)
    doc = np.repeat(np.arange(B), np.diff(indptr))
    want = np.bincount(doc, weights=cnts * np.log(row[ids] / row.sum()), minlength=B)
    assert np.allclose(loglik, want, rtol=1e-12, atol=0)
    assert np.array_equal(tokens, np.bincount(doc, weights=cnts, minlength=B))


def test_restatement_edge_cases():
    lam = np.array([[1.0, 3.0], [2.0, 2.0]])
    gamma = np.array([[1.0, 5.0, 2.0], [3.0, 5.0, 2.0]])
    indptr, ids, cnts = [0, 0, 3, 5], [0, 1, 1, 1, 0], [2, 0, 1, 4, 0]
    loglik, tokens = heldout_host.score(indptr, ids, cnts, gamma, lam)
    assert loglik[0] == 0 and tokens[0] == 0                     # no entries
    p0 = 0.5 * 0.25 + 0.5 * 0.5
    p1 = 0.5 * 0.75 + 0.5 * 0.5
    assert np.isclose(loglik[1], 2 * np.log(p0) + np.log(p1), rtol=1e-14)
    assert tokens[1] == 3
    assert np.isclose(loglik[2], 4 * np.log(p1), rtol=1e-14)     # zero count, duplicate id
    assert tokens[2] == 4


# -- split_documents ------------------------------------------------------------------------------
def _corpus(seed=3, B=400, V=500):
    from trlda_amd.documents import CSRDocuments
    rng = np.random.RandomState(seed)
    indptr, ids, cnts = _csr(rng, B, V, 30)
    cnts = rng.randint(1, 20, size=len(ids))
    return CSRDocuments(indptr, ids, cnts)


def _dense(docs, B, V):
    from trlda_amd.documents import as_csr
    c = as_csr(docs)
    out = np.zeros((B, V), dtype=np.int64)
    np.add.at(out, (np.repeat(np.arange(B), np.diff(c.indptr)), c.ids), c.cnts)
    return out


def test_split_keeps_every_token():
    import trlda_amd
    from trlda_amd.documents import as_csr
    from trlda_amd.utils import split_documents
    csr = _corpus()
    trlda_amd.seed(11)
    obs, held = split_documents(csr, 0.3)
    assert len(obs) == len(held) == len(csr)
    B, V = len(csr), 500
    assert np.array_equal(_dense(obs, B, V) + _dense(held, B, V), _dense(csr, B, V))
    for part in (obs, held):
        c = as_csr(part)
        assert (c.cnts > 0).all()
        # entry order kept: each part's entries are a subsequence of the input's
        for d in (0, 7, 99):
            src = list(csr.ids[csr.indptr[d]:csr.indptr[d + 1]])
            got = list(c.ids[c.indptr[d]:c.indptr[d + 1]])
            it = iter(src)
            assert all(w in it for w in got)


def test_split_fraction_follows_the_binomial_law():
    import trlda_amd
    from trlda_amd.documents import as_csr
    from trlda_amd.utils import split_documents
    from trlda_amd.documents import CSRDocuments
    n = 100000
    rng = np.random.RandomState(5)
    ids = rng.randint(0, 1000, size=n)
    csr = CSRDocuments(np.arange(0, n + 1, 100), ids, np.ones(n))
    for q in (0.05, 0.2, 0.5):
        trlda_amd.seed(21)
        _, held = split_documents(csr, q)
        got = int(as_csr(held).cnts.sum())
        assert abs(got - q * n) < 5 * np.sqrt(n * q * (1 - q)), (q, got)


def test_split_extremes():
    from trlda_amd.documents import as_csr
    from trlda_amd.utils import split_documents
    csr = _corpus(B=50)
    for q, full in ((0.0, 0), (1.0, 1)):
        parts = split_documents(csr, q)
        c, e = as_csr(parts[full]), as_csr(parts[1 - full])
        assert np.array_equal(c.indptr, csr.indptr)
        assert np.array_equal(c.ids, csr.ids) and np.array_equal(c.cnts, csr.cnts)
        assert len(parts[1 - full]) == 50 and e.indptr[-1] == 0


def test_split_is_reproducible_under_seed():
    import trlda_amd
    from trlda_amd.documents import as_csr
    from trlda_amd.utils import split_documents
    csr = _corpus()
    trlda_amd.seed(99)
    a = as_csr(split_documents(csr, 0.2)[1])
    b = as_csr(split_documents(csr, 0.2)[1])                # the stream moved on
    trlda_amd.seed(99)
    c = as_csr(split_documents(csr, 0.2)[1])
    assert np.array_equal(a.cnts, c.cnts) and np.array_equal(a.ids, c.ids)
    assert not (len(a.ids) == len(b.ids) and np.array_equal(a.cnts, b.cnts))


def test_split_accepts_lists_document_lists_and_csr():
    import trlda_amd
    from trlda_amd.documents import DocumentList, as_csr
    from trlda_amd.utils import split_documents
    csr = _corpus(B=60)
    lists = csr.to_list()
    results = []
    for docs in (lists, DocumentList(csr), csr):
        trlda_amd.seed(4)
        obs, held = split_documents(docs, 0.4)
        results.append((as_csr(obs), as_csr(held)))
    for o, h in results[1:]:
        for x, y in ((o, results[0][0]), (h, results[0][1])):
            assert np.array_equal(x.indptr, y.indptr) and np.array_equal(x.ids, y.ids)
            assert np.array_equal(x.cnts, y.cnts)
    obs, held = split_documents([[], [(3, 1)]], 0.5)
    assert len(obs) == len(held) == 2 and obs[0] == [] and held[0] == []


def test_split_rejects_bad_arguments():
    from trlda_amd.utils import split_documents
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            split_documents([[(0, 1)]], q)
    with pytest.raises(TypeError):
        split_documents("not documents", 0.2)
    with pytest.raises(TypeError):
        split_documents([[(0, 1.5)]], 0.2)
    with pytest.raises(ValueError):
        split_documents([[(0, -2)]], 0.2)


def test_split_is_not_on_the_reference_surface():
    import trlda.utils
    assert not hasattr(trlda.utils, "split_documents")


# -- the library ----------------------------------------------------------------------------------
def test_predictive_entry_point_is_exported(hip_lib):
    from trlda_amd import _ffi
    assert "trlda_model_predictive" in _ffi.EXPORTED_SYMBOLS
    assert hasattr(hip_lib, "trlda_model_predictive")
    # (no model: the argument check answers before any device is touched)
    rc = hip_lib.trlda_model_predictive(None, None, None, np.zeros(1), 10, 1e-3, np.zeros(1), np.zeros(1))
    assert rc == _ffi.ERR_ARG


def test_heldout_kernel_uses_no_scratch(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    held = {k: v for k, v in res.items() if "heldout_docs_kernel" in k}
    assert len(held) == 1, sorted(held)
    for name, f in held.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["vgpr_count"] <= 128, (name, f)
