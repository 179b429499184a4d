"""Spectral initialisation on the GPU (csrc/anchor_kernels.h) against the restatement
of tests/anchor_host.py: the co-occurrence matrix bit for bit, however the corpus is cut; the anchor
words on planted and sampled inputs; the recovered simplex weights by their constraints and their
Frank-Wolfe gap in longdouble; planted recovery; a word's independence of the others; both places
the solver reads G from; initialize_spectral; the error paths; the buffers."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import anchor_host as ah
from test_anchor_host import GPU_PLANTED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    return _ffi.lib()


def _model(K, V):
    from trlda_amd.models import OnlineLDA
    return OnlineLDA(num_words=V, num_topics=K, num_documents=1000, alpha=.1, eta=.3, device=0)


def _corpus(B, V, seed, mean_unique=8, lengths=None):
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.utils.synthetic import make_corpus
    return CSRDocuments(*make_corpus(B, V, seed=seed, mean_unique=mean_unique, lengths=lengths))


def _cuts(csr, size):
    return [csr.slice(lo, min(lo + size, len(csr))) for lo in range(0, len(csr), size)]


def _check_counts(cooc, want):
    Q, df, wc, docs, skipped, tokens = want
    got = cooc.read()
    assert np.array_equal(got, Q)                              # bit for bit
    assert np.array_equal(got, got.T)
    # (an element is a sum of at most `docs` quotients: gamma(docs + 1) of the whole)
    assert abs(math.fsum(got.ravel()) - docs) <= ah.gamma(docs + 1) * docs
    assert np.array_equal(cooc.doc_freq, df) and np.array_equal(cooc.word_count, wc)
    assert (cooc.num_documents, cooc.num_skipped, cooc.num_tokens) == (docs, skipped, tokens)


# ---- 1. the matrix ----------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [40, 37])                        # (37: the rows' stride is 40, the tail zero)
def test_q_equals_the_plain_loop_however_the_corpus_is_cut(hip, V):
    rng = np.random.RandomState(V)
    lengths = 1 + rng.poisson(7, size=64)
    lengths[5], lengths[17] = 1, 0                             # a one-word and an empty document
    csr = _corpus(64, V, seed=V, lengths=lengths)
    csr.cnts[csr.indptr[5]] = 1
    want = ah.cooccurrence([csr], V)
    assert want[4] == 2 and want[3] == 62
    model = _model(4, V)
    for size in (64, 1, 7):
        cooc = model.word_cooccurrence(iter(_cuts(csr, size)))
        _check_counts(cooc, want)
        cooc.close()
    cooc = model.word_cooccurrence(csr)                         # a batch, not an iterator
    _check_counts(cooc, want)
    rows = np.array([V - 1, 0, 3])
    assert np.array_equal(cooc.read(rows), want[0][rows])
    # the row sums and the probabilities, in the documented order
    r, total = cooc.row_sums()
    r_want, total_want = ah.row_sums(want[0])
    assert np.array_equal(r, r_want) and total == total_want
    assert np.array_equal(cooc.word_probabilities(), r_want / total_want)
    model.close()


def test_a_word_in_every_document(hip):
    """Word 0 lies in all 300 documents of one batch: its list is longer than both thresholds of the
    word-major index (16 entries: a long list; 256: a very long one, cut into segments).  The row
    kernel has no threshold of its own -- it walks a list entry by entry whatever its length -- so
    the long list must come out like any other."""
    from trlda_amd.documents import CSRDocuments
    V, B = 30, 300
    csr = _corpus(B, V, seed=3, mean_unique=5)
    ids, cnts, indptr = [], [], [0]
    for d in range(B):
        w = csr.ids[csr.indptr[d]:csr.indptr[d + 1]]
        c = csr.cnts[csr.indptr[d]:csr.indptr[d + 1]]
        keep = w != 0
        ids += [0] + list(w[keep])
        cnts += [2 + d % 3] + list(c[keep])                 # (n >= 2: every document contributes)
        indptr.append(len(ids))
    csr = CSRDocuments(indptr, ids, cnts)
    model = _model(4, V)
    batch = model.upload(csr)
    assert hip.trlda_batch_num_long_words(batch.handle) >= 1
    assert hip.trlda_batch_num_very_long_words(batch.handle) >= 1
    cooc = model.word_cooccurrence(batch)
    want = ah.cooccurrence([csr], V)
    assert want[1][0] == B
    _check_counts(cooc, want)
    model.close()


# ---- 2. the anchors ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    """per (K, V): Q, beta, the planted anchors, the float64 restatement's selection"""
    out = {}
    for K, V in GPU_PLANTED:
        Q, beta, anchors = ah.planted(K, V)
        out[K, V] = (Q, beta, anchors, ah.anchor_words(Q, K))
    return out


@pytest.mark.parametrize("K,V", GPU_PLANTED[:2])
def test_planted_anchors_and_scores(hip, planted, K, V):
    from trlda_amd import WordCooccurrence
    Q, _, anchors, (ids, _, _, _) = planted[K, V]
    model = _model(K, V)
    cooc = WordCooccurrence.from_matrix(model, Q)
    assert np.array_equal(cooc.read(), Q)
    got, scores = model.anchor_words(cooc, return_scores=True)
    assert got.dtype == np.int32 and np.array_equal(got, ids) and sorted(got) == sorted(anchors)
    assert np.array_equal(model.anchor_words(cooc), got)       # the work copy is made anew
    _, s_ld, r_ld, bound = ah.anchor_words(Q, K, dtype=np.longdouble)
    # the winner's and the runner-up's norm^2 of every round, each within the bound of its own row
    for name, want, bd in (("winner", s_ld, bound[0]), ("runner_up", r_ld, bound[1])):
        err = np.abs(scores[name].astype(np.longdouble) - want)
        print("K=%d: %s errors / bound, largest %.3g" % (K, name, float(np.max(err / bd))))
        assert np.isfinite(bd).all() and (err <= bd).all()
    assert (scores["runner_up"] <= scores["winner"]).all()
    model.close()


def test_anchors_of_a_sampled_corpus(hip):
    K, V = 6, 120
    csr = _corpus(400, V, seed=11, mean_unique=25)
    Q, df, _, docs, _, _ = ah.cooccurrence([csr], V)
    model = _model(K, V)
    cooc = model.word_cooccurrence(iter(_cuts(csr, 150)))
    assert np.array_equal(cooc.read(), Q)
    min_df = ah.default_min_doc_freq(docs)
    assert min_df == 2 and (df >= min_df).sum() >= K
    ids, score, runner, _ = ah.anchor_words(Q, K, candidates=df >= min_df)
    ties = ah.near_ties(score, runner)
    print("sampled corpus: near-ties %r" % (ties,))
    upto = ties[0][0] if ties else K                           # (from a near-tie on either word may win)
    got = model.anchor_words(cooc)
    assert np.array_equal(got[:upto], ids[:upto])
    # a threshold that leaves other candidates
    strict = int(np.sort(df)[-40])
    ids2 = ah.anchor_words(Q, K, candidates=df >= strict)[0]
    assert np.array_equal(model.anchor_words(cooc, min_doc_freq=strict), ids2) and (df[ids2] >= strict).all()
    model.close()


# ---- 3. the recovery --------------------------------------------------------------------------------

def _check_solution(Q, anchors, x, info, tol, max_iter, dtype=np.longdouble, slack=1):
    """the constraints and the gap of the device's x, recomputed from the restatement's rows"""
    K = len(anchors)
    r, _ = ah.row_sums(Q)
    W = ah.normalise(Q, r)
    assert (x >= 0).all()
    sums = np.array([math.fsum(row) for row in x])
    assert np.abs(sums - 1).max() <= K * 2.0 ** -52
    Wd = W.astype(dtype)
    H, G = ah.products(Wd, anchors)
    qq = (Wd * Wd).sum(axis=1)
    gap = ah.gap_of(x.astype(dtype), G, H) / np.where(qq > 0, qq, 1)
    allow = slack * ah.gap_allowance(W, anchors, tol)
    done = info["iterations"] < max_iter
    print("K=%d: iterations <= %d, relative gap <= %.3g (allowance %.3g)" %
          (K, info["iterations"].max(), float(gap.max()), float(allow.max())))
    assert (gap[done & (qq > 0)] <= tol + allow[done & (qq > 0)]).all()
    assert (info["gaps"][done] <= tol).all()
    return W, done


@pytest.mark.parametrize("K,V", GPU_PLANTED[:2])
def test_recovered_weights(hip, planted, K, V):
    from trlda_amd import WordCooccurrence
    Q, _, _, (ids, _, _, _) = planted[K, V]
    model = _model(K, V)
    cooc = WordCooccurrence.from_matrix(model, Q)
    beta, pi, info = model.recover_topics(cooc, ids, return_info=True)
    assert beta.shape == (K, V) and beta.flags.f_contiguous and pi.shape == (K,)
    W, done = _check_solution(Q, ids, info["x"], info, 1e-7, 2000)
    # max_iter is reached only where the restatement does not converge either
    _, it_host, _ = ah.recover(W.astype(np.longdouble), ids, 1e-7, 2000)
    assert done[it_host < 2000].all()
    # beta and pi from x: the rounded products x_wk p_w, their fixed-order sums, one division
    p = cooc.word_probabilities()
    M = info["x"] * p[:, None]
    pi_want = ah.fixed_sum(np.ascontiguousarray(M.T))
    assert np.array_equal(pi, pi_want) and np.array_equal(beta, (M / pi_want).T)
    assert abs(pi.sum() - 1) < 1e-13 and np.abs(beta.sum(axis=1) - 1).max() < 1e-13
    # without info: the same
    b2, p2 = model.recover_topics(cooc, ids)
    assert np.array_equal(b2, beta) and np.array_equal(p2, pi)
    model.close()


@pytest.mark.parametrize("K,V", GPU_PLANTED[:2])
def test_planted_topics_are_recovered(hip, planted, K, V):
    """At tol = 1e-10 the device's beta lies within ten times the restatement's own total-variation
    distance to the planted beta (the margin covers the fp64 products against its longdouble ones).
    Measured: K = 5, V = 60: restatement 1.47e-07, device 1.47e-07; K = 20, V = 500: restatement
    1.54e-06, device 1.54e-06."""
    from trlda_amd import WordCooccurrence
    Q, beta_true, anchors, (ids, _, _, _) = planted[K, V]
    r, total = ah.row_sums(Q)
    X, it_host, _ = ah.recover(ah.normalise(Q, r).astype(np.longdouble), ids, 1e-10, 5000)
    host = ah.total_variation(ah.topics_of(X, (r / total).astype(np.longdouble))[0], beta_true, ids, anchors)
    model = _model(K, V)
    cooc = WordCooccurrence.from_matrix(model, Q)
    got = model.anchor_words(cooc)
    beta, _, info = model.recover_topics(cooc, got, tol=1e-10, max_iter=5000, return_info=True)
    dev = ah.total_variation(beta, beta_true, got, anchors)
    print("K=%d V=%d: total variation to the planted beta: restatement %.3g, device %.3g" % (K, V, host, dev))
    assert it_host.max() < 5000 and info["iterations"].max() < 5000
    assert dev <= 10 * host
    model.close()


def test_a_word_depends_on_its_own_row_and_the_anchors_alone(hip, planted):
    """Entries (w1, w2) and (w2, w1) of Q between words that are neither anchors nor the words looked
    at leave those words' rows and the anchors' rows as they were: their x keeps every bit, with G in
    LDS and read from global memory -- the two launches the solver has.  (Their beta rows follow x
    through p_w and pi_k, which do move with the sum of Q: they are checked from x elsewhere.)"""
    from trlda_amd import WordCooccurrence
    K, V = GPU_PLANTED[1]
    Q, _, _, (ids, _, _, _) = planted[K, V]
    others = np.setdiff1d(np.arange(V), ids)
    w1, w2, kept = others[3], others[10], np.setdiff1d(np.arange(V), [others[3], others[10]])
    Q2 = Q.copy()
    Q2[w1, w2] = Q2[w2, w1] = 3 * Q[w1, w2] + 1e-4
    model = _model(K, V)
    runs = []
    for q in (Q, Q2):
        cooc = WordCooccurrence.from_matrix(model, q)
        for mode in (0, 1):
            cooc._set_gram_lds(mode)
            runs.append(model.recover_topics(cooc, ids, return_info=True))
        cooc.close()
    x0, it0 = runs[0][2]["x"], runs[0][2]["iterations"]
    assert np.array_equal(runs[1][2]["x"], x0) and np.array_equal(runs[1][0], runs[0][0])      # LDS / global
    assert np.array_equal(runs[1][2]["iterations"], it0) and np.array_equal(runs[1][1], runs[0][1])
    assert np.array_equal(runs[3][2]["x"], runs[2][2]["x"])
    for run in runs[2:]:
        assert np.array_equal(run[2]["x"][kept], x0[kept]) and np.array_equal(run[2]["iterations"][kept], it0[kept])
        assert not np.array_equal(run[2]["x"][[w1, w2]], x0[[w1, w2]])
    model.close()


def test_more_anchors_than_g_fits_in_lds(hip, planted):
    """K = 130 is past the 128 anchors up to which G lies in LDS: selection and solution as below it."""
    from trlda_amd import WordCooccurrence
    K, V = GPU_PLANTED[2]
    Q, _, anchors, (ids, _, _, _) = planted[K, V]
    model = _model(K, V)
    cooc = WordCooccurrence.from_matrix(model, Q)
    got = model.anchor_words(cooc)
    assert np.array_equal(got, ids) and sorted(got) == sorted(anchors)
    beta, pi, info = model.recover_topics(cooc, got, return_info=True)
    _check_solution(Q, got, info["x"], info, 1e-7, 2000)
    assert info["iterations"].max() < 2000 and np.isfinite(beta).all() and abs(pi.sum() - 1) < 1e-13
    model.close()


def test_512_anchors(hip):
    """K = 512, G read from global memory, the planted anchors given.  The planted alpha is scaled to
    0.002 (1 + k / K) so that its sum stays about 1.5 as at small K: with 0.1 the anchors' rows are all
    but one mixture and neither the restatement nor the device gets any word to 1e-7 in 2000 iterations.
    Here every word converges (the restatement's float64 solve: at most 1154 iterations), the start
    x = 1 / K has a relative gap of at least 0.6, and the solution is held by its constraints and its
    gap, recomputed in float64 (a longdouble product of this size takes minutes): the recomputation's
    own rounding is of the size the allowance grants the device, hence twice the allowance."""
    from trlda_amd import WordCooccurrence
    K, V = 512, 640
    Q, _, anchors = ah.planted(K, V, alpha_scale=0.002)
    model = _model(K, V)
    cooc = WordCooccurrence.from_matrix(model, Q)
    beta, pi, info = model.recover_topics(cooc, anchors, return_info=True)
    W, done = _check_solution(Q, anchors, info["x"], info, 1e-7, 2000, dtype=np.float64, slack=2)
    H, G = ah.products(W, anchors)
    start = ah.gap_of(np.full((V, K), 1.0 / K), G, H) / (W * W).sum(axis=1)
    assert start.min() > 0.5                                   # (the start is far from passing)
    _, it_host, _ = ah.recover(W, anchors, 1e-7, 2000)
    assert (it_host < 2000).all() and done[it_host < 2000].all() and done.sum() == V
    assert np.isfinite(beta).all() and abs(pi.sum() - 1) < 1e-13
    model.close()
    wide = _model(4, 700)
    with pytest.raises(RuntimeError, match="640"):                        # the solver's LDS ends there
        wide.recover_topics(WordCooccurrence.from_matrix(wide, np.eye(700)), np.arange(641))
    wide.close()


# ---- 4. initialize_spectral ---------------------------------------------------------------------------

def test_initialize_spectral_is_the_three_stages(hip):
    import trlda_amd
    K, V = 6, 120
    csr = _corpus(400, V, seed=11, mean_unique=25)
    trlda_amd.seed(5)
    model = _model(K, V)
    state = np.zeros(33, dtype=np.uint32)
    hip.trlda_rng_get_state(state)
    alpha, eta = model.alpha, model.eta
    cooc = model.word_cooccurrence(csr)
    anchors = model.anchor_words(cooc)
    beta, pi = model.recover_topics(cooc, anchors)
    strength = cooc.num_tokens
    assert strength == int(csr.cnts.sum())
    want = eta + (float(strength) * pi)[:, None] * beta
    got = model.initialize_spectral(iter(_cuts(csr, 90)))
    lam = model.lambdas
    assert np.array_equal(got, anchors) and np.array_equal(lam, want)
    assert np.isfinite(lam).all() and (lam > 0).all()
    assert np.abs(lam.sum(axis=1) - (eta * V + strength * pi)).max() <= 1e-12 * strength
    # from an accumulator, with a strength of one's own
    model.initialize_spectral(cooc, strength=50.0, tol=1e-7)
    assert np.array_equal(model.lambdas, eta + (50.0 * pi)[:, None] * beta)
    after = np.zeros(33, dtype=np.uint32)
    hip.trlda_rng_get_state(after)
    assert np.array_equal(after, state)
    assert np.array_equal(model.alpha, alpha) and model.eta == eta
    with pytest.raises(TypeError):
        model.initialize_spectral(cooc, rounds=3)
    # the model trains from there
    model.update_parameters(csr, max_iter_tr=1, max_iter_inference=5)
    assert np.isfinite(model.lambdas).all()
    model.close()


# ---- 5. errors ------------------------------------------------------------------------------------------

def test_errors(hip):
    from trlda_amd import WordCooccurrence
    from trlda_amd.documents import CSRDocuments
    V = 50
    model, other = _model(3, V), _model(3, V + 1)
    with pytest.raises(RuntimeError, match=str(2 * V * 52 * 8)):           # the bytes needed are named
        model.word_cooccurrence(max_bytes=1000)
    cooc = model.word_cooccurrence()
    with pytest.raises(RuntimeError, match="empty"):
        cooc.word_probabilities()
    with pytest.raises(RuntimeError, match="candidate"):
        model.anchor_words(cooc)
    csr = _corpus(30, V, seed=2)
    with pytest.raises(RuntimeError):
        cooc.add(other.upload(_corpus(5, V + 1, seed=2)))                 # a batch of another model
    with pytest.raises(RuntimeError, match="once per document"):
        cooc.add(CSRDocuments([0, 3], [4, 7, 4], [1, 1, 1]))
    with pytest.raises(RuntimeError, match="negative"):
        cooc.add(CSRDocuments([0, 2], [4, 7], [1, -1]))
    assert cooc.num_documents == 0 and not cooc.read().any()              # the refused batches added nothing
    cooc.add(csr)
    with pytest.raises(RuntimeError, match="candidate"):
        model.anchor_words(cooc, num_anchors=3, min_doc_freq=10 ** 6)
    with pytest.raises(RuntimeError):
        other.anchor_words(cooc)                                          # an accumulator of another model
    for bad in ([0, V], [-1, 2], [3, 3], [], [[1, 2]], [0.5, 2.0]):
        with pytest.raises(RuntimeError):
            model.recover_topics(cooc, np.array(bad))
    Q = cooc.read()
    for spoil in ("asymmetric", "negative", "nan", "shape"):
        q = Q.copy()
        if spoil == "asymmetric":
            q[1, 2] += 1e-9
        elif spoil == "negative":
            q[1, 2] = q[2, 1] = -1e-9
        elif spoil == "nan":
            q[4, 4] = np.nan
        else:
            q = q[:-1]
        with pytest.raises(RuntimeError):
            WordCooccurrence.from_matrix(model, q)
    with pytest.raises(RuntimeError):
        model.anchor_words(WordCooccurrence.from_matrix(model, Q), min_doc_freq=2)   # no doc_freq was given
    loaded = WordCooccurrence.from_matrix(model, Q, doc_freq=cooc.doc_freq)
    assert np.array_equal(model.anchor_words(loaded, min_doc_freq=2), model.anchor_words(cooc, min_doc_freq=2))
    lam = model.lambdas
    with pytest.raises(RuntimeError, match="strength"):                   # a loaded matrix has counted no tokens
        model.initialize_spectral(loaded)
    assert np.array_equal(model.lambdas, lam)
    model.initialize_spectral(loaded, strength=100.0, min_doc_freq=2)
    assert (model.lambdas > 0).all() and abs(model.lambdas.sum() - (0.3 * 3 * V + 100.0)) < 1e-9
    cooc.close()
    with pytest.raises(RuntimeError, match="closed"):
        cooc.read()
    model.close()
    other.close()


# ---- 6. buffers -----------------------------------------------------------------------------------------

def test_no_buffer_is_left_after_close(hip):
    """A fresh process (the count is the process's): after the four stages and close() the library holds
    no device buffer."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "anchor_buffers_worker.py")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, worker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout
