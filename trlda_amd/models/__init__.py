"""``trlda_amd.models`` -- host-side mirror of ``trlda.models`` (reference
python/models/__init__.py:1-5) for the accelerated path.

Same class names, constructor arguments, properties, method signatures, defaults and
error behaviour as the reference's CPython types (python/src/module.cpp,
ldainterface.cpp, onlineldainterface.cpp, batchldainterface.cpp); the computation
goes through ``libtrlda_hip.so`` (include/trlda_hip.h) to the gfx950 kernels.  State
(lambda) lives in HBM; getters return fresh, read-only, Fortran-ordered copies just
like ``PyArray_FromMatrixXd`` (python/src/pyutils.cpp:15-36).
"""
import ctypes as C
import operator
import os

import numpy as np

from .. import _ffi
from ..documents import CSRDocuments, DeviceBatch, DocumentList, as_csr
from ..index import _measure

__all__ = ["Distribution", "LDA", "OnlineLDA", "BatchLDA", "CumulativeLDA"]


def _default_device():
    return int(os.environ.get("LOCAL_RANK", "0"))


def _alpha_vector(alpha, num_topics):
    """alpha argument handling of OnlineLDA_init (onlineldainterface.cpp:58-83).

    Returns (K, alpha[K]).  A scalar keeps ``num_topics``; an array *defines* K
    (the reference calls the ArrayXd constructor and ignores num_topics)."""
    if alpha is None:
        alpha = .1
    if isinstance(alpha, (float, int, np.floating, np.integer)) and not isinstance(alpha, bool):
        return int(num_topics), np.full(int(num_topics), float(alpha), dtype=np.float64)
    try:
        arr = np.asarray(alpha, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("Alpha should be of type `ndarray`.")
    if arr.ndim == 0:
        return int(num_topics), np.full(int(num_topics), float(arr), dtype=np.float64)
    if arr.ndim == 1:
        arr = arr.reshape(-1, 1)
    if arr.ndim != 2:
        raise TypeError("Alpha should be one-dimensional.")
    if arr.shape[0] == 1:
        arr = arr.T
    if arr.shape[1] != 1:
        raise TypeError("Alpha should be one-dimensional.")
    return arr.shape[0], np.ascontiguousarray(arr[:, 0])


_INFERENCE_METHODS = "`inference_method` should be one of 'VI', 'GIBBS' or 'CVB0'."
_CVB0_NO_TRAINING = "Training from CVB0 statistics is not built yet: use 'VI' or 'GIBBS' here."


def _inference_method(name):
    """ldainterface.cpp:343-359: first letter decides; returns 'VI', 'GIBBS' or -- beyond the
    reference -- 'CVB0'."""
    if name is None:
        return "VI"
    if not isinstance(name, str):
        raise TypeError(_INFERENCE_METHODS)
    first = name[:1]
    if first in ("v", "V"):
        return "VI"
    if first in ("g", "G"):
        return "GIBBS"
    if first in ("c", "C"):
        return "CVB0"
    raise TypeError(_INFERENCE_METHODS)


def _coherence(measure, doc_freq, co, num_docs):
    """UMass / NPMI per word list from the device's counts (LDA.topic_coherence): K N^2-sized fp64
    arithmetic on the host, the pairs (l, m), l < m, added in the order m ascending, then l
    ascending."""
    T, N = doc_freq.shape
    m_idx, l_idx = np.array([(m, l) for m in range(1, N) for l in range(m)], dtype=np.int64).T
    d_l = doc_freq[:, l_idx].astype(np.float64)
    d_m = doc_freq[:, m_idx].astype(np.float64)
    d_lm = co[:, l_idx, m_idx].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure == "umass":
            keep = d_l > 0
            term = np.where(keep, np.log((d_lm + 1.) / d_l), 0.)
            used = keep.sum(axis=1)
            total = np.cumsum(term, axis=1)[:, -1]
            return np.where(used > 0, total / np.maximum(used, 1), np.nan)
        M = float(num_docs)
        log_m = np.log(M)
        term = (np.log(d_lm) + log_m - np.log(d_l) - np.log(d_m)) / (log_m - np.log(d_lm))
        term = np.where(d_lm == M, 1., term)
        term = np.where(d_lm == 0, -1., term)
        return np.cumsum(term, axis=1)[:, -1] / float(len(m_idx))


TOPIC_MEASURES = {"hellinger": 0, "cosine": 1, "kl": 2, "jensen_shannon": 3, "js": 3}


def _topic_measure(name):
    if not isinstance(name, str):
        raise TypeError("`measure` should be of type `str`.")
    try:
        return TOPIC_MEASURES[name.lower()]
    except KeyError:
        raise ValueError("Unknown measure '%s' (expected 'hellinger', 'cosine', 'kl' or "
                         "'jensen_shannon')." % name)


def _greedy_match(dist):
    """Greedy one-to-one matching on a K x K' distance matrix (LDA.match_topics): K K'-sized host
    arithmetic.  The pairs in the total order (distance, i, j) -- a stable sort of the row-major
    matrix -- each kept when both its topics are free."""
    K, K2 = dist.shape
    match = np.full(K, -1, dtype=np.int64)
    best = np.full(K, np.inf, dtype=np.float64)
    col_free = np.ones(K2, dtype=bool)
    left = min(K, K2)
    flat = np.ascontiguousarray(dist).ravel()
    for e in np.argsort(flat, kind="stable"):
        i, j = divmod(int(e), K2)
        if match[i] < 0 and col_free[j]:
            match[i], best[i], col_free[j] = j, flat[e], False
            left -= 1
            if left == 0:
                break
    return match, best


RECOMMEND_MAX_TOP_N = 100


def _seen_keys(indptr, ids, cnts, num_words):
    """The sorted distinct keys ``d * num_words + w`` of the entries ``(w, c)`` with ``c > 0`` of a
    CSR: the (document, word) pairs a part has seen."""
    indptr = np.asarray(indptr, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    doc = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    keep = np.asarray(cnts) > 0
    return np.unique(doc[keep] * np.int64(num_words) + ids[keep])


def _recall_at(words, observed, heldout, num_words):
    """Recall of recommended word ids against held-out words (LDA.recall_at): host arithmetic on
    B x top_n ids.  ``words``: int B x top_n, -1 where a row is padded; ``observed`` and ``heldout``:
    the two parts as CSR triples ``(indptr, ids, cnts)`` of B documents each.  A word is relevant
    to document d when ``heldout_d`` has it with a positive count and ``observed_d`` has not seen it
    (no entry with a positive count); repeated entries count once.  Returns ``(recall, hits,
    relevant)``: per document the number of relevant words and how many of them are among its
    recommended ids (int64, length B), and the mean of ``hits / relevant`` over the documents with
    ``relevant > 0``, added in document order.  RuntimeError when there is no such document."""
    words = np.asarray(words, dtype=np.int64)
    B = words.shape[0]
    V = np.int64(num_words)
    if len(observed[0]) - 1 != B or len(heldout[0]) - 1 != B:
        raise RuntimeError("Observed and held-out documents should be equal in number.")
    want = np.setdiff1d(_seen_keys(*heldout, num_words=V), _seen_keys(*observed, num_words=V),
                        assume_unique=True)
    relevant = np.bincount(want // V, minlength=B).astype(np.int64)
    row = np.repeat(np.arange(B, dtype=np.int64), words.shape[1]).reshape(words.shape)
    given = np.unique((row * V + words)[words >= 0])
    hits = np.bincount(np.intersect1d(given, want, assume_unique=True) // V, minlength=B).astype(np.int64)
    keep = relevant > 0
    if not keep.any():
        raise RuntimeError("There are no held-out words that the observed parts have not seen.")
    ratio = hits[keep] / relevant[keep].astype(np.float64)
    return float(np.cumsum(ratio)[-1] / ratio.size), hits, relevant


def _ranks_entries(indptr, ids, ranks, scores, num_words):
    """The library's per-entry ranks (LDA.heldout_ranks) as per-document lists: of the entries with a
    positive rank each distinct (document, word) once -- a word listed twice has the same rank twice
    -- in ascending word id.  Returns ``(indptr int64, words int32, ranks int32, scores float64)``."""
    indptr = np.asarray(indptr, dtype=np.int64)
    B = len(indptr) - 1
    V = np.int64(num_words)
    doc = np.repeat(np.arange(B, dtype=np.int64), np.diff(indptr))
    keep = np.flatnonzero(np.asarray(ranks) > 0)
    key, first = np.unique(doc[keep] * V + np.asarray(ids, dtype=np.int64)[keep], return_index=True)
    at = keep[first]
    out = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // V, minlength=B), out=out[1:])
    return (out, (key % V).astype(np.int32), np.asarray(ranks, dtype=np.int32)[at],
            np.asarray(scores, dtype=np.float64)[at])


def _ranking_tops(top_n):
    """``top_n`` of LDA.ranking_metrics as a tuple of positive ints (one int: a tuple of one)."""
    try:
        tops = (operator.index(top_n),)
    except TypeError:
        try:
            tops = tuple(operator.index(n) for n in top_n)
        except TypeError:
            raise TypeError("`top_n` should be an integer or a sequence of integers.")
    if any(n < 1 for n in tops):
        raise RuntimeError("`top_n` should hold positive integers.")
    return tops


def _ranking_metrics(indptr, ranks, candidates, top_n, return_documents=False):
    """Full-ranking metrics from the ranks of the relevant words (LDA.ranking_metrics): host arithmetic
    in float64, every sum through ``math.fsum``.  ``indptr`` (B + 1) and ``ranks`` (1-based) as
    ``LDA.heldout_ranks`` returns them, ``candidates`` (B) the length n of each document's ranking,
    ``top_n`` an int or a sequence of positive ints.  Document d with relevant ranks
    r_1 < ... < r_R among n candidates:

        mean_percentile_rank  mean over all relevant (d, w) of (r - 1) / (n - 1), 0 where n = 1
        auc                   1 - sum_j (r_j - j) / (R (n - R)); mean over documents with R > 0, n > R
        mrr                   mean of 1 / r_1
        map                   mean of (1 / R) sum_j j / r_j
        ndcg                  mean of sum_j 1 / log2(1 + r_j) / sum_{j = 1..R} 1 / log2(1 + j)
        recall[N]             mean of #{r_j <= N} / R, for every N of top_n

    the means over the documents with R > 0 (RuntimeError when there is none; ``auc`` is NaN when no
    document has n > R).  With ``return_documents`` the entry ``documents`` holds the per-document
    arrays (``relevant`` int64; ``percentile_rank``, ``auc``, ``mrr``, ``map``, ``ndcg`` and
    ``recall[N]`` float64, NaN where a document is left out of the mean)."""
    import math
    tops = _ranking_tops(top_n)
    indptr = np.asarray(indptr, dtype=np.int64)
    ranks = np.asarray(ranks, dtype=np.int64)
    candidates = np.asarray(candidates, dtype=np.int64)
    B = len(indptr) - 1
    if len(candidates) != B:
        raise RuntimeError("`candidates` should hold one value per document.")
    relevant = np.diff(indptr)
    if not (relevant > 0).any():
        raise RuntimeError("There are no held-out words that the observed parts have not seen.")
    doc = {name: np.full(B, np.nan) for name in ("percentile_rank", "auc", "mrr", "map", "ndcg")}
    doc_recall = {n: np.full(B, np.nan) for n in tops}
    pairs = []
    for d in np.flatnonzero(relevant > 0):
        r = np.sort(ranks[indptr[d]:indptr[d + 1]]).astype(np.float64)
        R, n = len(r), int(candidates[d])
        j = np.arange(1, R + 1, dtype=np.float64)
        pct = (r - 1.0) / (n - 1.0) if n > 1 else np.zeros(R)
        pairs.extend(pct.tolist())
        doc["percentile_rank"][d] = math.fsum(pct) / R
        if n > R:
            doc["auc"][d] = 1.0 - math.fsum(r - j) / (float(R) * float(n - R))
        doc["mrr"][d] = 1.0 / r[0]
        doc["map"][d] = math.fsum(j / r) / R
        doc["ndcg"][d] = math.fsum(1.0 / np.log2(1.0 + r)) / math.fsum(1.0 / np.log2(1.0 + j))
        for top in tops:
            doc_recall[top][d] = np.count_nonzero(r <= top) / float(R)

    def mean(a):
        a = a[~np.isnan(a)]
        return math.fsum(a) / len(a) if len(a) else float("nan")

    out = {"mean_percentile_rank": math.fsum(pairs) / len(pairs), "auc": mean(doc["auc"]),
           "mrr": mean(doc["mrr"]), "map": mean(doc["map"]), "ndcg": mean(doc["ndcg"]),
           "recall": {n: mean(doc_recall[n]) for n in tops}}
    if return_documents:
        out["documents"] = dict(doc, recall=doc_recall, relevant=relevant.astype(np.int64))
    return out


class Distribution(object):
    """Abstract base (reference include/distribution.h, distributioninterface.cpp)."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("This is an abstract class.")


class LDA(Distribution):
    """Base of the LDA models: state + the E-step (reference include/lda.h)."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("This is an abstract class.")      # ldainterface.cpp:35-38

    # -- construction shared by the subclasses --------------------------------------
    def _setup(self, num_words, num_topics, alpha, eta, device, _lambda=None):
        if int(num_words) <= 0:
            raise RuntimeError("Number of words should be positive.")
        K, alpha_vec = _alpha_vector(alpha, num_topics)
        if K <= 0:
            raise RuntimeError("Number of topics should be positive.")
        self._V = int(num_words)
        self._K = int(K)
        self._alpha = alpha_vec
        self._eta = float(eta)
        self._device = _default_device() if device is None else int(device)
        self._handle = _ffi.vp()
        L = _ffi.lib()
        _ffi.require_gpu()
        _ffi.check(L.trlda_model_create(C.byref(self._handle), self._device, self._K, self._V))
        _ffi.check(L.trlda_model_set_alpha(self._handle, self._alpha))
        if _lambda is None:
            # lambda = sampleGamma(K, V, 100) / 100 from libc rand()       (lda.cpp:71)
            lam = np.empty((self._K, self._V), dtype=np.float64, order="F")
            L.trlda_sample_gamma_init(self._K, self._V, lam)
        else:
            lam = np.asfortranarray(_lambda, dtype=np.float64)
        _ffi.check(L.trlda_model_set_lambda(self._handle, lam))

    # An empirical-Bayes step whose device sums are still on their way (OnlineLDA defers the wait
    # so that the next mini-batch is parsed, converted and uploaded meanwhile): (rho, min_alpha,
    # min_eta), finished by whoever next needs alpha, eta or an E-step.
    _eb_pending = None

    def _settle(self):
        pending = self._eb_pending
        if pending is None:
            return
        self._eb_pending = None
        rho, min_alpha, min_eta = pending
        alpha = np.ascontiguousarray(self._alpha, dtype=np.float64).copy()
        eta = C.c_double(self._eta)
        _ffi.check(_ffi.lib().trlda_model_online_eb_finish(self._handle, rho, min_alpha, min_eta,
                                                          alpha, C.byref(eta)))
        self._alpha, self._eta = alpha, float(eta.value)

    def close(self):
        # an empirical-Bayes step still on its way is finished, not dropped: alpha / eta stay
        # readable after close() with the values the last update_parameters call gave them
        if getattr(self, "_handle", None) and self._eb_pending is not None:
            try:
                self._settle()
            except Exception:                        # noqa: BLE001 -- closing must not raise
                self._eb_pending = None
        self._eb_pending = None
        # (a document index runs on the model's stream: it goes first)
        for index in list(getattr(self, "_indexes", None) or ()):
            index.close()
        if getattr(self, "_handle", None):
            _ffi.lib().trlda_model_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- properties (ldainterface.cpp:41-148, module.cpp:67-90) ---------------------
    @property
    def num_topics(self):
        return self._K

    @property
    def num_words(self):
        return self._V

    @property
    def device(self):
        return self._device

    def _get_lambda(self):
        lam = np.empty((self._K, self._V), dtype=np.float64, order="F")
        _ffi.check(_ffi.lib().trlda_model_get_lambda(self._handle, lam))
        lam.flags.writeable = False                                  # ldainterface.cpp:57
        return lam

    def _set_lambda(self, value):
        try:
            arr = np.asarray(value, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError("Lambda should be of type `ndarray`.")
        if arr.ndim == 1:
            arr = arr.reshape(-1, 1)                                 # pyutils.cpp:91-128
        if arr.ndim != 2 or arr.shape != (self._K, self._V):
            raise RuntimeError("Lambda has wrong dimensionality.")   # lda.h:186-187
        _ffi.check(_ffi.lib().trlda_model_set_lambda(self._handle, np.asfortranarray(arr)))

    lambdas = property(_get_lambda, _set_lambda,
                       doc="Parameters governing beliefs over topics (K x V).")
    _lambda = property(_get_lambda, _set_lambda, doc="Alias for `lambdas`.")

    @property
    def alpha(self):
        self._settle()
        return self._alpha.reshape(-1, 1).copy(order="F")            # K x 1, ldainterface.cpp:87

    @alpha.setter
    def alpha(self, value):
        if isinstance(value, (float, int, np.floating, np.integer)) and \
                not isinstance(value, bool):
            if value < 0.:
                raise RuntimeError("Alpha should not be negative.")  # lda.h:147-151
            new = np.full(self._K, float(value), dtype=np.float64)
        else:
            _, new = _alpha_vector(value, self._K)
            if new.size != self._K:
                raise RuntimeError("Alpha has wrong dimensionality.")  # lda.h:155-156
            if (new < 0.).any():
                raise RuntimeError("Alpha should not be negative.")
        self._settle()
        _ffi.check(_ffi.lib().trlda_model_set_alpha(self._handle, new))
        self._alpha = new

    @property
    def eta(self):
        self._settle()
        return self._eta

    @eta.setter
    def eta(self, value):
        value = float(value)
        if value < 0.:
            raise RuntimeError("Eta should not be negative.")        # lda.h:172-173
        self._settle()
        self._eta = value

    # -- documents ---------------------------------------------------------------
    def upload(self, docs):
        """Convert + upload a batch once; the result can be passed as ``docs``."""
        if isinstance(docs, DeviceBatch):
            return docs
        return DeviceBatch(docs, self._V, self._device)

    def _batch(self, docs):
        if isinstance(docs, DeviceBatch):
            if docs.num_words != self._V or docs.device != self._device:
                raise RuntimeError("Batch was uploaded for a different model.")
            return docs, False
        return DeviceBatch(docs, self._V, self._device), True

    # -- E-step (ldainterface.cpp:311-390 -> lda.cpp:119-220) ------------------------
    def update_variables(self, docs, latents=None, inference_method='VI', max_iter=100,
                         threshold=0.001, num_samples=1, burn_in=2, return_iterations=False):
        """E-step: returns ``(gamma K x N, sstats K x V)`` as Fortran-ordered float64.

        ``inference_method='GIBBS'`` (ldainterface.cpp:343-385 -> lda.cpp:224-293) returns
        ``(theta K x N, sstats K x V)`` instead: collapsed Gibbs sampling of the tokens' topics on
        the GPU (csrc/gibbs_kernels.h, K <= 1024), ``burn_in`` sweeps, then ``num_samples``
        sweeps whose topic counts make up the statistics (each token adds ``1 / num_samples``;
        they are not multiplied by exp E[log beta], unlike VI), and ``theta = Dirichlet(alpha +
        topic counts)`` of the final state.  ``latents`` is the initial theta (default:
        Dirichlet(1) per document).  Deviations from the reference: the
        initialisation reads theta's column of the document, not of the word (lda.cpp:254);
        the random numbers are Philox4x32-10 keyed by two draws of the seeded stream, so
        ``trlda.seed`` makes a call reproducible and results do not depend on the launch; the
        statistics are exact counts scaled once; theta's gamma draws are Marsaglia-Tsang in log
        space.  ``return_iterations`` does not apply to Gibbs sampling (TypeError).

        ``inference_method='CVB0'`` (no reference counterpart; csrc/cvb0_kernels.h, K <= 1024)
        returns ``(theta K x N, sstats K x V[, iters])``: collapsed variational Bayes, zero order
        (Asuncion et al. 2009; Foulds et al. 2013) -- the deterministic form of the Gibbs
        conditional, each token's topic count replaced by its expectation.  At most ``max_iter``
        sweeps per document, ended once the mean change of its expected topic counts is below
        ``threshold``; ``latents`` is the weight vector the documents' responsibilities start
        from (default: alpha).  ``theta = (alpha + n) / (sum alpha + N_d)``; the statistics are
        expected counts, not multiplied by exp E[log beta] (like Gibbs).  No seed is involved:
        calls repeat bitwise.  ``num_samples`` and ``burn_in`` are ignored, as VI ignores them."""
        method = _inference_method(inference_method)
        if method == "CVB0":
            return self._update_variables_cvb0(docs, latents, max_iter, threshold, return_iterations)
        if method == "GIBBS":
            if return_iterations:
                raise TypeError("`return_iterations` applies to VI only.")
            return self._update_variables_gibbs(docs, latents, num_samples, burn_in)
        _ffi.check_vi_topics(self._K)                               # (before the draw and the upload)
        batch, owned = self._batch(docs)
        try:
            self._settle()
            B = len(batch)
            L = _ffi.lib()
            if latents is not None:
                try:
                    g = np.array(latents, dtype=np.float64, order="F", copy=True)
                except (TypeError, ValueError):
                    raise TypeError("`latents` should be of type `ndarray`.")
                if g.ndim == 1:
                    g = g.reshape(-1, 1, order="F")
                if g.ndim != 2 or g.shape != (self._K, B):
                    raise RuntimeError("Initial gamma has wrong dimensionality.")  # lda.cpp:165
                gamma = np.asfortranarray(g)
            else:
                gamma = np.empty((self._K, B), dtype=np.float64, order="F")
                L.trlda_sample_gamma_init(self._K, B, gamma)          # lda.cpp:135
            sstats = np.empty((self._K, self._V), dtype=np.float64, order="F")
            iters = np.zeros(B, dtype=np.int32)
            _ffi.check(L.trlda_model_estep_host(self._handle, batch.handle, gamma, sstats,
                                                int(max_iter), float(threshold),
                                                iters.ctypes.data))
        finally:
            if owned:
                batch.close()
        if return_iterations:
            return gamma, sstats, iters
        return gamma, sstats

    do_e_step = update_variables                                     # module.cpp:103-106

    def _initial_theta(self, latents, B):
        """The K x B in/out array of the Gibbs and CVB0 entry points: a checked copy of ``latents``,
        or zeros for the result."""
        if latents is None:
            return np.zeros((self._K, B), dtype=np.float64, order="F")
        try:
            t = np.array(latents, dtype=np.float64, order="F", copy=True)
        except (TypeError, ValueError):
            raise TypeError("`latents` should be of type `ndarray`.")
        if t.ndim == 1:
            t = t.reshape(-1, 1, order="F")
        if t.ndim != 2 or t.shape != (self._K, B):
            raise RuntimeError("Initial theta has wrong dimensionality.")  # lda.cpp:229-230
        return np.asfortranarray(t)

    def _update_variables_gibbs(self, docs, latents, num_samples, burn_in):
        """lda.cpp:224-293 through trlda_model_gibbs_host (include/trlda_hip.h)."""
        num_samples, burn_in = int(num_samples), int(burn_in)
        if num_samples < 0 or burn_in < 0:
            raise RuntimeError("`num_samples` and `burn_in` should not be negative.")
        batch, owned = self._batch(docs)
        try:
            self._settle()
            B = len(batch)
            theta = self._initial_theta(latents, B)
            sstats = np.empty((self._K, self._V), dtype=np.float64, order="F")
            _ffi.check(_ffi.lib().trlda_model_gibbs_host(self._handle, batch.handle, theta,
                                                         int(latents is not None), sstats,
                                                         num_samples, burn_in))
        finally:
            if owned:
                batch.close()
        return theta, sstats

    def _update_variables_cvb0(self, docs, latents, max_iter, threshold, return_iterations):
        """CVB0 through trlda_model_cvb0_host (include/trlda_hip.h)."""
        batch, owned = self._batch(docs)
        try:
            self._settle()
            B = len(batch)
            theta = self._initial_theta(latents, B)
            sstats = np.empty((self._K, self._V), dtype=np.float64, order="F")
            iters = np.zeros(B, dtype=np.int32)
            _ffi.check(_ffi.lib().trlda_model_cvb0_host(self._handle, batch.handle, theta,
                                                        int(latents is not None), sstats,
                                                        int(max_iter), float(threshold),
                                                        iters.ctypes.data))
        finally:
            if owned:
                batch.close()
        if return_iterations:
            return theta, sstats, iters
        return theta, sstats

    # -- the variational lower bound (ldainterface.cpp:394-470 -> lda.cpp:297-360) ----------
    def _default_num_documents(self):
        return -1                                                    # lda.h: numDocuments = -1

    def lower_bound(self, docs, num_documents=-1, inference_method='VI', max_iter=100,
                    num_samples=1, burn_in=2):
        """Estimate of the lower bound on the given documents (fresh E-step from a random
        gamma drawn from the seeded libc stream, as the reference does), scaled to
        ``num_documents`` when that is given.

        Deviation from upstream's actual output: the reference's src/lda.cpp:334 reads
        ``psiLambda.row(id)`` of the K x V matrix where the word's column is meant (an indexing
        slip its release build does not trap); this implements the column read -- the formula of
        the paper and of Hoffman's ``approx_bound`` -- so values differ from upstream's by about
        1e-4 relative on its own test set-up (the oracle can reproduce either).

        ``inference_method='GIBBS'`` raises NotImplementedError: the reference's bound would plug
        the sampled theta in as gamma, which does not bound anything."""
        method = _inference_method(inference_method)
        if method == "CVB0":
            raise NotImplementedError(_CVB0_NO_TRAINING + "  (No bound is defined on them either.)")
        if method != "VI":
            raise NotImplementedError(
                "A lower bound from Gibbs samples (lda.cpp:224-293) is outside the accelerated path.")
        _ffi.check_vi_topics(self._K)
        num_documents = int(num_documents)
        if num_documents < 0:
            num_documents = self._default_num_documents()            # onlinelda.cpp:184-191
        batch, owned = self._batch(docs)
        try:
            self._settle()
            B = len(batch)
            if B == 0:
                raise RuntimeError("The lower bound needs at least one document.")
            L = _ffi.lib()
            gamma = np.empty((self._K, B), dtype=np.float64, order="F")
            L.trlda_sample_gamma_init(self._K, B, gamma)              # lda.cpp:309 -> :135
            factor = num_documents / float(B) if num_documents >= 0 else 1.   # lda.cpp:302-303
            bound = C.c_double(0.)
            _ffi.check(L.trlda_model_lower_bound(self._handle, batch.handle, gamma, self._eta,
                                                 factor, int(max_iter), 0.001, C.byref(bound)))
        finally:
            if owned:
                batch.close()
        return bound.value

    # -- held-out predictive log-likelihood (Hoffman et al. 2013; csrc/heldout_kernels.h) -----------
    def predictive_log_likelihood(self, observed, heldout, latents=None, max_iter=100,
                                  threshold=0.001, return_documents=False):
        """Per-word predictive log-likelihood of held-out words: VI on ``observed`` with lambda
        fixed (from ``latents`` as gamma0, else a random gamma drawn from the seeded stream as
        ``update_variables`` draws it), then

            score = sum_d sum_{(w, c) in heldout_d} c log p(w | d) / sum of those c,
            p(w | d) = sum_k (gamma_dk / sum_j gamma_dj) (lambda_kw / sum_v lambda_kv),

        on the GPU.  ``observed`` and ``heldout`` hold the same documents' two parts
        (``trlda_amd.utils.split_documents``) as lists, ``DocumentList`` or ``DeviceBatch``.
        Returns the score; with ``return_documents=True`` ``(score, loglik, tokens)``, each of the
        last two float64 of length B (per document the sum of c log p(w | d) and of c).  lambda,
        alpha, eta and the update counters stay as they are."""
        _ffi.check_vi_topics(self._K)
        obs, own_obs = self._batch(observed)
        try:
            held, own_held = self._batch(heldout)
        except BaseException:
            if own_obs:
                obs.close()
            raise
        try:
            self._settle()
            B = len(obs)
            if len(held) != B:
                raise RuntimeError("Observed and held-out documents should be equal in number.")
            if int(held.csr.cnts.sum(dtype=np.int64)) <= 0:
                raise RuntimeError("There are no held-out tokens.")
            L = _ffi.lib()
            if latents is not None:
                try:
                    g = np.array(latents, dtype=np.float64, order="F", copy=True)
                except (TypeError, ValueError):
                    raise TypeError("`latents` should be of type `ndarray`.")
                if g.ndim == 1:
                    g = g.reshape(-1, 1, order="F")
                if g.ndim != 2 or g.shape != (self._K, B):
                    raise RuntimeError("Initial gamma has wrong dimensionality.")  # lda.cpp:165
                gamma = np.asfortranarray(g)
            else:
                gamma = np.empty((self._K, B), dtype=np.float64, order="F")
                L.trlda_sample_gamma_init(self._K, B, gamma)          # lda.cpp:135
            loglik = np.empty(B, dtype=np.float64)
            tokens = np.empty(B, dtype=np.float64)
            _ffi.check(L.trlda_model_predictive(self._handle, obs.handle, held.handle, gamma,
                                                int(max_iter), float(threshold), loglik, tokens))
        finally:
            if own_obs:
                obs.close()
            if own_held:
                held.close()
        # totals in document order, as the lower bound adds its documents' terms
        score = float(np.cumsum(loglik)[-1] / np.cumsum(tokens)[-1])
        if return_documents:
            return score, loglik, tokens
        return score

    # -- marginal likelihood of whole documents (Wallach et al. 2009; csrc/marginal_kernels.h) -----
    def document_log_likelihood(self, docs, num_samples=256, proposal='vi', latents=None,
                                max_iter=100, threshold=0.001, return_ess=False):
        """Estimates ``log p(w_d | alpha, beta)`` of each document of ``docs`` (a list,
        ``DocumentList`` or ``DeviceBatch``) by importance sampling of theta on the GPU (Wallach,
        Murray, Salakhutdinov & Mimno 2009, section 4.1).  Per document d with entries (w, c):

            theta_s ~ Dir(a_d),  s = 1 .. num_samples
            log w_s = sum_(w, c) c log(sum_k theta_sk beta_kw) + log Dir(theta_s; alpha) - log Dir(theta_s; a_d)
            loglik_d = logsumexp_s(log w_s) - log num_samples

        ``exp(loglik_d)`` is an unbiased estimate of ``p(w_d | alpha, beta)``.  Topics enter as the
        point estimate ``beta_kw = lambda_kw / sum_v lambda_kv`` that ``predictive_log_likelihood``
        uses, not integrated over ``Dir(lambda_k)``.  ``proposal='vi'``: ``a_d`` is the document's
        gamma from the E-step of ``update_variables`` on lambda as it is (``latents`` as gamma0, else
        a random gamma drawn from the seeded stream; ``max_iter``, ``threshold`` as there);
        ``proposal='prior'``: ``a_d = alpha``, no E-step (``latents`` is then a TypeError) -- far
        higher variance on all but the shortest documents.

        Returns a float64 array of length B, nats per document (an empty document: exactly 0); with
        ``return_ess=True`` ``(loglik, ess)``, ``ess_d = (sum_s w_s)^2 / sum_s w_s^2`` being the
        effective sample size, between 1 and ``num_samples``: when it is a small fraction of
        ``num_samples`` a few samples carry the estimate, which is then poor (too low, as a rule)
        -- take more samples or the 'vi' proposal.  Per-word perplexity of the documents is
        ``exp(-loglik.sum() / number of tokens)``.

        The draws are Philox4x32-10 keyed by two draws of the seeded stream (after gamma0's), so
        ``trlda.seed`` makes a call reproducible, and a document's value depends on its position in
        ``docs`` but not on the other documents.  lambda, alpha, eta and the update counters stay
        as they are."""
        if not isinstance(proposal, str) or proposal.lower() not in ("vi", "prior"):
            raise TypeError("`proposal` should be either 'vi' or 'prior'.")
        vi = proposal.lower() == "vi"
        if latents is not None and not vi:
            raise TypeError("`latents` applies to the 'vi' proposal only.")
        num_samples = operator.index(num_samples)
        if num_samples < 1:
            raise RuntimeError("`num_samples` should be positive.")
        if num_samples * self._K >= 2 ** 32:
            raise RuntimeError("`num_samples` times the number of topics should be below 2^32.")
        _ffi.check_vi_topics(self._K)                               # (before the draw and the upload)
        batch, owned = self._batch(docs)
        try:
            self._settle()
            B = len(batch)
            L = _ffi.lib()
            gamma = None
            if latents is not None:
                try:
                    g = np.array(latents, dtype=np.float64, order="F", copy=True)
                except (TypeError, ValueError):
                    raise TypeError("`latents` should be of type `ndarray`.")
                if g.ndim == 1:
                    g = g.reshape(-1, 1, order="F")
                if g.ndim != 2 or g.shape != (self._K, B):
                    raise RuntimeError("Initial gamma has wrong dimensionality.")  # lda.cpp:165
                gamma = np.asfortranarray(g)
            elif vi:
                gamma = np.empty((self._K, B), dtype=np.float64, order="F")
                L.trlda_sample_gamma_init(self._K, B, gamma)          # lda.cpp:135
            loglik = np.empty(B, dtype=np.float64)
            ess = np.empty(B, dtype=np.float64)
            _ffi.check(L.trlda_model_document_loglik(
                self._handle, batch.handle, None if gamma is None else gamma.ctypes.data,
                _ffi.PROPOSAL_VI if vi else _ffi.PROPOSAL_PRIOR, num_samples, int(max_iter),
                float(threshold), loglik, ess.ctypes.data))
        finally:
            if owned:
                batch.close()
        if return_ess:
            return loglik, ess
        return loglik

    # -- left-to-right likelihood of whole documents (Wallach et al. 2009, Alg. 3; csrc/l2r_kernels.h)
    def left_to_right(self, docs, num_particles=20, resample=True, combine='particle',
                      return_tokens=False):
        """Estimates ``log p(w_d | alpha, beta)`` of each document of ``docs`` (a list,
        ``DocumentList`` or ``DeviceBatch``) by the left-to-right sequential sampler on the GPU
        (Wallach, Murray, Salakhutdinov & Mimno 2009, Algorithm 3; Buntine 2009).  It samples the
        tokens' topics, not theta, so unlike ``document_log_likelihood`` it has no proposal that
        can fit badly.  Per document with tokens w_0 .. w_{N-1} (the entries in order, an entry
        ``(w, c)`` giving ``c`` consecutive tokens), per particle r and position n, with n_k the
        counts of the topics the prefix's tokens hold at the moment:

            resample: for t = 0 .. n-1: take z_t out; z_t ~ beta_{k, w_t} (alpha_k + n_k); put it back
            z_n ~ beta_{k, w_n} (alpha_k + n_k);  p_r(n) = sum_k beta_{k, w_n} (alpha_k + n_k) / (sum alpha + n)

        ``resample=False`` is the O(N) sequential sampler; ``resample=True`` costs O(N^2) per
        particle and has the lower variance.  Topics enter as the point estimate
        ``beta_kw = lambda_kw / sum_v lambda_kv`` of ``predictive_log_likelihood``.

        ``combine='particle'`` (default): ``loglik_d = logsumexp_r(sum_n log p_r(n)) - log R``, the
        mean over the particles of each particle's product; ``exp(loglik_d)`` is an unbiased
        estimate of ``p(w_d | alpha, beta)`` for any number of particles R.
        ``combine='position'``: ``loglik_d = sum_n log(mean_r p_r(n))``, Algorithm 3 as published.
        It looks consistent but is biased for R > 1, and the bias does not shrink with R: one
        prefix sweep does not draw exactly from p(z_<n | w_<n), so each per-position mean is itself
        off.  On a 6-token, K = 3 document the mean of ``exp(loglik - exact)`` over 20 000 runs was
        0.9854 +- 0.0019 at R = 4 and 0.9840 +- 0.0009 at R = 16 (1.0293 +- 0.0013 at R = 4
        without ``resample``), against 0.9997 +- 0.0020 and 1.0008 +- 0.0009 for 'particle'
        (DESIGN.md 3.17).  With one particle the two are the same bits.

        Returns a float64 array of length B, nats per document (a document without tokens: exactly
        0); with ``return_tokens=True`` ``(loglik, tokens)``, ``tokens`` holding the N_d as float64,
        so that per-word perplexity is ``exp(-loglik.sum() / tokens.sum())``.

        The draws are Philox4x32-10 keyed by two draws of the seeded stream, so ``trlda.seed`` makes
        a call reproducible; a document's value depends on its position in ``docs`` and on
        ``num_particles`` but not on the other documents.  K <= 1024 (the Gibbs path's limit).
        lambda, alpha, eta and the update counters stay as they are."""
        if not isinstance(combine, str) or combine.lower() not in ("particle", "position"):
            raise TypeError("`combine` should be either 'particle' or 'position'.")
        num_particles = operator.index(num_particles)
        if num_particles < 1:
            raise RuntimeError("`num_particles` should be positive.")
        if max(len(docs), 1) * num_particles >= 2 ** 32:
            raise RuntimeError("The number of documents times `num_particles` should be below 2^32.")
        if self._K > _ffi.L2R_MAX_TOPICS:                           # (before the draw and the upload)
            raise _ffi.TrldaError(_ffi.ERR_ARG, "the left-to-right sampler supports at most 1024 topics "
                                                "(the Gibbs path's limit)")
        batch, owned = self._batch(docs)
        try:
            self._settle()
            B = len(batch)
            loglik = np.empty(B, dtype=np.float64)
            tokens = np.empty(B, dtype=np.float64)
            _ffi.check(_ffi.lib().trlda_model_left_to_right(
                self._handle, batch.handle, num_particles, 1 if resample else 0,
                _ffi.L2R_PARTICLE if combine.lower() == "particle" else _ffi.L2R_POSITION,
                loglik, tokens.ctypes.data))
        finally:
            if owned:
                batch.close()
        if return_tokens:
            return loglik, tokens
        return loglik

    # -- per-word topic posteriors (csrc/wordtopics_kernels.h) --------------------------------------
    def word_topics(self, docs, top_n=1, latents=None, max_iter=100, threshold=0.001,
                    return_gamma=False):
        """The topics each word of each document belongs to: the variational posterior phi that
        the E-step forms inside its fixed point.  VI on ``docs`` (a list, ``DocumentList`` or
        ``DeviceBatch``) with lambda fixed (from ``latents`` as gamma0, else a random gamma drawn
        from the seeded stream as ``update_variables`` draws it), then per ``(id, count)`` pair p of
        document d, on the GPU,

            s_pk = exp(psi(gamma_dk) - psi(sum_v lambda_kv)) exp(psi(lambda_{k, id_p})),
            phi_pk = s_pk / sum_j s_pj.

        Returns ``(indptr, topics, probs)``: ``indptr`` int64 of length B + 1, ``topics`` int32 and
        ``probs`` float64 of shape (number of pairs, top_n).  Rows ``indptr[d] .. indptr[d + 1]``
        line up with document d's pairs as given (a pair with count 0 has a row like any other); a
        row holds the ``top_n`` topics in decreasing phi, equal values by smaller topic id first,
        and their phi.  ``1 <= top_n <= min(num_topics, 32)``, else RuntimeError; with
        ``top_n = num_topics`` a row of ``probs`` is the whole posterior in ranked order.  With
        ``return_gamma=True`` gamma (K x B) is appended.  A document's rows do not depend on the
        other documents of ``docs``.  lambda, alpha, eta and the update counters stay as they are
        (DESIGN.md 3.18)."""
        top_n = operator.index(top_n)
        if not 1 <= top_n <= min(self._K, 32):
            raise RuntimeError("`top_n` should lie between 1 and min(num_topics, 32).")
        _ffi.check_vi_topics(self._K)                               # (before the draw and the upload)
        batch, owned = self._batch(docs)
        try:
            self._settle()
            B = len(batch)
            L = _ffi.lib()
            if latents is not None:
                try:
                    g = np.array(latents, dtype=np.float64, order="F", copy=True)
                except (TypeError, ValueError):
                    raise TypeError("`latents` should be of type `ndarray`.")
                if g.ndim == 1:
                    g = g.reshape(-1, 1, order="F")
                if g.ndim != 2 or g.shape != (self._K, B):
                    raise RuntimeError("Initial gamma has wrong dimensionality.")  # lda.cpp:165
                gamma = np.asfortranarray(g)
            else:
                gamma = np.empty((self._K, B), dtype=np.float64, order="F")
                L.trlda_sample_gamma_init(self._K, B, gamma)          # lda.cpp:135
            indptr = np.asarray(batch.csr.indptr, dtype=np.int64).copy()
            nnz = int(indptr[-1])
            topics = np.empty((nnz, top_n), dtype=np.int32)
            probs = np.empty((nnz, top_n), dtype=np.float64)
            _ffi.check(L.trlda_model_word_topics(self._handle, batch.handle, gamma.ctypes.data, top_n,
                                                 int(max_iter), float(threshold), topics.ctypes.data,
                                                 probs.ctypes.data))
        finally:
            if owned:
                batch.close()
        if return_gamma:
            return indptr, topics, probs, gamma
        return indptr, topics, probs

    # -- the words a document most likely holds next (csrc/recommend_kernels.h) --------------------
    def _recommend_top_n(self, top_n):
        top_n = operator.index(top_n)
        if not 1 <= top_n <= min(self._V, RECOMMEND_MAX_TOP_N):
            raise RuntimeError("`top_n` should lie between 1 and min(num_words, %d)." % RECOMMEND_MAX_TOP_N)
        return top_n

    def recommend(self, docs, top_n=10, exclude_seen=True, latents=None, max_iter=100, threshold=0.001,
                  return_gamma=False):
        """The ``top_n`` words each document of ``docs`` most likely holds next.  VI on ``docs`` (a
        list, ``DocumentList`` or ``DeviceBatch``) with lambda fixed (from ``latents`` as gamma0,
        else a random gamma drawn from the seeded stream as ``update_variables`` draws it), then
        per document d and word w of the vocabulary, on the GPU,

            p(w | d) = sum_k (gamma_dk / sum_j gamma_dj) (lambda_kw / sum_v lambda_kv),

        the quantity ``predictive_log_likelihood`` scores held-out words by, ranked per document.
        With users as documents and items as words (``trlda.utils.load_users``) these are the
        items a user does not have yet and most likely wants.

        Returns ``(words, probs)``, int32 and float64 of shape (B, top_n): per document the words
        in decreasing p(w | d), equal values by smaller word id first, and their p.  With
        ``exclude_seen`` (default) the words a document has seen -- a pair ``(w, c)`` with
        ``c > 0``; repeated pairs count once, ``c <= 0`` does not count -- are left out of its
        ranking; a document with fewer than ``top_n`` words left pads its row with ``(-1, 0.0)``.
        An empty document is ranked from its gamma like any other.  ``1 <= top_n <= min(num_words,
        100)``, else RuntimeError.  With ``return_gamma=True`` gamma (K x B) is appended.  A
        document's row does not depend on the other documents of ``docs``, and two calls agree
        bitwise.  lambda, alpha, eta and the update counters stay as they are."""
        top_n = self._recommend_top_n(top_n)
        _ffi.check_vi_topics(self._K)                               # (before the draw and the upload)
        batch, owned = self._batch(docs)
        try:
            self._settle()
            B = len(batch)
            L = _ffi.lib()
            if latents is not None:
                try:
                    g = np.array(latents, dtype=np.float64, order="F", copy=True)
                except (TypeError, ValueError):
                    raise TypeError("`latents` should be of type `ndarray`.")
                if g.ndim == 1:
                    g = g.reshape(-1, 1, order="F")
                if g.ndim != 2 or g.shape != (self._K, B):
                    raise RuntimeError("Initial gamma has wrong dimensionality.")  # lda.cpp:165
                gamma = np.asfortranarray(g)
            else:
                gamma = np.empty((self._K, B), dtype=np.float64, order="F")
                L.trlda_sample_gamma_init(self._K, B, gamma)          # lda.cpp:135
            words = np.empty((B, top_n), dtype=np.int32)
            probs = np.empty((B, top_n), dtype=np.float64)
            _ffi.check(L.trlda_model_recommend(self._handle, batch.handle, gamma.ctypes.data, top_n,
                                               1 if exclude_seen else 0, int(max_iter), float(threshold),
                                               words.ctypes.data, probs.ctypes.data))
        finally:
            if owned:
                batch.close()
        if return_gamma:
            return words, probs, gamma
        return words, probs

    def recommend_gamma(self, gamma, top_n=10, docs=None):
        """The ranking of ``recommend`` for documents given by their ``gamma`` (K x B, every value
        finite and positive, else RuntimeError; not an array, TypeError): no E-step runs and
        nothing is drawn, so any number of topics is taken, and any positive K x B array serves
        -- the ``alpha + n`` of a Gibbs or CVB0 run as well.  ``docs`` (a list, ``DocumentList``
        or ``DeviceBatch`` of B documents) gives the seen words that are left out; without it
        every word is ranked.  Returns ``(words, probs)`` as ``recommend`` does -- the same
        formula, tie rule (smaller word id first) and pad ``(-1, 0.0)`` -- and on the gamma
        ``recommend`` returned the same bits.  lambda, alpha, eta, the update counters, the
        model's statistics and the seeded stream stay as they are."""
        top_n = self._recommend_top_n(top_n)
        try:
            g = np.array(gamma, dtype=np.float64, order="F", copy=True)
        except (TypeError, ValueError):
            raise TypeError("`gamma` should be of type `ndarray`.")
        if g.ndim == 1:
            g = g.reshape(-1, 1, order="F")
        if g.ndim != 2 or g.shape[0] != self._K:
            raise RuntimeError("Gamma has wrong dimensionality.")
        if not (np.all(np.isfinite(g)) and np.all(g > 0)):
            raise RuntimeError("Gamma should be finite and positive.")
        g = np.asfortranarray(g)
        B = g.shape[1]
        if docs is not None and len(docs) != B:
            raise RuntimeError("`docs` and `gamma` should hold the same number of documents.")
        words = np.empty((B, top_n), dtype=np.int32)
        probs = np.empty((B, top_n), dtype=np.float64)
        if B == 0:
            return words, probs
        batch, owned = self._batch(docs) if docs is not None else (None, False)
        L = _ffi.lib()
        ptrs = []
        try:
            self._settle()
            for nbytes in (g.nbytes, words.nbytes, probs.nbytes):
                ptr = _ffi.vp()
                _ffi.check(L.trlda_dev_alloc(self._device, nbytes, C.byref(ptr)))
                ptrs.append(ptr)
            _ffi.check(L.trlda_dev_upload(self._device, ptrs[0], g.ctypes.data, g.nbytes))
            _ffi.check(L.trlda_model_recommend_dev(self._handle, None if batch is None else batch.handle,
                                                   ptrs[0], B, top_n, ptrs[1], ptrs[2]))
            _ffi.check(L.trlda_model_synchronize(self._handle))
            _ffi.check(L.trlda_dev_download(self._device, words.ctypes.data, ptrs[1], words.nbytes))
            _ffi.check(L.trlda_dev_download(self._device, probs.ctypes.data, ptrs[2], probs.nbytes))
        finally:
            for ptr in ptrs:
                L.trlda_dev_free(self._device, ptr)
            if owned:
                batch.close()
        return words, probs

    def recall_at(self, observed, heldout, top_n=20, latents=None, max_iter=100, threshold=0.001,
                  return_documents=False):
        """Recall@``top_n`` of the recommendations against held-out words.  ``observed`` and
        ``heldout`` hold the same documents' two parts (``trlda_amd.utils.split_documents``) as
        lists, ``DocumentList`` or ``DeviceBatch``, equal in number (else RuntimeError).
        ``recommend(observed, top_n, exclude_seen=True, ...)`` ranks p(w | d) on the GPU, equal
        values by smaller word id first and short rows padded with -1; then per document, on the
        host,

            relevant_d = distinct words with a positive count in heldout_d that observed_d has not seen,
            hits_d     = how many of them are among the recommended ids,
            recall     = mean of hits_d / relevant_d over the documents with relevant_d > 0.

        RuntimeError when no document has a relevant word.  With ``return_documents=True`` returns
        ``(recall, hits, relevant)``, the last two int64 of length B.  lambda, alpha, eta and the
        update counters stay as they are."""
        top_n = self._recommend_top_n(top_n)
        if len(observed) != len(heldout):
            raise RuntimeError("Observed and held-out documents should be equal in number.")
        _ffi.check_vi_topics(self._K)                               # (before the upload and the draw)
        held = as_csr(heldout)
        batch, owned = self._batch(observed)
        try:
            words, _ = self.recommend(batch, top_n=top_n, exclude_seen=True, latents=latents,
                                      max_iter=max_iter, threshold=threshold)
            obs = batch.csr
        finally:
            if owned:
                batch.close()
        recall, hits, relevant = _recall_at(words, (obs.indptr, obs.ids, obs.cnts),
                                            (held.indptr, held.ids, held.cnts), self._V)
        if return_documents:
            return recall, hits, relevant
        return recall

    # -- where held-out words stand in the whole ranking (csrc/ranks_kernels.h) --------------------
    def heldout_ranks(self, observed, heldout, latents=None, max_iter=100, threshold=0.001,
                      return_scores=False, return_gamma=False):
        """The position of every relevant held-out word in the ranking of the whole vocabulary.
        ``observed`` and ``heldout`` hold the same documents' two parts as for ``recall_at`` (lists,
        ``DocumentList`` or ``DeviceBatch``, equal in number, else RuntimeError).  VI on
        ``observed`` exactly as ``recommend`` runs it (``latents`` as gamma0, else the draw of
        ``update_variables``), then on the GPU, per document, the rank of each of its relevant
        words -- the distinct words with a positive count in ``heldout_d`` that ``observed_d`` has
        not seen, ``recall_at``'s rule -- in the ranking ``recommend(observed, exclude_seen=True)``
        would return for it were ``top_n`` unbounded: 1 + the number of unseen words before it in
        the order (p(w | d) descending, word id ascending).  The rank is a count behind the product
        ``recommend`` forms: nothing is sorted and nothing of size B x V exists.

        Returns ``(indptr, words, ranks, candidates)``: ``indptr`` int64 of length B + 1; ``words``
        int32, per document its relevant words in ascending id; ``ranks`` int32, 1-based;
        ``candidates`` int32 of length B, ``n_d = num_words - (distinct words d has seen)``, the
        length of that ranking.  ``return_scores=True`` appends the float64 p(w | d) of each
        relevant word (the bits ``recommend`` returns for it), ``return_gamma=True`` gamma (K x B).
        A document's ranks do not depend on the other documents, and two calls agree bitwise.
        lambda, alpha, eta and the update counters stay as they are."""
        if len(observed) != len(heldout):
            raise RuntimeError("Observed and held-out documents should be equal in number.")
        _ffi.check_vi_topics(self._K)                               # (before the draw and the upload)
        obs, own_obs = self._batch(observed)
        try:
            held, own_held = self._batch(heldout)
        except BaseException:
            if own_obs:
                obs.close()
            raise
        try:
            self._settle()
            B = len(obs)
            L = _ffi.lib()
            if latents is not None:
                try:
                    g = np.array(latents, dtype=np.float64, order="F", copy=True)
                except (TypeError, ValueError):
                    raise TypeError("`latents` should be of type `ndarray`.")
                if g.ndim == 1:
                    g = g.reshape(-1, 1, order="F")
                if g.ndim != 2 or g.shape != (self._K, B):
                    raise RuntimeError("Initial gamma has wrong dimensionality.")  # lda.cpp:165
                gamma = np.asfortranarray(g)
            else:
                gamma = np.empty((self._K, B), dtype=np.float64, order="F")
                L.trlda_sample_gamma_init(self._K, B, gamma)          # lda.cpp:135
            csr = held.csr
            nnz = len(csr.ids)
            ranks = np.zeros(nnz, dtype=np.int32)
            scores = np.zeros(nnz, dtype=np.float64)
            candidates = np.empty(B, dtype=np.int32)
            _ffi.check(L.trlda_model_heldout_ranks(self._handle, obs.handle, held.handle, gamma.ctypes.data, 1,
                                                   int(max_iter), float(threshold), ranks.ctypes.data,
                                                   scores.ctypes.data if return_scores else None,
                                                   candidates.ctypes.data))
        finally:
            if own_obs:
                obs.close()
            if own_held:
                held.close()
        indptr, words, ranks, scores = _ranks_entries(csr.indptr, csr.ids, ranks, scores, self._V)
        out = (indptr, words, ranks, candidates)
        if return_scores:
            out += (scores,)
        if return_gamma:
            out += (gamma,)
        return out

    def heldout_ranks_gamma(self, gamma, heldout, docs=None, return_scores=False):
        """The ranks of ``heldout_ranks`` for documents given by their ``gamma`` (K x B, every value
        finite and positive, else RuntimeError; not an array, TypeError): no E-step runs and
        nothing is drawn, so any number of topics is taken.  ``heldout`` (a list, ``DocumentList``
        or ``DeviceBatch`` of B documents) holds the words to rank; ``docs`` (the same kinds, B
        documents) gives the seen words.  Without ``docs`` every word is a candidate
        (``candidates == num_words``) and every distinct held-out word with a positive count is
        relevant.  Returns ``(indptr, words, ranks, candidates)`` as ``heldout_ranks`` does, with
        ``return_scores=True`` the scores appended; on the gamma ``heldout_ranks`` returned the
        same bits.  lambda, alpha, eta, the update counters, the model's statistics and the seeded
        stream stay as they are."""
        try:
            g = np.array(gamma, dtype=np.float64, order="F", copy=True)
        except (TypeError, ValueError):
            raise TypeError("`gamma` should be of type `ndarray`.")
        if g.ndim == 1:
            g = g.reshape(-1, 1, order="F")
        if g.ndim != 2 or g.shape[0] != self._K:
            raise RuntimeError("Gamma has wrong dimensionality.")
        if not (np.all(np.isfinite(g)) and np.all(g > 0)):
            raise RuntimeError("Gamma should be finite and positive.")
        g = np.asfortranarray(g)
        B = g.shape[1]
        if len(heldout) != B:
            raise RuntimeError("`heldout` and `gamma` should hold the same number of documents.")
        if docs is not None and len(docs) != B:
            raise RuntimeError("`docs` and `gamma` should hold the same number of documents.")
        candidates = np.empty(B, dtype=np.int32)
        if B == 0:
            out = (np.zeros(1, dtype=np.int64), np.empty(0, dtype=np.int32), np.empty(0, dtype=np.int32), candidates)
            return out + (np.empty(0, dtype=np.float64),) if return_scores else out
        held, own_held = self._batch(heldout)
        try:
            batch, owned = self._batch(docs) if docs is not None else (None, False)
        except BaseException:
            if own_held:
                held.close()
            raise
        L = _ffi.lib()
        ptrs = []
        try:
            self._settle()
            csr = held.csr
            nnz = len(csr.ids)
            ranks = np.zeros(nnz, dtype=np.int32)
            scores = np.zeros(nnz, dtype=np.float64)
            for nbytes in (g.nbytes, ranks.nbytes, scores.nbytes, candidates.nbytes):
                ptr = _ffi.vp()
                _ffi.check(L.trlda_dev_alloc(self._device, max(nbytes, 8), C.byref(ptr)))
                ptrs.append(ptr)
            _ffi.check(L.trlda_dev_upload(self._device, ptrs[0], g.ctypes.data, g.nbytes))
            _ffi.check(L.trlda_model_heldout_ranks_dev(self._handle, None if batch is None else batch.handle,
                                                       held.handle, ptrs[0], B, ptrs[1],
                                                       ptrs[2] if return_scores else None, ptrs[3]))
            _ffi.check(L.trlda_model_synchronize(self._handle))
            if nnz:
                _ffi.check(L.trlda_dev_download(self._device, ranks.ctypes.data, ptrs[1], ranks.nbytes))
                if return_scores:
                    _ffi.check(L.trlda_dev_download(self._device, scores.ctypes.data, ptrs[2], scores.nbytes))
            _ffi.check(L.trlda_dev_download(self._device, candidates.ctypes.data, ptrs[3], candidates.nbytes))
        finally:
            for ptr in ptrs:
                L.trlda_dev_free(self._device, ptr)
            if owned:
                batch.close()
            if own_held:
                held.close()
        indptr, words, ranks, scores = _ranks_entries(csr.indptr, csr.ids, ranks, scores, self._V)
        out = (indptr, words, ranks, candidates)
        return out + (scores,) if return_scores else out

    def ranking_metrics(self, observed, heldout, top_n=(10, 100), latents=None, max_iter=100, threshold=0.001,
                        return_documents=False):
        """The full-ranking figures of the implicit-feedback literature for the recommendations
        against held-out words: ``heldout_ranks(observed, heldout, ...)`` on the GPU, then on the
        host, in float64 with every sum through ``math.fsum``, for document d with relevant ranks
        r_1 < ... < r_R among n candidates

            mean_percentile_rank  mean over all relevant (d, w) of (r - 1) / (n - 1) (0 where n = 1):
                                  0 is best, 0.5 chance (Hu, Koren & Volinsky 2008)
            auc                   1 - sum_j (r_j - j) / (R (n - R)), over documents with R > 0, n > R
            mrr                   1 / r_1
            map                   (1 / R) sum_j j / r_j
            ndcg                  sum_j 1 / log2(1 + r_j) / sum_{j = 1..R} 1 / log2(1 + j)
            recall[N]             #{r_j <= N} / R for every N of ``top_n`` (positive ints, not capped)

        each but the first the mean over the documents with R > 0 (``recall_at``'s rule, and its
        RuntimeError when no document has a relevant word).  Relevance is binary: held-out counts
        only decide positive or not.  Returns a dict of these entries, ``recall`` a dict N -> value;
        with ``return_documents=True`` the entry ``documents`` holds the per-document arrays (NaN
        where a document is left out of a mean).  lambda, alpha, eta and the update counters stay
        as they are."""
        tops = _ranking_tops(top_n)
        indptr, _, ranks, candidates = self.heldout_ranks(observed, heldout, latents=latents, max_iter=max_iter,
                                                          threshold=threshold)
        return _ranking_metrics(indptr, ranks, candidates, tops, return_documents=return_documents)

    # -- nearest documents in topic space (csrc/docindex_kernels.h) ---------------------------------
    def _register_index(self, index):
        import weakref
        if getattr(self, "_indexes", None) is None:
            self._indexes = weakref.WeakSet()
        self._indexes.add(index)

    def document_index(self, measure='hellinger'):
        """An empty ``trlda_amd.DocumentIndex`` for this model: documents are added to it by their
        topic proportions theta = gamma / sum(gamma) and the ``top_n`` nearest of them are found for
        the documents of a batch, on the GPU.  ``measure``: 'hellinger' (default) or 'cosine', case
        does not matter; another string raises ValueError, a non-string TypeError.  The index is
        closed with the model."""
        from ..index import DocumentIndex
        return DocumentIndex(self, measure)

    # -- distances between topics (csrc/topicdist_kernels.h) ---------------------------------------
    def _second_lambda(self, other):
        """(the other model or None, a K2 x V Fortran-ordered lambda or None, K2) for ``other`` of
        ``topic_distances``, checked without any GPU work."""
        if other is None or other is self:
            return None, None, self._K
        if isinstance(other, LDA):
            if other.num_words != self._V:
                raise ValueError("The other model has another number of words.")
            if other.device != self._device:
                raise ValueError("The other model lives on another device.")
            return other, None, other.num_topics
        try:                                             # (a string, a dict: no array; a number: no dimensions)
            arr = np.asarray(other, dtype=np.float64)
        except (TypeError, ValueError):
            arr = None
        if arr is None or arr.ndim == 0:
            raise TypeError("`other` should be None, an LDA model or a K' x V array of lambdas.")
        if arr.ndim != 2 or arr.shape[0] < 1 or arr.shape[1] != self._V:
            raise ValueError("An array `other` should be K' x %d (topics x words)." % self._V)
        if not (np.all(np.isfinite(arr)) and np.all(arr > 0)):
            raise ValueError("Every lambda of `other` should be finite and positive.")
        return None, np.asfortranarray(arr), int(arr.shape[0])

    def topic_distances(self, other=None, measure='hellinger'):
        """Distances between this model's topics and the topics of ``other``: a K x K' float64 array.

        A topic is the distribution ``p_i = lambdas[i] / lambdas[i].sum()`` (E[beta_i], what
        ``top_words`` ranks by); ``q_j`` is the same of the second lambda.  Entry (i, j):

        - ``'hellinger'`` (default): ``sqrt(max(0, 1 - sum_v sqrt(p_iv q_jv)))``, in [0, 1];
        - ``'cosine'``: ``max(0, 1 - sum_v p_iv q_jv / (|p_i| |q_j|))``, in [0, 1];
        - ``'kl'``: ``sum_v p_iv log(p_iv / q_jv)`` in nats, this model's topic first (asymmetric);
        - ``'jensen_shannon'`` (or ``'js'``): ``H(m) - H(p_i) / 2 - H(q_j) / 2`` with
          ``m = (p_i + q_j) / 2``, in nats, at most ln 2 -- the divergence, not its square root.

        Case does not matter; another string raises ValueError, a non-string TypeError.

        ``other`` is None (the model against itself: the diagonal is exactly 0 and the three symmetric
        measures give a bitwise symmetric matrix), another model of any subclass with the same
        ``num_words`` on the same device, or a K' x V array-like of lambdas (finite and positive, e.g.
        the topics a synthetic corpus was drawn from; it is uploaded for the call and not kept).
        Anything else raises TypeError; another number of words or device, or an array of the wrong
        shape or with a non-finite or non-positive entry, ValueError -- all before any GPU work.  A
        *copy* of the model is another model: its diagonal is near 0, not exactly 0.  The models'
        own lambdas are not checked; one set by hand with zeros gives what IEEE arithmetic gives.

        The matrix is formed on the GPU without atomics, in an order that depends on (K, K', V,
        measure) alone: two calls on the same lambdas agree bitwise.  Only the K x K' result is
        copied to the host."""
        code = _topic_measure(measure)                               # (before the model is looked at)
        model, lam, K2 = self._second_lambda(other)
        if getattr(self, "_handle", None) is None or (model is not None and model._handle is None):
            raise RuntimeError("The model has been closed.")
        self._settle()
        if model is not None:
            model._settle()
        out = np.empty((self._K, K2), dtype=np.float64, order="F")
        _ffi.check(_ffi.lib().trlda_model_topic_distances(
            self._handle, None if model is None else model._handle,
            None if lam is None else lam.ctypes.data, K2, code, out.ctypes.data))
        return out

    def match_topics(self, other, measure='hellinger'):
        """``(match, dist)``: for each topic i of this model the topic ``match[i]`` of ``other`` it is
        paired with (int64) and their distance ``dist[i]`` (float64), by greedy one-to-one matching on
        ``topic_distances(other, measure)``: the pairs are taken in the order (distance ascending, i
        ascending, j ascending) and a pair is kept when both its topics are still free.  With more
        topics here than in ``other`` the rows left over get ``match = -1`` and ``dist = inf``.  Not
        the optimal assignment.  ``other=None`` raises ValueError (a model matched with itself is the
        identity); ``other`` and ``measure`` are otherwise those of ``topic_distances``."""
        _topic_measure(measure)
        if other is None:
            raise ValueError("`other` is None: a model matched with itself is the identity.")
        return _greedy_match(self.topic_distances(other, measure))

    # -- topic coherence (Mimno et al. 2011; Bouma 2009; csrc/coherence_kernels.h) -----------------
    def top_words(self, top_n=10):
        """The ``top_n`` word ids of each topic in decreasing order of lambda_kw (the order of
        E[beta_kw] too), equal values by smaller word id first: row k is
        ``np.lexsort((np.arange(V), -lambdas[k]))[:top_n]``.  Returns a K x top_n int32 array.
        ``1 <= top_n <= min(num_words, 100)``, else RuntimeError.  The selection runs on the GPU;
        only the ids come back."""
        top_n = operator.index(top_n)
        if not 1 <= top_n <= min(self._V, 100):
            raise RuntimeError("`top_n` should lie between 1 and min(num_words, 100).")
        self._settle()
        words = np.empty((self._K, top_n), dtype=np.int32)
        _ffi.check(_ffi.lib().trlda_model_top_words(self._handle, top_n, words))
        return words

    def topic_coherence(self, docs, top_n=10, measure='umass', words=None, return_counts=False):
        """Coherence of each topic's top words on a corpus: float64, one value per word list.

        ``docs`` is a batch (a list of documents, ``DocumentList``, ``CSRDocuments`` or a
        ``DeviceBatch`` of this model) or an iterator of batches (anything with ``__next__``, e.g.
        ``load_documents(path, 1000)``; for a list of batches pass ``iter(batches)``), whose counts
        add up on the device.  ``words`` (T x N word ids, each row N >= 2 distinct ids in
        [0, num_words), best first) replaces ``top_words(top_n)``; bad shapes, ids out of range
        and repeated ids raise RuntimeError.

        Document d contains word w when it has an entry (w, c) with c > 0 (repeated entries count
        once).  M is the number of documents (empty ones included), D(w) the number containing w,
        D(w, w') the number containing both.  For a list v_1 .. v_N:

          'umass'  the mean over the pairs l < m of log((D(v_m, v_l) + 1) / D(v_l)), pairs with
                   D(v_l) = 0 left out (NaN if none is left).  Mimno et al.'s sum is this times
                   N (N - 1) / 2.
          'npmi'   the mean over the pairs i < j of -1 if D_ij = 0, +1 if D_ij = M, otherwise
                   (log D_ij + log M - log D_i - log D_j) / (log M - log D_ij).

        The counting and the top-word selection run on the GPU; the per-pair formulas are fp64 on
        the host, pairs added in the order m (j) ascending, then l (i) ascending.  ``measure`` is
        case-insensitive; other values raise ValueError.  With ``return_counts=True`` returns
        ``(coherence, counts)``, counts a dict of ``words`` (T x N int32), ``doc_freq`` (T x N
        int64), ``co_doc_freq`` (T x N x N int64, symmetric, doc_freq on the diagonal) and
        ``num_documents``.  lambda, alpha, eta, the counters and the random stream are left as
        they are."""
        if not isinstance(measure, str) or measure.lower() not in ("umass", "npmi"):
            raise ValueError("`measure` should be either 'umass' or 'npmi'.")
        measure = measure.lower()
        self._settle()
        if words is None:
            top_n = operator.index(top_n)
            if top_n < 2:
                raise RuntimeError("Coherence needs `top_n` of at least 2.")
            words = self.top_words(top_n)
        else:
            try:
                w = np.asarray(words)
            except (TypeError, ValueError):
                raise RuntimeError("`words` should be a two-dimensional array of word ids.")
            if w.ndim != 2 or w.size == 0 or not np.issubdtype(w.dtype, np.integer):
                raise RuntimeError("`words` should be a two-dimensional array of word ids.")
            if ((w < 0) | (w >= self._V)).any():
                raise RuntimeError("Word id out of range in `words`.")
            words = np.ascontiguousarray(w, dtype=np.int32)
        T, N = words.shape
        L = _ffi.lib()
        cooc = _ffi.vp()
        _ffi.check(L.trlda_cooc_create(self._handle, words, T, N, C.byref(cooc)))
        try:
            for part in (docs if hasattr(docs, "__next__") else (docs,)):
                batch, owned = self._batch(part)
                try:
                    _ffi.check(L.trlda_cooc_add(cooc, batch.handle))
                finally:
                    if owned:
                        batch.close()
            doc_freq = np.empty((T, N), dtype=np.int64)
            co = np.empty((T, N, N), dtype=np.int64)
            num_docs = C.c_int64(0)
            _ffi.check(L.trlda_cooc_read(cooc, doc_freq, co, C.byref(num_docs)))
        finally:
            L.trlda_cooc_destroy(cooc)
        coh = _coherence(measure, doc_freq, co, num_docs.value)
        if return_counts:
            return coh, {"words": words, "doc_freq": doc_freq, "co_doc_freq": co,
                         "num_documents": int(num_docs.value)}
        return coh

    # -- spectral initialisation: anchor words from word co-occurrence (csrc/anchor_kernels.h) -----
    def word_cooccurrence(self, docs=None, max_bytes=None):
        """A ``trlda_amd.WordCooccurrence`` for this model's vocabulary: the device-resident matrix Q
        of Arora et al.'s unbiased word co-occurrence estimator, with ``docs`` (a batch or an iterator
        of batches, as ``topic_coherence`` takes them) added when given.  ``max_bytes`` (default
        16 GiB) bounds Q plus its one work copy: a larger vocabulary raises RuntimeError naming the
        bytes needed before anything is allocated.  The accumulator is closed with the model
        (DESIGN.md 3.36)."""
        from ..anchor import DEFAULT_MAX_BYTES, WordCooccurrence
        self._settle()
        cooc = WordCooccurrence(self, DEFAULT_MAX_BYTES if max_bytes is None else max_bytes)
        if docs is not None:
            try:
                cooc.add(docs)
            except Exception:
                cooc.close()
                raise
        return cooc

    def _own_cooc(self, cooc):
        from ..anchor import WordCooccurrence
        if not isinstance(cooc, WordCooccurrence):
            raise RuntimeError("`cooc` should be a WordCooccurrence of this model.")
        if cooc._model is not self:
            raise RuntimeError("The co-occurrence matrix was made for a different model.")
        return cooc._live()

    def anchor_words(self, cooc, num_anchors=None, min_doc_freq=None, return_scores=False):
        """FastAnchorWords on the row-normalised ``Qbar_w = Q_w / sum_v Q_wv`` of ``cooc``:
        ``num_anchors`` (default: the number of topics) int32 word ids in selection order.

        Candidates are the words with ``doc_freq >= min_doc_freq`` (default ``max(2, ceil(0.005 *
        num_documents))``) and a positive row sum; for a matrix loaded without ``doc_freq`` every
        word with a positive row sum is one.  Fewer candidates than anchors raise RuntimeError.
        Round 0 takes the candidate row of the largest squared norm and subtracts it from every
        candidate row; each later round takes the largest squared residual norm, normalises that row
        and removes its component from every candidate row of the work copy (modified Gram-Schmidt).
        Norms and dot products are fixed-order sums of the row alone (``WordCooccurrence.row_sums``
        documents the order); the winner is the first in the order (norm^2 descending, word id
        ascending) and leaves the candidates.  With ``return_scores=True`` returns ``(anchors,
        scores)``, scores a dict of each round's ``winner`` and ``runner_up`` norm^2 (-1 where there
        is no runner-up): near-ties show there.  lambda, alpha, eta, the counters and the random stream
        are left as they are."""
        handle = self._own_cooc(cooc)
        num = self._K if num_anchors is None else operator.index(num_anchors)
        if num < 1:
            raise RuntimeError("`num_anchors` should be positive.")
        if not cooc.has_doc_freq:
            if min_doc_freq is not None:
                raise RuntimeError("The matrix was loaded without `doc_freq`: no threshold applies.")
            min_df = -1
        elif min_doc_freq is None:
            min_df = max(2, -(-5 * cooc.num_documents // 1000))
        else:
            min_df = operator.index(min_doc_freq)
            if min_df < 0:
                raise RuntimeError("`min_doc_freq` should not be negative.")
        ids = np.empty(num, dtype=np.int32)
        score, runner = np.empty(num, dtype=np.float64), np.empty(num, dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_anchor_select(handle, num, min_df, ids, score.ctypes.data,
                                                  runner.ctypes.data))
        if return_scores:
            return ids, {"winner": score, "runner_up": runner}
        return ids

    def recover_topics(self, cooc, anchors, tol=1e-7, max_iter=2000, return_info=False):
        """RecoverL2: for every word ``min over the simplex of |Qbar_w - x' Qbar_S|^2`` with S the
        ``anchors`` (distinct word ids; out of range or repeated ones raise RuntimeError), then
        ``(beta, pi)``: beta, K x V in Fortran order like ``lambdas``, column k of ``x_wk p_w``
        normalised over the words (``p = cooc.word_probabilities()``), and pi, the K column masses.

        ``H = Qbar Qbar_S'`` comes from the staged fp64 tile product over the words in ascending
        chunks and ``G`` is its anchors' rows.  A wave per word runs projected gradient with Nesterov's
        momentum and gradient restart (reset when ``(y - x+) . (x+ - x) > 0``), step ``1 / L`` with
        ``L = 2 max_i sum_j |G_ij|``, from ``x = 1 / K``, with the exact Euclidean projection onto the
        simplex (Michelot's finite iteration), and stops on its own when its Frank-Wolfe gap
        ``x . g - min_k g_k`` is at most ``tol |Qbar_w|^2``, or after ``max_iter`` iterations: a word's
        result depends on its row and the anchors' rows alone.  Words with a zero row get beta = 0.
        With ``return_info=True`` returns ``(beta, pi, info)``, info a dict of ``x`` (V x K),
        ``iterations`` (int32 per word) and ``gaps`` (the final gap over ``|Qbar_w|^2``)."""
        handle = self._own_cooc(cooc)
        try:
            a = np.asarray(anchors)
        except (TypeError, ValueError):
            raise RuntimeError("`anchors` should be a one-dimensional array of word ids.")
        if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
            raise RuntimeError("`anchors` should be a one-dimensional array of word ids.")
        if a.min() < 0 or a.max() >= self._V:
            raise RuntimeError("Anchor word out of range.")
        if len(np.unique(a)) != len(a):
            raise RuntimeError("An anchor word occurs twice.")
        a = np.ascontiguousarray(a, dtype=np.int32)
        A, V = len(a), self._V
        tol = float(tol)
        max_iter = operator.index(max_iter)
        if not tol >= 0.0 or max_iter < 1:
            raise RuntimeError("`tol` should not be negative and `max_iter` at least 1.")
        beta = np.empty((A, V), dtype=np.float64, order="F")
        pi = np.empty(A, dtype=np.float64)
        x = np.empty((V, A), dtype=np.float64)
        iters = np.empty(V, dtype=np.int32)
        gaps = np.empty(V, dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_anchor_recover(handle, a, A, tol, max_iter, beta.ctypes.data,
                                                   pi.ctypes.data, x.ctypes.data, iters.ctypes.data,
                                                   gaps.ctypes.data))
        if return_info:
            return beta, pi, {"x": x, "iterations": iters, "gaps": gaps}
        return beta, pi

    def initialize_spectral(self, docs_or_cooc, strength=None, **kw):
        """Sets ``lambda_kw = eta + (strength * pi_k) * beta_kw`` from the anchor words of a corpus:
        ``word_cooccurrence`` (unless a ``WordCooccurrence`` is given), ``anchor_words`` with K
        anchors and ``recover_topics``, in that order; ``strength`` defaults to the accumulator's
        ``num_tokens`` -- a matrix loaded with ``from_matrix`` has counted none and needs ``strength``
        given (RuntimeError otherwise).  Keywords ``min_doc_freq``, ``tol``, ``max_iter`` and ``max_bytes`` go to the
        stage that takes them.  Returns the anchors.  alpha, eta and the counters are left alone and
        nothing is drawn from the random stream: the same corpus gives the same lambda."""
        from ..anchor import WordCooccurrence
        unknown = set(kw) - {"min_doc_freq", "tol", "max_iter", "max_bytes"}
        if unknown:
            raise TypeError("initialize_spectral() got an unexpected keyword argument %r" % sorted(unknown)[0])
        self._settle()
        owned = not isinstance(docs_or_cooc, WordCooccurrence)
        cooc = self.word_cooccurrence(docs_or_cooc, kw.get("max_bytes")) if owned else docs_or_cooc
        try:
            if strength is None:
                strength = cooc.num_tokens
                if strength == 0:
                    raise RuntimeError("The accumulator has counted no tokens (a loaded matrix, or no "
                                       "document of two tokens): give `strength`.")
            strength = float(strength)
            if not (strength > 0.0 and np.isfinite(strength)):
                raise RuntimeError("`strength` should be positive.")
            anchors = self.anchor_words(cooc, min_doc_freq=kw.get("min_doc_freq"))
            beta, pi = self.recover_topics(cooc, anchors, tol=kw.get("tol", 1e-7),
                                           max_iter=kw.get("max_iter", 2000))
        finally:
            if owned:
                cooc.close()
        self.lambdas = self._eta + (strength * pi)[:, None] * beta
        return anchors

    # -- relevance, saliency and topic prevalence (csrc/relevance_kernels.h) -----------------------
    def _rank_top_n(self, top_n):
        top_n = operator.index(top_n)
        if not 1 <= top_n <= min(self._V, 100):
            raise RuntimeError("`top_n` should lie between 1 and min(num_words, 100).")
        return top_n

    def _topic_weights(self, topic_weights):
        """None, or the weights as K contiguous float64 (checked; the library normalises them)."""
        if topic_weights is None:
            return None
        try:
            w = np.array(topic_weights, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise RuntimeError("`topic_weights` should be an array of num_topics weights.")
        if w.size != self._K:
            raise RuntimeError("`topic_weights` should hold num_topics weights.")
        if not (np.all(np.isfinite(w)) and np.all(w > 0)):
            raise RuntimeError("`topic_weights` should be finite and positive.")
        return np.ascontiguousarray(w)

    def _open_handle(self):
        if getattr(self, "_handle", None) is None:
            raise RuntimeError("The model has been closed.")
        self._settle()
        return self._handle

    def relevant_words(self, top_n=10, weight=0.6, topic_weights=None, return_scores=False):
        """The ``top_n`` word ids of each topic ranked by relevance (Sievert & Shirley 2014, the
        ranking of LDAvis): with ``beta_kw = lambdas[k, w] / lambdas[k].sum()`` and the marginal
        word probability ``p_w = sum_k pi_k beta_kw``,

            r_kw = weight * log(beta_kw) + (1 - weight) * log(beta_kw / p_w),

        a blend of a word's probability in the topic and its lift over the corpus.  ``weight = 1``
        ranks as ``top_words`` does; smaller weights push words that every topic holds down the
        lists (0.6 is the value the paper's user study arrived at).  Returns a K x top_n int32
        array, best first, equal values by smaller word id: row k is
        ``np.lexsort((np.arange(V), -r[k]))[:top_n]``; with ``return_scores=True`` also the K x
        top_n float64 r_kw.  The lists go straight into ``topic_coherence(words=...)``.

        ``topic_weights`` (pi): None weighs each topic by its share of lambda's mass,
        ``lambdas[k].sum() / lambdas.sum()``; else K finite, positive weights (normalised to sum
        1), e.g. ``topic_prevalence(docs)``.  ``1 <= top_n <= min(num_words, 100)`` and ``0 <=
        weight <= 1``, else RuntimeError, as for weights of the wrong length, not finite or not
        positive.  A lambda with an entry <= 0 or not finite raises RuntimeError.  Everything runs on
        the GPU (one pass over lambda by columns, then ``top_words``' selection); only the result
        comes back, and two calls agree bitwise.  lambda, alpha, eta, the counters and the seeded
        stream stay as they are."""
        top_n = self._rank_top_n(top_n)
        try:
            weight = float(weight)
        except (TypeError, ValueError):
            raise RuntimeError("`weight` should be a number between 0 and 1.")
        if not 0.0 <= weight <= 1.0:
            raise RuntimeError("`weight` should lie between 0 and 1.")
        pi = self._topic_weights(topic_weights)
        handle = self._open_handle()
        words = np.empty((self._K, top_n), dtype=np.int32)
        scores = np.empty((self._K, top_n), dtype=np.float64) if return_scores else None
        _ffi.check(_ffi.lib().trlda_model_relevant_words(
            handle, top_n, weight, None if pi is None else pi.ctypes.data, words.ctypes.data,
            None if scores is None else scores.ctypes.data))
        if return_scores:
            return words, scores
        return words

    def word_statistics(self, topic_weights=None):
        """``(p_w, distinctiveness, saliency)``, three float64 arrays of length V (Chuang, Manning &
        Heer 2012): the marginal word probability ``p_w = sum_k pi_k beta_kw``; the distinctiveness
        ``D_w = sum_k p(k | w) log(p(k | w) / pi_k)`` with ``p(k | w) = pi_k beta_kw / p_w`` -- the
        Kullback-Leibler divergence of a word's topics from the topic weights, >= 0, in nats; and the
        saliency ``S_w = p_w D_w``, which sums to the mutual information of topic and word (at most
        log K).  ``topic_weights`` and the errors are those of ``relevant_words``.  Formed on the GPU
        in one pass over lambda; 3 V numbers come back."""
        pi = self._topic_weights(topic_weights)
        handle = self._open_handle()
        p, d, s = (np.empty(self._V, dtype=np.float64) for _ in range(3))
        _ffi.check(_ffi.lib().trlda_model_word_stats(
            handle, None if pi is None else pi.ctypes.data, p.ctypes.data, d.ctypes.data, s.ctypes.data))
        return p, d, s

    def salient_words(self, top_n=30, topic_weights=None):
        """``(words, saliency)``: the ``top_n`` word ids of the vocabulary in decreasing saliency
        (``word_statistics``), equal values by smaller word id first, int32, and their saliency,
        float64 -- the terms that say most about which topic they came from.  ``topic_weights`` and
        the errors are those of ``relevant_words``."""
        top_n = self._rank_top_n(top_n)
        pi = self._topic_weights(topic_weights)
        handle = self._open_handle()
        words = np.empty(top_n, dtype=np.int32)
        sal = np.empty(top_n, dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_model_salient_words(
            handle, top_n, None if pi is None else pi.ctypes.data, words.ctypes.data, sal.ctypes.data))
        return words, sal

    # -- the words nearest a word in topic space (csrc/wordsim_kernels.h) --------------------------
    def _word_ids(self, words):
        """The query words as B contiguous int32 ids (a single int: one query)."""
        if isinstance(words, np.ndarray):
            if words.dtype.kind not in "iu":
                raise TypeError("`words` should hold integer word ids.")
            ids = [int(w) for w in words.reshape(-1)]
        else:
            try:
                ids = [operator.index(words)]
            except TypeError:
                try:
                    ids = [operator.index(w) for w in words]
                except TypeError:
                    raise TypeError("`words` should be a word id or a sequence of word ids.")
        if any(not 0 <= w < self._V for w in ids):
            raise RuntimeError("Word id outside [0, num_words).")
        return np.array(ids, dtype=np.int32)

    def _wordsim_top_n(self, top_n, exclude_self):
        top_n = operator.index(top_n)
        if exclude_self:
            if not 1 <= top_n <= min(self._V - 1, 100):
                raise RuntimeError("`top_n` should lie between 1 and min(num_words - 1, 100).")
        elif not 1 <= top_n <= min(self._V, 100):
            raise RuntimeError("`top_n` should lie between 1 and min(num_words, 100).")
        return top_n

    @staticmethod
    def _wordsim_result(ids, sim, measure, return_similarity):
        if return_similarity:
            return ids, sim
        rest = np.maximum(0.0, 1.0 - sim)
        return ids, (rest if measure else np.sqrt(rest))

    def similar_words(self, words, top_n=10, measure="hellinger", topic_weights=None, exclude_self=True,
                      return_similarity=False):
        """The ``top_n`` words the model treats most like each of ``words`` (a word id or a
        sequence of B ids): every word is the distribution over topics ``p(k | w) = pi_k beta_kw /
        p_w`` (``word_statistics``), and two words are compared as ``DocumentIndex`` compares two
        documents -- ``measure='hellinger'`` (default) by the Bhattacharyya coefficient ``s = sum_k
        sqrt(p(k | q) p(k | w))`` with distance ``sqrt(max(0, 1 - s))``, ``measure='cosine'`` by the
        cosine ``s`` of ``pi_k beta_kq`` and ``pi_k beta_kw`` with distance ``max(0, 1 - s)``.
        Returns ``(ids, dist)``, B x top_n int32 and float64, nearest first, equal similarities by
        smaller word id; with ``return_similarity=True`` the second array holds ``s``.  With
        ``exclude_self`` (default) a query word is left out of its own list, by id: another word
        with an equal column of lambda stays in, at distance 0.

        ``topic_weights`` (pi) as for ``relevant_words``.  ``1 <= top_n <= min(num_words - 1, 100)``
        (``num_words`` without ``exclude_self``), else RuntimeError; a measure that is no string is a
        TypeError, an unknown one a ValueError; a word id that is no integer is a TypeError, one
        outside the vocabulary a RuntimeError, as is a lambda with an entry <= 0 or not finite.  The
        V x B x K product runs on the GPU's matrix cores against lambda where it lies; only the
        lists come back.  A query's list does not depend on the other queries, ``s(q, w)`` and
        ``s(w, q)`` are the same bits, and two calls agree bitwise.  lambda, alpha, eta, the counters
        and the seeded stream stay as they are."""
        ids = self._word_ids(words)
        top_n = self._wordsim_top_n(top_n, exclude_self)
        measure = _measure(measure)
        pi = self._topic_weights(topic_weights)
        B = ids.size
        out = np.empty((B, top_n), dtype=np.int32)
        sim = np.empty((B, top_n), dtype=np.float64)
        if B:
            handle = self._open_handle()
            _ffi.check(_ffi.lib().trlda_model_similar_words(
                handle, ids.ctypes.data, B, top_n, measure, None if pi is None else pi.ctypes.data,
                1 if exclude_self else 0, out.ctypes.data, sim.ctypes.data))
        return self._wordsim_result(out, sim, measure, return_similarity)

    def words_near(self, proportions, top_n=10, measure="hellinger", topic_weights=None, return_similarity=False):
        """The ``top_n`` words nearest points of the topic simplex: ``proportions`` is K x B or a
        length-K vector of finite, positive values (each column is normalised) -- a document's
        ``gamma``, a centroid of ``DocumentIndex.cluster``, a topic.  The measures, the result and
        the errors are those of ``similar_words``; there is no self to leave out, so ``top_n`` may
        reach ``min(num_words, 100)``.  Proportions that are not finite or not positive raise
        RuntimeError."""
        try:
            g = np.array(proportions, dtype=np.float64, order="F", copy=True)
        except (TypeError, ValueError):
            raise TypeError("`proportions` should be of type `ndarray`.")
        if g.ndim == 1:
            g = g.reshape(-1, 1, order="F")
        if g.ndim != 2 or g.shape[0] != self._K:
            raise RuntimeError("Proportions have wrong dimensionality.")
        g = np.asfortranarray(g)
        top_n = self._wordsim_top_n(top_n, False)
        measure = _measure(measure)
        pi = self._topic_weights(topic_weights)
        if not (np.all(np.isfinite(g)) and np.all(g > 0)):
            raise RuntimeError("Proportions should be finite and positive.")
        B = g.shape[1]
        out = np.empty((B, top_n), dtype=np.int32)
        sim = np.empty((B, top_n), dtype=np.float64)
        if B:
            handle = self._open_handle()
            _ffi.check(_ffi.lib().trlda_model_similar_words_rows(
                handle, g.ctypes.data, B, top_n, measure, None if pi is None else pi.ctypes.data,
                out.ctypes.data, sim.ctypes.data))
        return self._wordsim_result(out, sim, measure, return_similarity)

    def word_topic_proportions(self, words, topic_weights=None):
        """``p(k | w)`` of each of ``words`` (a word id or a sequence of B ids): K x B float64 in
        Fortran order, each column summing to 1 -- the distributions ``similar_words`` compares.
        ``topic_weights`` and the errors as there."""
        ids = self._word_ids(words)
        pi = self._topic_weights(topic_weights)
        B = ids.size
        out = np.empty((self._K, B), dtype=np.float64, order="F")
        if B:
            handle = self._open_handle()
            _ffi.check(_ffi.lib().trlda_model_word_topic_proportions(
                handle, ids.ctypes.data, B, None if pi is None else pi.ctypes.data, out.ctypes.data))
        return out

    def _prevalence(self, weight_by_length, feed):
        """Runs ``feed(acc)`` and returns the normalised weights; ``acc()`` is the accumulator, made
        when first asked for -- after the first batch has been checked, so that a batch of another
        model or a gamma of the wrong shape raises before anything is allocated."""
        handle = self._open_handle()
        L = _ffi.lib()
        made = _ffi.vp()

        def acc():
            if not made:
                _ffi.check(L.trlda_prevalence_create(handle, 1 if weight_by_length else 0, C.byref(made)))
            return made

        try:
            feed(acc)
            pi = np.empty(self._K, dtype=np.float64)
            num_docs = C.c_int64(0)
            _ffi.check(L.trlda_prevalence_read(acc(), pi.ctypes.data, C.byref(num_docs)))
        finally:
            if made:
                L.trlda_prevalence_destroy(made)
        return pi

    def _corpus_gamma0(self, docs, latents):
        """``latents`` of a call that runs the E-step over ``docs`` (a batch or an iterator of
        batches) as a K x B Fortran array, or None; checked before anything is drawn or uploaded."""
        _ffi.check_vi_topics(self._K)                               # (before the draw and the upload)
        if latents is None:
            return None
        try:
            g0 = np.array(latents, dtype=np.float64, order="F", copy=True)
        except (TypeError, ValueError):
            raise TypeError("`latents` should be of type `ndarray`.")
        if g0.ndim == 1:
            g0 = g0.reshape(-1, 1, order="F")
        if g0.ndim != 2 or g0.shape[0] != self._K:
            raise RuntimeError("Initial gamma has wrong dimensionality.")  # lda.cpp:165
        # (one batch: its size is known before anything is uploaded or run)
        if not hasattr(docs, "__next__") and g0.shape[1] != len(docs):
            raise RuntimeError("Initial gamma has wrong dimensionality.")
        return g0

    def _corpus_estep(self, docs, g0, add):
        """``add(batch, gamma0)`` for every batch of ``docs``, gamma0 the batch's columns of ``g0``
        or a draw from the seeded stream as ``update_variables`` draws it."""
        L = _ffi.lib()
        at = 0
        for part in (docs if hasattr(docs, "__next__") else (docs,)):
            batch, owned = self._batch(part)
            try:
                B = len(batch)
                if g0 is not None:
                    if at + B > g0.shape[1]:
                        raise RuntimeError("Initial gamma has wrong dimensionality.")
                    gamma = np.asfortranarray(g0[:, at:at + B])
                else:
                    gamma = np.empty((self._K, B), dtype=np.float64, order="F")
                    L.trlda_sample_gamma_init(self._K, B, gamma)  # lda.cpp:135
                add(batch, gamma)
                at += B
            finally:
                if owned:
                    batch.close()
        if g0 is not None and at != g0.shape[1]:
            raise RuntimeError("Initial gamma has wrong dimensionality.")

    def topic_prevalence(self, docs, latents=None, max_iter=100, threshold=0.001, weight_by_length=True):
        """The weight of each topic in a corpus: a float64 array of K that sums to 1,

            pi_k ~ sum_d N_d gamma_dk / sum_j gamma_dj,

        ``N_d`` the sum of document d's positive counts (``weight_by_length=False``: 1, every
        document counts the same); a document without a positive count is skipped.  gamma comes
        from ``update_variables``' E-step on each batch (lambda fixed; ``latents`` as gamma0, its
        columns in the order of the documents, else a random gamma drawn from the seeded stream as
        ``update_variables`` draws it); only K sums stay on the device between batches.

        ``docs`` is what ``topic_coherence`` takes: a batch (a list of documents, ``DocumentList``,
        ``CSRDocuments`` or a ``DeviceBatch`` of this model) or an iterator of batches.  The sum
        runs over the documents in order, one addition per document per topic, so the result does
        not depend on how the corpus is cut into batches beyond what gamma itself does.  No
        contributing document, or a batch of another model, raises RuntimeError.  The result plugs
        into ``topic_weights=``.  lambda, alpha, eta and the counters stay as they are (DESIGN.md
        3.23)."""
        g0 = self._corpus_gamma0(docs, latents)
        L = _ffi.lib()

        def feed(acc):
            self._corpus_estep(docs, g0, lambda batch, gamma: _ffi.check(L.trlda_prevalence_add(
                acc(), batch.handle, gamma.ctypes.data, int(max_iter), float(threshold))))

        return self._prevalence(weight_by_length, feed)

    def topic_prevalence_gamma(self, gamma, docs, weight_by_length=True):
        """``topic_prevalence`` for documents given by their ``gamma`` (K x B, every value finite
        and positive, else RuntimeError; not an array, TypeError): no E-step runs and nothing is
        drawn, so any number of topics is taken and the ``alpha + n`` of a Gibbs or CVB0 run serves
        as well.  ``docs`` (one batch of B documents) gives the lengths N_d and which documents are
        skipped.  On the gamma ``update_variables`` returns, bitwise the result of
        ``topic_prevalence``."""
        try:
            g = np.array(gamma, dtype=np.float64, order="F", copy=True)
        except (TypeError, ValueError):
            raise TypeError("`gamma` should be of type `ndarray`.")
        if g.ndim == 1:
            g = g.reshape(-1, 1, order="F")
        if g.ndim != 2 or g.shape[0] != self._K:
            raise RuntimeError("Gamma has wrong dimensionality.")
        if not (np.all(np.isfinite(g)) and np.all(g > 0)):
            raise RuntimeError("Gamma should be finite and positive.")
        g = np.asfortranarray(g)
        if len(docs) != g.shape[1]:
            raise RuntimeError("`docs` and `gamma` should hold the same number of documents.")
        L = _ffi.lib()

        def feed(acc):
            batch, owned = self._batch(docs)
            ptr = _ffi.vp()
            try:
                if g.shape[1] == 0:
                    return
                _ffi.check(L.trlda_dev_alloc(self._device, g.nbytes, C.byref(ptr)))
                _ffi.check(L.trlda_dev_upload(self._device, ptr, g.ctypes.data, g.nbytes))
                _ffi.check(L.trlda_prevalence_add_dev(acc(), batch.handle, ptr))
                _ffi.check(L.trlda_model_synchronize(self._handle))
            finally:
                if ptr:
                    L.trlda_dev_free(self._device, ptr)
                if owned:
                    batch.close()

        return self._prevalence(weight_by_length, feed)

    # -- per-topic diagnostics (csrc/diagnostics_kernels.h) -----------------------------------------
    def topic_word_diagnostics(self, top_n=10, topic_weights=None, words=None):
        """What lambda alone says about each topic's quality, the word-side columns of MALLET's
        diagnostics file: a dict of float64 arrays of length K (``beta_kw = lambdas[k, w] /
        lambdas[k].sum()``, ``p_w`` the marginal word probability of ``word_statistics``):

          ``eff_num_words``  ``1 / sum_w beta_kw**2``: from 1 (one word) to V (uniform).
          ``word_entropy``   ``H_k = -sum_w beta_kw log beta_kw``, nats.
          ``uniform_dist``   ``log V - H_k``, the divergence KL(beta_k || uniform); near 0: a topic
                             that says nothing.
          ``corpus_dist``    KL(beta_k || p); near 0: a topic that repeats the corpus' word
                             frequencies.
          ``exclusivity``    the mean over the topic's listed words of ``beta_kw / sum_j beta_jw``:
                             1 when no other topic holds them, 1 / K when every topic does.
          ``top_words``      the K x top_n int32 lists used: ``top_words(top_n)``, or ``words`` (K x
                             top_n ids in [0, num_words), distinct within a row, e.g. from
                             ``relevant_words``; else RuntimeError).

        ``topic_weights``, ``top_n`` and their errors are those of ``relevant_words``, as is the
        RuntimeError for a lambda with an entry <= 0 or not finite.  Everything is reduced on the
        GPU in an order that depends on K and V alone (5 K numbers come back; two calls agree
        bitwise); lambda, alpha, eta, the counters and the seeded stream stay as they are
        (DESIGN.md 3.31)."""
        pi = self._topic_weights(topic_weights)
        if words is None:
            top_n = self._rank_top_n(top_n)
        else:
            try:
                w = np.asarray(words)
            except (TypeError, ValueError):
                raise RuntimeError("`words` should be a num_topics x top_n array of word ids.")
            if w.ndim != 2 or w.shape[0] != self._K or not np.issubdtype(w.dtype, np.integer):
                raise RuntimeError("`words` should be a num_topics x top_n array of word ids.")
            top_n = self._rank_top_n(w.shape[1])
            if ((w < 0) | (w >= self._V)).any():
                raise RuntimeError("Word id out of range in `words`.")
            if (np.diff(np.sort(w, axis=1), axis=1) == 0).any():
                raise RuntimeError("A row of `words` holds a word twice.")
            words = np.ascontiguousarray(w, dtype=np.int32)
        handle = self._open_handle()
        if words is None:
            words = self.top_words(top_n)
        out = [np.empty(self._K, dtype=np.float64) for _ in range(5)]
        _ffi.check(_ffi.lib().trlda_model_word_diagnostics(
            handle, top_n, None if pi is None else pi.ctypes.data, words.ctypes.data,
            *[x.ctypes.data for x in out]))
        keys = ("eff_num_words", "word_entropy", "uniform_dist", "corpus_dist", "exclusivity")
        res = dict(zip(keys, out))
        res["top_words"] = words
        return res

    def _topic_document_diagnostics(self, weight_by_length, high, low, feed):
        """``_prevalence`` for the diagnostics accumulator: runs ``feed(acc)`` and reads it."""
        handle = self._open_handle()
        L = _ffi.lib()
        made = _ffi.vp()

        def acc():
            if not made:
                _ffi.check(L.trlda_topicdiag_create(handle, 1 if weight_by_length else 0, high, low,
                                                    C.byref(made)))
            return made

        K = self._K
        try:
            feed(acc)
            tokens, entropy = np.empty(K, dtype=np.float64), np.empty(K, dtype=np.float64)
            rank1, above, present = (np.empty(K, dtype=np.int64) for _ in range(3))
            num_docs = C.c_int64(0)
            _ffi.check(L.trlda_topicdiag_read(acc(), tokens.ctypes.data, entropy.ctypes.data, rank1.ctypes.data,
                                              above.ctypes.data, present.ctypes.data, C.byref(num_docs)))
        finally:
            if made:
                L.trlda_topicdiag_destroy(made)
        ratio = np.full(K, np.nan)
        some = present > 0
        ratio[some] = above[some] / present[some]
        return {"tokens": tokens, "document_entropy": entropy, "rank_1_docs": rank1, "docs_high": above,
                "docs_low": present, "allocation_ratio": ratio, "num_docs": int(num_docs.value)}

    @staticmethod
    def _diagnostic_thresholds(high, low):
        try:
            high, low = float(high), float(low)
        except (TypeError, ValueError):
            raise RuntimeError("`high` and `low` should be numbers with 0 <= low < high < 1.")
        if not 0.0 <= low < high < 1.0:
            raise RuntimeError("`high` and `low` should satisfy 0 <= low < high < 1.")
        return high, low

    def topic_document_diagnostics(self, docs, latents=None, max_iter=100, threshold=0.001,
                                   weight_by_length=True, high=0.5, low=0.02):
        """What a corpus says about each topic's quality, the document-side columns of MALLET's
        diagnostics file.  gamma comes from the E-step on each batch, ``docs``, ``latents``,
        ``max_iter``, ``threshold``, ``weight_by_length`` and the skipped documents exactly as for
        ``topic_prevalence``.  With ``theta_dk = gamma_dk / sum_j gamma_dj`` and ``a_dk = N_d
        theta_dk``, a dict of arrays of length K:

          ``tokens``            ``T_k = sum_d a_dk``, float64: the tokens the topic explains
                                (``topic_prevalence`` is ``tokens / tokens.sum()``, bitwise).
          ``document_entropy``  the entropy of ``p(d | k) = a_dk / T_k``, nats, float64: 0 for a
                                topic that lives in one document, ``log(num_docs)`` for one spread
                                evenly.
          ``rank_1_docs``       int64: the documents whose largest gamma_dk is topic k (ties go to
                                the smaller k); sums to ``num_docs``.
          ``docs_high``, ``docs_low``  int64: the documents with ``theta_dk > high`` and ``> low``.
          ``allocation_ratio``  ``docs_high / docs_low``, float64, NaN where ``docs_low`` is 0: small
                                for a topic that is present in many documents and dominant in few.
          ``num_docs``          the documents that contributed (an int).

        ``0 <= low < high < 1``, else RuntimeError before anything is allocated; no contributing
        document raises RuntimeError.  2 K sums and 3 K counters stay on the device between
        batches, one addition per document each, so any cut of the corpus into batches gives the
        same bits on the same gamma.  Like ``topic_prevalence`` the E-step overwrites the model's
        gamma and statistics and draws only the gamma0 of batches without ``latents``; lambda,
        alpha, eta and the counters stay as they are."""
        high, low = self._diagnostic_thresholds(high, low)
        g0 = self._corpus_gamma0(docs, latents)
        L = _ffi.lib()

        def feed(acc):
            self._corpus_estep(docs, g0, lambda batch, gamma: _ffi.check(L.trlda_topicdiag_add(
                acc(), batch.handle, gamma.ctypes.data, int(max_iter), float(threshold))))

        return self._topic_document_diagnostics(weight_by_length, high, low, feed)

    def topic_document_diagnostics_gamma(self, gamma, docs, weight_by_length=True, high=0.5, low=0.02):
        """``topic_document_diagnostics`` for documents given by their ``gamma`` (K x B, finite and
        positive, as for ``topic_prevalence_gamma``): no E-step runs, nothing is drawn and the
        model's gamma and statistics are left alone.  ``docs`` is a batch of B documents or an
        iterator of batches that hold B documents together, gamma's columns in their order.  On
        the gamma ``update_variables`` returns, bitwise the result of
        ``topic_document_diagnostics``."""
        high, low = self._diagnostic_thresholds(high, low)
        try:
            g = np.array(gamma, dtype=np.float64, order="F", copy=True)
        except (TypeError, ValueError):
            raise TypeError("`gamma` should be of type `ndarray`.")
        if g.ndim == 1:
            g = g.reshape(-1, 1, order="F")
        if g.ndim != 2 or g.shape[0] != self._K:
            raise RuntimeError("Gamma has wrong dimensionality.")
        if not (np.all(np.isfinite(g)) and np.all(g > 0)):
            raise RuntimeError("Gamma should be finite and positive.")
        streamed = hasattr(docs, "__next__")
        if not streamed and len(docs) != g.shape[1]:
            raise RuntimeError("`docs` and `gamma` should hold the same number of documents.")
        L = _ffi.lib()

        def feed(acc):
            at = 0
            for part in (docs if streamed else (docs,)):
                batch, owned = self._batch(part)
                ptr = _ffi.vp()
                try:
                    B = len(batch)
                    if at + B > g.shape[1]:
                        raise RuntimeError("`docs` and `gamma` should hold the same number of documents.")
                    if B:
                        cols = np.asfortranarray(g[:, at:at + B])
                        _ffi.check(L.trlda_dev_alloc(self._device, cols.nbytes, C.byref(ptr)))
                        _ffi.check(L.trlda_dev_upload(self._device, ptr, cols.ctypes.data, cols.nbytes))
                        _ffi.check(L.trlda_topicdiag_add_dev(acc(), batch.handle, ptr))
                        _ffi.check(L.trlda_model_synchronize(self._handle))
                    at += B
                finally:
                    if ptr:
                        L.trlda_dev_free(self._device, ptr)
                    if owned:
                        batch.close()
            if at != g.shape[1]:
                raise RuntimeError("`docs` and `gamma` should hold the same number of documents.")

        return self._topic_document_diagnostics(weight_by_length, high, low, feed)

    def topic_diagnostics(self, docs=None, **kw):
        """The per-topic diagnostics table: ``topic_word_diagnostics`` alone when ``docs`` is None,
        else its dict merged with ``topic_document_diagnostics(docs, ...)``'s.  Keyword arguments
        go to the side that takes them (``top_n``, ``topic_weights``, ``words``: the word side; the
        others: the document side); an unknown one is a TypeError."""
        word_kw = {k: kw.pop(k) for k in ("top_n", "topic_weights", "words") if k in kw}
        if docs is None and kw:
            raise TypeError("Unexpected keyword arguments without `docs`: %s." % ", ".join(sorted(kw)))
        res = self.topic_word_diagnostics(**word_kw)
        if docs is not None:
            res.update(self.topic_document_diagnostics(docs, **kw))
        return res

    # -- device reductions for the empirical-Bayes steps (csrc/eb_kernels.h) ----------------
    def _psi_gamma_diff_device(self, num_docs):
        """sum_d (psi(gamma_dk) - psi(sum_k gamma_dk)) over the gamma the last update / resident
        E-step left on the device (onlinelda.cpp:123-128, batchlda.cpp:72-74): K numbers."""
        out = np.empty(self._K, dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_model_eb_gamma_stats(self._handle, int(num_docs), None, out))
        return out

    def _lambda_psi_stats_device(self):
        """(sum_kw psi(lambda_kw), row sums of lambda): onlinelda.cpp:152-154, batchlda.cpp:152."""
        total = C.c_double(0.)
        rowsums = np.empty(self._K, dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_model_eb_lambda_stats(self._handle, C.byref(total), rowsums))
        return total.value, rowsums

    def _resident_estep(self, batch, max_iter, threshold=0.001):
        """updateVariables(documents, parameters) from a fresh random gamma, results left on the
        device (onlinelda.cpp:118-120)."""
        _ffi.check(_ffi.lib().trlda_model_estep_resident(self._handle, batch.handle, int(max_iter),
                                                         float(threshold)))

    # -- sampling documents (ldainterface.cpp:218-262 -> lda.cpp:88-115) ------------------------
    def sample(self, num_documents, length, return_theta=False):
        """Samples ``num_documents`` documents from the model: topics beta_k ~ Dirichlet(lambda_k)
        once per call, then per document a length ~ Poisson(``length``), theta ~ Dirichlet(alpha)
        and per token a topic ~ theta and a word ~ beta of that topic (csrc/sample_kernels.h).

        Returns a list of documents, each a list of ``(word id, 1)`` tuples in token order (a
        ``DocumentList``, which ``update_parameters`` takes as it is); with ``return_theta=True``
        ``(documents, theta K x num_documents)``.  Deviations from the reference:
        the random numbers are Philox4x32-10 keyed by two draws of the seeded stream, so
        ``trlda.seed`` makes a call reproducible, and the first n documents do not depend on how
        many more are asked for; lengths are drawn by inversion, correct for any ``length``."""
        num_documents = operator.index(num_documents)                # the binding's "ii"
        length = operator.index(length)
        if num_documents < 0:
            raise RuntimeError("The number of documents should not be negative.")
        if length < 0:
            raise RuntimeError("The length should not be negative.")
        self._settle()
        L = _ffi.lib()
        key = C.c_uint64(0)
        _ffi.check(L.trlda_rng_draw_key(C.byref(key)))
        indptr = np.empty(num_documents + 1, dtype=np.int32)
        _ffi.check(L.trlda_sample_lengths(num_documents, float(length), key.value, indptr))
        ids = np.empty(int(indptr[-1]), dtype=np.int32)
        theta = np.empty((self._K, num_documents), dtype=np.float64, order="F") if return_theta else None
        _ffi.check(L.trlda_model_sample_host(self._handle, num_documents, indptr, ids,
                                             None if theta is None else theta.ctypes.data, key.value))
        docs = DocumentList(CSRDocuments(indptr, ids, np.ones(len(ids), dtype=np.int32)))
        if return_theta:
            return docs, theta
        return docs

    def __str__(self):                                               # ldainterface.cpp:473-490
        self._settle()
        return "Number of topics: %d\nEta: %.4g\nAlpha: %.4g, %.4g (min, max)\n" % (
            self._K, self._eta, self._alpha.min(), self._alpha.max())


class OnlineLDA(LDA):
    """Online trust-region LDA (reference src/onlinelda.cpp, onlineldainterface.cpp).

        >>> model = OnlineLDA(num_words=7000, num_topics=100, num_documents=10000,
        ...                   alpha=.1, eta=.3)

    ``alpha`` can be a scalar or an array with one entry for each topic.
    """

    def __init__(self, num_words, num_topics, num_documents, alpha=.1, eta=.3, kappa_=0.,
                 tau_=0., device=None):
        # kappa_ / tau_ are accepted and ignored (old pickles; onlineldainterface.cpp:50-52)
        self._num_documents = int(num_documents)
        self._update_count = 0
        # adaptive learning rate state (onlinelda.cpp:28-31; not pickled, like the reference)
        self._ada_tau = 1000.
        self._ada_rho = 1. / self._ada_tau
        self._ada_sq_norm = 1.
        self._setup(num_words, num_topics, alpha, eta, device)

    def _default_num_documents(self):
        return self._num_documents                                   # onlinelda.cpp:184-191

    @property
    def num_documents(self):
        return self._num_documents

    @num_documents.setter
    def num_documents(self, value):
        value = int(value)
        if value < 0:                                                # onlinelda.h:57-58
            raise RuntimeError("The number of documents should not be negative.")
        self._num_documents = value

    @property
    def update_count(self):
        return self._update_count

    @update_count.setter
    def update_count(self, value):
        value = int(value)
        if value < 0:                                                # onlinelda.h:71-72
            raise RuntimeError("The update count should not be negative.")
        self._update_count = value

    def update_parameters(self, docs, max_iter_tr=10, max_iter_inference=20, kappa=.7,
                          tau=100., rho=-1., adaptive=False, init_gamma=True,
                          update_lambda=True, update_alpha=False, update_eta=False,
                          min_alpha=1e-6, min_eta=1e-6, verbosity=0, inference_method='VI',
                          num_samples=1, burn_in=2):
        """One online update; returns the learning rate used
        (onlineldainterface.cpp:204-256 -> onlinelda.cpp:53-179).

        The lambda path (E-steps, trust-region loop, M-steps) runs on the GPU, and so do the
        sums over gamma, lambda and the statistics that the empirical-Bayes steps for alpha and
        eta and the adaptive learning rate need (onlinelda.cpp:116-175, csrc/eb_kernels.h); the
        host keeps the K- and scalar-sized Newton steps.

        ``inference_method='GIBBS'`` makes every E-step of the loop collapsed Gibbs sampling
        (``burn_in`` sweeps, then ``num_samples`` counted ones; lda.cpp:224-293) -- the hybrid
        stochastic inference of Mimno, Hoffman & Blei (2012), K <= 1024.  ``max_iter_inference``
        does not apply to it; ``update_alpha`` is not supported with it (NotImplementedError)."""
        method = _inference_method(inference_method)
        if method == "CVB0":
            raise NotImplementedError(_CVB0_NO_TRAINING)
        if method == "GIBBS":
            num_samples, burn_in = _gibbs_args(update_alpha, num_samples, burn_in)
        else:
            _ffi.check_vi_topics(self._K)
        batch, owned = self._batch(docs)
        try:
            # (the previous call's empirical-Bayes step, if it is still on its way: the conversion
            # and upload above ran beside the device's work on that call)
            self._settle()
            B = len(batch)
            if B == 0:
                return 1.0                                           # onlinelda.cpp:54-56
            L = _ffi.lib()
            rho_arg = float(rho)
            if rho_arg < 0. and adaptive:
                rho_arg = self._ada_rho                              # onlinelda.cpp:61-62
            eta_old = self._eta
            # the adaptive rate reads lambda' and the statistics after the update
            # (onlinelda.cpp:167-175): the device keeps both
            _ffi.check(L.trlda_model_set_keep_sstats(self._handle,
                                                     int(bool(adaptive and update_lambda))))
            count = C.c_int(self._update_count)
            rho_out = C.c_double(0.)
            if method == "GIBBS":
                _ffi.check(L.trlda_model_online_update_gibbs(
                    self._handle, batch.handle, self._num_documents, self._eta, int(max_iter_tr),
                    float(kappa), float(tau), rho_arg, int(bool(init_gamma)),
                    int(bool(update_lambda)), num_samples, burn_in, C.byref(count),
                    C.byref(rho_out), None))
            else:
                _ffi.check(L.trlda_model_online_update(
                    self._handle, batch.handle, self._num_documents, self._eta, int(max_iter_tr),
                    int(max_iter_inference), float(kappa), float(tau), rho_arg,
                    int(bool(init_gamma)), int(bool(update_lambda)), 0.001,  # lda.h:56: fixed
                    C.byref(count), C.byref(rho_out), None))
            rho_used = rho_out.value

            if update_alpha or update_eta:                           # onlinelda.cpp:116-162
                if update_alpha and not update_lambda:
                    self._resident_estep(batch, max_iter_inference)
                # the device sums over gamma and lambda and their way back to the host are
                # enqueued; the wait, the K-sized Newton steps on the host and the new alpha's way
                # to the device are left to whoever next needs alpha, eta or an E-step (_settle):
                # a loop over mini-batches prepares its next one meanwhile
                _ffi.check(L.trlda_model_online_eb_begin(
                    self._handle, None, B, B, int(bool(update_alpha)), int(bool(update_eta))))
                self._eb_pending = (rho_used, float(min_alpha), float(min_eta))
                if update_lambda and adaptive:
                    self._settle()

            if update_lambda and adaptive:                           # onlinelda.cpp:167-175
                t = self._ada_tau
                u2, g2 = C.c_double(0.), C.c_double(0.)
                _ffi.check(L.trlda_model_adaptive_stats(
                    self._handle, eta_old, float(self._num_documents) / B, t,
                    C.byref(u2), C.byref(g2)))
                self._ada_sq_norm = (1. - 1. / t) * self._ada_sq_norm + 1. / t * u2.value
                self._ada_rho = g2.value / self._ada_sq_norm
                self._ada_tau = t * (1. - self._ada_rho) + 1.

            self._update_count = count.value
        finally:
            if owned:
                batch.close()
        return rho_used

    def __reduce__(self):                                            # onlineldainterface.cpp:265
        self._settle()
        args = (self._V, self._K, self._num_documents, self.alpha, self._eta)
        state = (self.lambdas, self._update_count)
        return (self.__class__, args, state)

    def __setstate__(self, state):                                   # onlineldainterface.cpp:296
        lam, count = state
        self.lambdas = lam
        self.update_count = count


def _gibbs_args(update_alpha, num_samples, burn_in):
    """The checks of an update with inference_method='GIBBS' that come before anything is drawn or
    launched: the reference would put the sampled theta where gamma belongs (onlinelda.cpp:116-141),
    as lower_bound(..., 'gibbs') would."""
    if update_alpha:
        raise NotImplementedError("`update_alpha` is not supported with Gibbs sampling.")
    num_samples, burn_in = int(num_samples), int(burn_in)
    if num_samples < 0 or burn_in < 0:
        raise RuntimeError("`num_samples` and `burn_in` should not be negative.")
    return num_samples, burn_in


def _online_alpha_step(alpha, psi_gamma_diff, num_docs, rho, min_alpha):
    """One natural-gradient step on alpha, onlinelda.cpp:123-142; psi_gamma_diff[k] = sum over the
    mini-batch's documents of psi(gamma_dk) - psi(sum_k gamma_dk).  K-sized host arithmetic in
    the library (csrc/eb_steps.cpp)."""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    out = np.empty_like(alpha)
    _ffi.check(_ffi.lib().trlda_eb_online_alpha_step(
        alpha.size, alpha, np.ascontiguousarray(psi_gamma_diff, dtype=np.float64), float(num_docs),
        float(rho), float(min_alpha), out))
    return out


def _online_eta_step(eta, sum_psi_lambda, rowsums, K, V, rho, min_eta):
    """One Newton step on eta, onlinelda.cpp:147-162 (csrc/eb_steps.cpp)."""
    return float(_ffi.lib().trlda_eb_online_eta_step(
        float(eta), float(sum_psi_lambda), np.ascontiguousarray(rowsums, dtype=np.float64), int(K),
        int(V), float(rho), float(min_eta)))


class _Verbosity(object):
    """`verbosity > 1`: the line searches print their progress to stdout in the reference's words
    (batchlda.cpp:78-88,120-123,155-165,184-187; cumulativelda.cpp:87-97,129-132) -- from C, so
    Python's own buffer is flushed first to keep the order of what a caller prints around it."""

    def __init__(self, verbosity):
        self.verbosity = int(verbosity)

    def __enter__(self):
        if self.verbosity > 1:
            import sys
            sys.stdout.flush()
        _ffi.lib().trlda_eb_set_verbosity(self.verbosity)

    def __exit__(self, *exc):
        _ffi.lib().trlda_eb_set_verbosity(0)


def _eta_line_search(eta, sum_psi_lambda, rowsums, K, V, max_iter_eta, min_eta, threshold, verbosity=0):
    """Newton steps on eta with a step-halving line search on the lower bound,
    batchlda.cpp:147-205 (csrc/eb_steps.cpp)."""
    with _Verbosity(verbosity):
        return float(_ffi.lib().trlda_eb_eta_line_search(
            float(eta), float(sum_psi_lambda), np.ascontiguousarray(rowsums, dtype=np.float64), int(K),
            int(V), int(max_iter_eta), float(min_eta), float(threshold)))


def _alpha_line_search(alpha, psi_gamma_diff, num_docs, max_iter_alpha, min_alpha, threshold, verbosity=0):
    """Newton / natural-gradient steps on alpha with a step-halving line search on the lower
    bound: batchlda.cpp:81-141 == cumulativelda.cpp:90-150 (csrc/eb_steps.cpp)."""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    out = np.empty_like(alpha)
    with _Verbosity(verbosity):
        _ffi.check(_ffi.lib().trlda_eb_alpha_line_search(
            alpha.size, alpha, np.ascontiguousarray(psi_gamma_diff, dtype=np.float64), float(num_docs),
            int(max_iter_alpha), float(min_alpha), float(threshold), out))
    return out


class BatchLDA(LDA):
    """Batch variational LDA (reference src/batchlda.cpp, batchldainterface.cpp)."""

    def __init__(self, num_words, num_topics, alpha=.1, eta=.3, device=None):
        self._setup(num_words, num_topics, alpha, eta, device)

    def update_parameters(self, docs, max_epochs=100, max_iter_inference=100, max_iter_alpha=10,
                          max_iter_eta=20, update_lambda=True, update_alpha=False,
                          update_eta=False, min_alpha=1e-6, min_eta=1e-6,
                          emp_bayes_threshold=1e-8, verbosity=0, inference_method='VI',
                          num_samples=1, burn_in=2):
        """batchldainterface.cpp:126-172 -> batchlda.cpp:43-208.  The E-steps and
        lambda = eta + sstats run on the GPU, as do the sums over gamma and lambda behind the
        alpha / eta line searches (batchlda.cpp:66-205); the searches themselves are K- and
        scalar-sized and run on the host.

        ``inference_method='GIBBS'``: every epoch's E-step is collapsed Gibbs sampling from a
        fresh theta (see OnlineLDA.update_parameters); ``update_alpha`` is not supported with it."""
        method = _inference_method(inference_method)
        if method == "CVB0":
            raise NotImplementedError(_CVB0_NO_TRAINING)
        if method == "GIBBS":
            num_samples, burn_in = _gibbs_args(update_alpha, num_samples, burn_in)
        else:
            _ffi.check_vi_topics(self._K)
        batch, owned = self._batch(docs)
        try:
            B = len(batch)
            if B == 0:
                return 1.                                            # batchlda.cpp:44-46
            L = _ffi.lib()
            K, V = self._K, self._V
            if method == "GIBBS":
                def lambda_step(epochs, upd):
                    _ffi.check(L.trlda_model_batch_update_gibbs(
                        self._handle, batch.handle, self._eta, epochs, upd, num_samples, burn_in,
                        None))
            else:
                def lambda_step(epochs, upd):
                    _ffi.check(L.trlda_model_batch_update(
                        self._handle, batch.handle, self._eta, epochs, int(max_iter_inference), upd,
                        0.001, None))
            if not (update_alpha or update_eta):
                lambda_step(int(max_epochs), int(bool(update_lambda)))
                return 1.
            for _epoch in range(int(max_epochs)):                    # batchlda.cpp:48
                if update_lambda:
                    lambda_step(1, 1)
                if update_alpha:                                     # batchlda.cpp:64-142
                    if not update_lambda:
                        self._resident_estep(batch, max_iter_inference)
                    alpha = _alpha_line_search(self._alpha, self._psi_gamma_diff_device(B), B,
                                               max_iter_alpha, min_alpha, emp_bayes_threshold, verbosity)
                    _ffi.check(L.trlda_model_set_alpha(self._handle, np.ascontiguousarray(alpha)))
                    self._alpha = alpha
                if update_eta:                                       # batchlda.cpp:147-205
                    sum_psi, rowsums = self._lambda_psi_stats_device()
                    self._eta = _eta_line_search(self._eta, sum_psi, rowsums, K, V, max_iter_eta,
                                                 min_eta, emp_bayes_threshold, verbosity)
        finally:
            if owned:
                batch.close()
        return 1.                                                    # batchlda.cpp:207

    def __reduce__(self):                                            # batchldainterface.cpp:181
        return (self.__class__, (self._V, self._K, self.alpha, self._eta), (self.lambdas,))

    def __setstate__(self, state):
        self.lambdas = state[0]


class CumulativeLDA(LDA):
    """SDA-Bayes streaming LDA (reference src/cumulativelda.cpp, cumulativeldainterface.cpp).

        >>> model = CumulativeLDA(num_words=7000, num_topics=100, alpha=.1, eta=.3)
        >>> for documents in load_documents('data_train.dat', 1000):
        ...     model.update_parameters(documents, max_epochs=100)

    In contrast to OnlineLDA, each document should be processed only once.
    """

    def __init__(self, num_words, num_topics, alpha=.1, eta=.3, device=None):
        # the base constructor draws a random lambda from the libc stream (lda.cpp:71) before
        # CumulativeLDA overwrites it with eta (cumulativelda.cpp:30): keep the stream in step
        self._setup(num_words, num_topics, alpha, eta, device)
        self.lambdas = np.full((self._K, self._V), float(eta))
        self._psi_gamma_diff = np.zeros(self._K)
        self._num_documents = 0

    def update_parameters(self, docs, max_epochs=100, max_iter_inference=100, max_iter_alpha=10,
                          update_lambda=True, update_alpha=False, min_alpha=1e-6,
                          emp_bayes_threshold=1e-8, inference_threshold=0.001, verbosity=0):
        """cumulativeldainterface.cpp:115-160 -> cumulativelda.cpp:49-153."""
        _ffi.check_vi_topics(self._K)
        batch, owned = self._batch(docs)
        try:
            B = len(batch)
            if B == 0:
                return 1.                                            # cumulativelda.cpp:50-52
            L = _ffi.lib()
            _ffi.check(L.trlda_model_cumulative_update(
                self._handle, batch.handle, int(max_epochs), int(max_iter_inference),
                int(bool(update_lambda)), float(inference_threshold), None))
            if update_alpha:                                         # cumulativelda.cpp:76-150
                self._resident_estep(batch, max_iter_inference, inference_threshold)
                self._psi_gamma_diff = self._psi_gamma_diff + self._psi_gamma_diff_device(B)
                self._num_documents += B
                alpha = _alpha_line_search(self._alpha, self._psi_gamma_diff, self._num_documents,
                                           max_iter_alpha, min_alpha, emp_bayes_threshold, verbosity)
                _ffi.check(L.trlda_model_set_alpha(self._handle, np.ascontiguousarray(alpha)))
                self._alpha = alpha
        finally:
            if owned:
                batch.close()
        return 1.

    def __reduce__(self):                                            # cumulativeldainterface.cpp
        return (self.__class__, (self._V, self._K, self.alpha, self._eta), (self.lambdas,))

    def __setstate__(self, state):
        self.lambdas = state[0]
