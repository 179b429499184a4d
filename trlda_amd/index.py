"""Nearest documents in topic space: ``DocumentIndex`` (csrc/docindex_kernels.h).

A device-resident table of the documents' topic proportions theta = gamma / sum(gamma) and the
ranked search over it; the topic summaries of the indexed corpus -- per topic its most representative
documents, and the covariance and correlations of theta (csrc/topicdocs_kernels.h);
the indexed documents that best explain a query's words (csrc/querylik_kernels.h); and
the document groups of the indexed corpus (csrc/cluster_kernels.h), their
silhouettes (csrc/silhouette_kernels.h), and the radius join -- the documents within
a distance of each document -- with the density-based groups built on it (csrc/neighbors_kernels.h,
DESIGN.md 3.29), and the minimum spanning tree of the indexed corpus with the single-linkage hierarchy
and HDBSCAN* on it (csrc/mst_kernels.h); and topic prevalence against what the caller
knows about the documents -- group means, topics over time, the regression on covariates
(csrc/effects_kernels.h); and the reverse direction, a document's class predicted from
its topic proportions -- multinomial logistic regression and a nearest-neighbour baseline
(csrc/classify_kernels.h).
No counterpart in the reference package.
"""
import ctypes as C
import math
import operator

import numpy as np

from . import _ffi

MEASURES = {"hellinger": 0, "cosine": 1}
MAX_TOP_N = 100
MAX_CLUSTERS = 4096                          # TRLDA_CLUSTER_MAX_CLUSTERS
MAX_NEIGHBORS = 99                           # kTsneMaxNeighbors
MAX_PERPLEXITY = 33                          # 3 * perplexity <= MAX_NEIGHBORS
MAX_DESIGN_COLUMNS = 256                     # TRLDA_EFFECTS_MAX_COLUMNS
MAX_CLASSES = 128                            # TRLDA_CLASSIFY_MAX_CLASSES
LBFGS_MEMORY = 10                            # pairs the classifier's optimiser keeps: a chosen number


def _measure(name):
    if not isinstance(name, str):
        raise TypeError("`measure` should be of type `str`.")
    try:
        return MEASURES[name.lower()]
    except KeyError:
        raise ValueError("Unknown measure '%s' (expected 'hellinger' or 'cosine')." % name)


class DocumentIndex(object):
    """The documents of a model ranked by how close their topic proportions are.

    ``measure='hellinger'`` (default) stores ``sqrt(theta)`` and ranks by the Bhattacharyya
    coefficient ``s = sum_k sqrt(theta_qk theta_dk)``; the distance is ``sqrt(max(0, 1 - s))``.
    ``measure='cosine'`` stores ``theta / |theta|`` and ranks by the cosine ``s``; the distance is
    ``max(0, 1 - s)``.  theta is the posterior mean ``gamma / sum(gamma)``.  Ids are the documents'
    positions in order of addition, from 0.  Equal similarities rank by smaller id, so the result
    does not depend on how the index was filled or how the search is cut up.

    The index stores theta, not lambda: after the model's lambda changes, the rows added before
    are stale.  This is not detected.  It lives on the model's device and is closed with it.
    """

    def __init__(self, model, measure="hellinger"):
        self._handle = None
        self._measure = _measure(measure)                    # (before any GPU work)
        _ffi.require_gpu()
        if getattr(model, "_handle", None) is None:
            raise RuntimeError("The model has been closed.")
        self._model = model
        self._K = model.num_topics
        handle = _ffi.vp()
        _ffi.check(_ffi.lib().trlda_docindex_create(model._handle, self._measure, C.byref(handle)))
        self._handle = handle
        model._register_index(self)

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_handle", None):
            _ffi.lib().trlda_docindex_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self._handle:
            raise RuntimeError("The index has been closed.")
        return self._handle

    @property
    def measure(self):
        return "cosine" if self._measure else "hellinger"

    def __len__(self):
        return int(_ffi.lib().trlda_docindex_size(self._live()))

    def reserve(self, n):
        """Room for ``n`` documents in all, so that adding them copies nothing."""
        _ffi.check(_ffi.lib().trlda_docindex_reserve(self._live(), operator.index(n)))

    def set_slab_rows(self, rows):
        """A/B switch: index rows per workgroup of the search (0: default).  Results do not depend on it."""
        _ffi.check(_ffi.lib().trlda_docindex_set_slab_rows(self._live(), operator.index(rows)))

    def rows(self, first=0, count=None):
        """The stored rows ``first .. first + count - 1`` (count x K float64)."""
        first = operator.index(first)
        count = len(self) - first if count is None else operator.index(count)
        out = np.empty((max(count, 0), self._K), dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_docindex_read_rows(self._live(), first, count, out.ctypes.data))
        return out

    # -- arguments --------------------------------------------------------------------------------
    def _gamma(self, gamma):
        try:
            g = np.array(gamma, dtype=np.float64, order="F", copy=True)
        except (TypeError, ValueError):
            raise TypeError("`gamma` should be of type `ndarray`.")
        if g.ndim == 1:
            g = g.reshape(-1, 1, order="F")
        if g.ndim != 2 or g.shape[0] != self._K:
            raise RuntimeError("Gamma has wrong dimensionality.")
        return np.asfortranarray(g)

    def _latents(self, latents, B):
        """gamma0 (K x B): ``latents``, else drawn from the seeded stream as ``update_variables`` draws it."""
        if latents is not None:
            try:
                g = np.array(latents, dtype=np.float64, order="F", copy=True)
            except (TypeError, ValueError):
                raise TypeError("`latents` should be of type `ndarray`.")
            if g.ndim == 1:
                g = g.reshape(-1, 1, order="F")
            if g.ndim != 2 or g.shape != (self._K, B):
                raise RuntimeError("Initial gamma has wrong dimensionality.")  # lda.cpp:165
            return np.asfortranarray(g)
        gamma = np.empty((self._K, B), dtype=np.float64, order="F")
        _ffi.lib().trlda_sample_gamma_init(self._K, B, gamma)                 # lda.cpp:135
        return gamma

    def _top_n(self, top_n):
        top_n = operator.index(top_n)
        if not 1 <= top_n <= min(len(self), MAX_TOP_N):
            raise RuntimeError("`top_n` should lie between 1 and min(len(index), %d)." % MAX_TOP_N)
        return top_n

    def _scored(self, ids, gamma, N):
        """(ids as int64 or None, gamma as K x M or None, M) of the documents a call scores: all N, the
        ids, or a gamma's columns."""
        rows = _silhouette_ids(ids, N)
        g = None if gamma is None else self._gamma(gamma)
        if g is not None and g.shape[1] < 1:
            raise RuntimeError("`gamma` should hold at least one document.")
        return rows, g, N if rows is None and g is None else (rows.shape[0] if g is None else g.shape[1])

    def _result(self, ids, sim, return_similarity):
        if return_similarity:
            return ids, sim
        rest = np.maximum(0.0, 1.0 - sim)
        return ids, (rest if self._measure else np.sqrt(rest))

    # -- adding -----------------------------------------------------------------------------------
    def add(self, docs, latents=None, max_iter=100, threshold=0.001, return_gamma=False):
        """VI on ``docs`` (a list, ``DocumentList`` or ``DeviceBatch``) with lambda fixed, from
        ``latents`` as gamma0 or a gamma drawn as ``update_variables`` draws it; the documents are
        appended.  Returns the first new id (with ``return_gamma=True`` also gamma, K x B)."""
        handle = self._live()
        model = self._model
        _ffi.check_vi_topics(self._K)                                # (before the draw and the upload)
        batch, owned = model._batch(docs)
        try:
            model._settle()
            B = len(batch)
            gamma = self._latents(latents, B)
            first = len(self)
            _ffi.check(_ffi.lib().trlda_docindex_add(handle, batch.handle, gamma.ctypes.data, int(max_iter),
                                                     float(threshold)))
        finally:
            if owned:
                batch.close()
        return (first, gamma) if return_gamma else first

    def add_gamma(self, gamma):
        """Appends the documents with variational parameters ``gamma`` (K x B, finite and
        positive); no E-step.  Returns the first new id."""
        handle = self._live()
        g = self._gamma(gamma)
        first = len(self)
        _ffi.check(_ffi.lib().trlda_docindex_add_gamma(handle, g.ctypes.data, g.shape[1]))
        return first

    def add_gamma_device(self, gamma_ptr, num_documents):
        """The same from a device pointer to K x B float64 (not validated; enqueued on the
        model's stream).  Returns the first new id."""
        handle = self._live()
        first = len(self)
        _ffi.check(_ffi.lib().trlda_docindex_add_gamma_dev(handle, gamma_ptr, operator.index(num_documents)))
        return first

    # -- searching --------------------------------------------------------------------------------
    def query(self, docs, top_n=10, latents=None, max_iter=100, threshold=0.001, return_gamma=False,
              return_similarity=False):
        """The ``top_n`` nearest indexed documents of each document of ``docs``, after VI on them
        as in ``add``.  Returns ``(ids, dist)``, int64 and float64 of shape (B, top_n), closest
        first; with ``return_similarity=True`` the similarity s in place of the distance; with
        ``return_gamma=True`` gamma (K x B) is appended.  ``1 <= top_n <= min(len(index), 100)``,
        else RuntimeError."""
        handle = self._live()
        model = self._model
        top_n = self._top_n(top_n)
        _ffi.check_vi_topics(self._K)                                # (before the draw and the upload)
        batch, owned = model._batch(docs)
        try:
            model._settle()
            B = len(batch)
            gamma = self._latents(latents, B)
            ids = np.empty((B, top_n), dtype=np.int64)
            sim = np.empty((B, top_n), dtype=np.float64)
            _ffi.check(_ffi.lib().trlda_docindex_query(handle, batch.handle, gamma.ctypes.data, int(max_iter),
                                                       float(threshold), top_n, ids.ctypes.data,
                                                       sim.ctypes.data))
        finally:
            if owned:
                batch.close()
        out = self._result(ids, sim, return_similarity)
        return out + (gamma,) if return_gamma else out

    def query_gamma(self, gamma, top_n=10, return_similarity=False):
        """The same search for documents given by their ``gamma`` (K x B); no E-step."""
        handle = self._live()
        top_n = self._top_n(top_n)
        g = self._gamma(gamma)
        B = g.shape[1]
        ids = np.empty((B, top_n), dtype=np.int64)
        sim = np.empty((B, top_n), dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_docindex_query_gamma(handle, g.ctypes.data, B, top_n, ids.ctypes.data,
                                                         sim.ctypes.data))
        return self._result(ids, sim, return_similarity)

    def query_likelihood(self, queries, top_n=10, per_word=False):
        """The ``top_n`` indexed documents that best explain each query's words (the query-likelihood
        document model; Wei & Croft 2006): ``score(q, d) = sum_i c_i log sum_k theta_dk beta_k,w_i``
        over the query's ``(id, count)`` pairs, in nats, with ``beta_kw = lambda_kw / sum_v lambda_kv``
        and theta recovered from the stored rows as in ``topic_documents``.  ``queries`` is a list of
        ``[(id, count), ...]``, a ``DocumentList`` or a ``DeviceBatch``.  Nothing is inferred for a
        query, so there is no gamma0, nothing is drawn from the seeded stream and any number of
        topics will do.

        Returns ``(ids, loglik)``, int64 and float64 of shape (B, top_n), in the total order (score
        descending, id ascending); ``per_word=True`` divides each returned score by the query's
        ``sum_i c_i`` (the ranking is the same; a query without words keeps 0.0).  A query without
        words scores 0.0 everywhere, so its ids are ``0 .. top_n - 1``; a document that gives a
        word no probability scores ``-inf`` and ranks last, by id.  ``1 <= top_n <= min(len(index),
        100)``, else RuntimeError.

        The call uses the model's lambda as it is now and the stored theta: the index stores theta,
        not lambda, so after the model's lambda changes, the rows added before are stale.  This is
        not detected."""
        handle = self._live()
        model = self._model
        top_n = self._top_n(top_n)
        batch, owned = model._batch(queries)
        try:
            model._settle()
            B = len(batch)
            ids = np.empty((B, top_n), dtype=np.int64)
            loglik = np.empty((B, top_n), dtype=np.float64)
            _ffi.check(_ffi.lib().trlda_docindex_query_likelihood(handle, batch.handle, top_n, ids.ctypes.data,
                                                                  loglik.ctypes.data))
            if per_word:
                csr = batch.csr
                # (counts <= 0 add nothing on the device either)
                run = np.concatenate(([0], np.cumsum(np.maximum(np.asarray(csr.cnts, dtype=np.int64), 0))))
                indptr = np.asarray(csr.indptr, dtype=np.int64)
                total = (run[indptr[1:]] - run[indptr[:-1]]).astype(np.float64)
                words = total > 0
                loglik[words] /= total[words, None]
        finally:
            if owned:
                batch.close()
        return ids, loglik

    # -- topic summaries (csrc/topicdocs_kernels.h) ---------------------------------
    def set_moment_chunk(self, rows):
        """A/B switch: index rows per chunk of the scatter's sum over the documents (0: default).
        Results with a forced chunk agree within rounding, not bitwise."""
        rows = operator.index(rows)
        _ffi.check(_ffi.lib().trlda_docindex_set_moment_chunk(self._live(), rows))

    def topic_documents(self, top_n=10, return_theta=False):
        """Per topic the ``top_n`` indexed documents that hold most of it: ``ids``, int64 of shape
        (K, top_n), in the total order (theta descending, id ascending); with ``return_theta=True``
        also their theta (float64, K x top_n).  theta is recovered from the stored rows: ``r * r``
        (hellinger) or ``r / sum(r)`` (cosine).  ``1 <= top_n <= min(len(index), 100)``, else
        RuntimeError."""
        top_n = self._top_n(top_n)
        handle = self._live()
        ids = np.empty((self._K, top_n), dtype=np.int64)
        theta = np.empty((self._K, top_n), dtype=np.float64) if return_theta else None
        _ffi.check(_ffi.lib().trlda_docindex_topic_documents(handle, top_n, ids.ctypes.data,
                                                             theta.ctypes.data if return_theta else None))
        return (ids, theta) if return_theta else ids

    def _moments(self):
        """(mean K, scatter K x K) of theta over the indexed documents, from the device."""
        handle = self._live()
        mean = np.empty(self._K, dtype=np.float64)
        scatter = np.empty((self._K, self._K), dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_docindex_topic_moments(handle, mean.ctypes.data, scatter.ctypes.data))
        return mean, scatter

    def topic_covariance(self, ddof=1, return_mean=False):
        """The K x K covariance of theta over the indexed documents, ``S / (N - ddof)`` with the
        centred scatter ``S = sum_d (theta_d - m)(theta_d - m)^T`` (with ``return_mean=True`` also
        the mean m, K).  ``N - ddof <= 0`` is a ValueError."""
        rest = len(self) - ddof
        if not rest > 0:
            raise ValueError("`ddof` leaves no degrees of freedom (%d documents)." % len(self))
        mean, scatter = self._moments()
        cov = scatter / float(rest)
        return (cov, mean) if return_mean else cov

    def topic_correlations(self):
        """The K x K correlations of theta over the indexed documents, ``S_ij / (sqrt(S_ii)
        sqrt(S_jj))`` clamped to [-1, 1]: an exact 1 on the diagonal, and NaN wherever one of the
        two variances is 0 (the diagonal included), as ``np.corrcoef`` gives."""
        return _correlation(self._moments()[1])

    # -- document groups (csrc/cluster_kernels.h) -----------------------------------
    def _num_clusters(self, num_clusters):
        num_clusters = operator.index(num_clusters)
        if not 1 <= num_clusters <= min(len(self), MAX_CLUSTERS):
            raise RuntimeError("`num_clusters` should lie between 1 and min(len(index), %d)." % MAX_CLUSTERS)
        return num_clusters

    def _theta(self, doc_id):
        """theta^ of one indexed document from its stored row: ``r * r`` or ``r / sum(r)``."""
        r = self.rows(doc_id, 1)[0]
        return r / r.sum() if self._measure else r * r

    def _init_centroids(self, num_clusters, init):
        """The initial centroids, K x C: drawn ids, given ids, or a given array."""
        N = len(self)
        if init is None:
            from .utils import random_select
            ids = random_select(num_clusters, N)
        else:
            a = np.asarray(init)
            if not (a.ndim == 1 and a.dtype.kind in "iu" and a.shape[0] == num_clusters):
                g = self._gamma(init)
                if g.shape[1] != num_clusters:
                    raise RuntimeError("`init` should hold `num_clusters` ids or columns.")
                return g
            ids = [int(i) for i in a]
            if len(set(ids)) != len(ids) or min(ids) < 0 or max(ids) >= N:
                raise ValueError("`init` should hold distinct ids of indexed documents.")
        return np.asfortranarray(np.stack([self._theta(i) for i in ids], axis=1))

    def cluster(self, num_clusters, init=None, max_iter=50, return_info=False):
        """The indexed documents in ``num_clusters`` groups by spherical k-means on the stored rows,
        which is Lloyd's algorithm for the index's own measure: a document goes to the centroid of
        largest similarity s (the smaller cluster on a tie), a centroid becomes the normalised sum of
        its members' rows, until no label changes or ``max_iter`` updates have run.  Returns
        ``(labels, centroids)``: int32 (N,) and the centroids' topic proportions, float64 K x C in
        Fortran order, ready for ``query_gamma`` (the documents nearest each centroid) or another
        index's ``add_gamma``; the labels are the assignment under the returned centroids.  With
        ``return_info=True`` also a dict: ``iterations`` (the updates that ran), ``converged``,
        ``sizes`` (int64, C), ``similarity`` (float64, N: each document's s to its centroid) and
        ``objective``, ``math.fsum(1 - similarity)``: the sum of squared Hellinger distances, or of
        cosine distances.

        ``init``: ``None`` draws ``num_clusters`` distinct ids with ``trlda_amd.utils.random_select``
        from the seeded stream (the only draw, on the host); a sequence of ``num_clusters`` distinct
        document ids (integers) starts from their theta; a K x C array is taken as it is (finite and
        positive).  Duplicate initial centroids leave the later one empty at the first assignment;
        an empty cluster keeps its centroid and reports size 0.  ``max_iter=0`` is a pure assignment.
        ``1 <= num_clusters <= min(len(index), 4096)``, else RuntimeError.  Nothing of size N leaves
        the device but the labels and similarities; two calls agree bitwise."""
        handle = self._live()
        num_clusters = self._num_clusters(num_clusters)
        max_iter = operator.index(max_iter)
        if max_iter < 0:
            raise ValueError("`max_iter` should not be negative.")
        centroids = self._init_centroids(num_clusters, init)
        N = len(self)
        labels = np.empty(N, dtype=np.int32)
        sim = np.empty(N, dtype=np.float64)
        sizes = np.empty(num_clusters, dtype=np.int64)
        iterations, converged = C.c_int(0), C.c_int(0)
        _ffi.check(_ffi.lib().trlda_docindex_cluster(handle, num_clusters, centroids.ctypes.data, max_iter,
                                                     labels.ctypes.data, sim.ctypes.data, sizes.ctypes.data,
                                                     C.byref(iterations), C.byref(converged)))
        if not return_info:
            return labels, centroids
        info = {"iterations": iterations.value, "converged": bool(converged.value), "sizes": sizes,
                "similarity": sim, "objective": math.fsum(1.0 - sim)}
        return labels, centroids, info

    def nearest_centroid(self, centroids, gamma=None, return_similarity=False):
        """The label of each indexed document under ``centroids`` (K x C topic proportions, as
        ``cluster`` returns them) -- or, with ``gamma`` (K x B), of each of those documents; no
        E-step.  int32; with ``return_similarity=True`` also the similarity s to that centroid."""
        handle = self._live()
        c = self._gamma(centroids)
        num_clusters = self._num_clusters(c.shape[1])
        g = None if gamma is None else self._gamma(gamma)
        n = len(self) if g is None else g.shape[1]
        labels = np.empty(n, dtype=np.int32)
        sim = np.empty(n, dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_docindex_assign(handle, c.ctypes.data, num_clusters,
                                                    None if g is None else g.ctypes.data, 0 if g is None else n,
                                                    labels.ctypes.data, sim.ctypes.data))
        return (labels, sim) if return_similarity else labels

    # -- silhouettes (csrc/silhouette_kernels.h) -----------------------------------
    def silhouette(self, labels, ids=None, return_parts=False):
        """The exact silhouette (Rousseeuw 1987) of the indexed documents under ``labels`` -- those of
        ``cluster`` or any grouping the caller brings -- in the index's own distance ``d``,
        ``sqrt(max(0, 1 - s))`` (hellinger) or ``max(0, 1 - s)`` (cosine).  For document i of cluster
        ``own``: ``a`` is its mean distance to the other members of ``own``, ``b`` the smallest mean
        distance to the members of another non-empty cluster, ``neighbour`` that cluster (the smaller
        label on a tie), and the silhouette ``(b - a) / max(a, b)``: 0.0 for the only member of a
        cluster (with ``a = 0.0``) and where ``max(a, b) = 0``.  A document is left out of its own
        mean by id, so two documents with equal rows are a pair at distance 0.

        ``labels``: an integer array of length ``len(index)`` with values in ``[0, C)``,
        ``C = max(labels) + 1 <= 4096``; values without members are ignored.  Fewer than two clusters
        with members is a ValueError; a wrong length, a negative label or C > 4096 a RuntimeError; a
        non-integer array a TypeError.  ``ids=None`` scores every document; otherwise ``ids`` is an
        integer array of row ids (any order, repeats allowed; out of range: RuntimeError), each scored
        against ALL indexed documents: an exact subsample -- ``utils.random_select`` draws one -- at
        cost ``len(ids) * N * K``.

        Returns the silhouettes, float64, one per scored document; with ``return_parts=True``
        ``(s, a, b, neighbour)``, float64 and int32.  The corpus figure is ``math.fsum(s) / len(s)``
        on the host.  A cluster's sum of distances depends on the document, the cluster's members and
        K alone, so two calls agree bitwise, whatever the other clusters, their numbering, the slab
        setting, the rows scored beside it or the way the index was filled.  Nothing is drawn."""
        handle = self._live()
        N = len(self)
        lab, num_clusters = _silhouette_labels(labels, N)
        rows = _silhouette_ids(ids, N)
        n = N if rows is None else rows.shape[0]
        s = np.empty(n, dtype=np.float64)
        if return_parts:
            a, b = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
            neighbour = np.empty(n, dtype=np.int32)
        _ffi.check(_ffi.lib().trlda_docindex_silhouette(handle, lab.ctypes.data, num_clusters,
                                                        None if rows is None else rows.ctypes.data,
                                                        0 if rows is None else n, s.ctypes.data,
                                                        a.ctypes.data if return_parts else None,
                                                        b.ctypes.data if return_parts else None,
                                                        neighbour.ctypes.data if return_parts else None))
        return (s, a, b, neighbour) if return_parts else s

    def select_num_clusters(self, candidates, max_iter=50, ids=None):
        """The number of clusters among ``candidates`` of largest mean silhouette: for each C, in the
        order given, ``cluster(C, max_iter=max_iter)`` (``init=None``: one ``random_select`` per
        candidate from the seeded stream) and ``silhouette(labels, ids=ids)``.  Returns ``(best_C,
        {C: mean silhouette})``, ``best_C`` the first in the order (mean descending, C ascending); a
        candidate whose clustering leaves fewer than two clusters with members scores ``-inf``."""
        scores = {}
        for num_clusters in candidates:
            num_clusters = operator.index(num_clusters)
            labels, _ = self.cluster(num_clusters, max_iter=max_iter)
            if len(np.unique(labels)) < 2:
                scores[num_clusters] = -math.inf
                continue
            s = self.silhouette(labels, ids=ids)
            scores[num_clusters] = math.fsum(s) / len(s)
        if not scores:
            raise ValueError("`candidates` should hold at least one number of clusters.")
        return min(scores, key=lambda c: (-scores[c], c)), scores

    # -- the radius join (csrc/neighbors_kernels.h) ---------------------------------
    def _neighbors(self, radius, rows, g, want_similarity, capacity, indptr, ids, val):
        M = 0 if rows is None and g is None else (rows.shape[0] if g is None else g.shape[1])
        _ffi.check(_ffi.lib().trlda_docindex_neighbors(self._live(), radius,
                                                       None if rows is None else rows.ctypes.data,
                                                       None if g is None else g.ctypes.data, M,
                                                       1 if want_similarity else 0, capacity, indptr.ctypes.data,
                                                       None if ids is None else ids.ctypes.data,
                                                       None if val is None else val.ctypes.data))

    def neighbors_within(self, radius, ids=None, gamma=None, return_similarity=False, count_only=False,
                         max_pairs=1 << 26):
        """The indexed documents within distance ``radius`` of each scored document, in the index's own
        distance ``d``: ``sqrt(max(0, 1 - s))`` (hellinger) or ``max(0, 1 - s)`` (cosine); a pair is a
        hit iff ``d <= radius``.  ``ids=None, gamma=None`` scores every indexed document; ``ids`` is an
        integer array of row ids (any order, repeats allowed; out of range: RuntimeError); ``gamma``
        (K x M) scores documents given by their variational parameters, as ``query_gamma`` takes them
        (no E-step).  An indexed document is left out of its own list by id, so two documents with
        equal rows find each other; for ``gamma`` nothing is left out, so a stored document's own
        gamma finds that document too.

        Returns ``(indptr, ids, dist)`` in CSR form: ``indptr`` int64 of length M + 1, ``ids`` int64 and
        ``dist`` float64 of length ``indptr[-1]``; the hits of scored document q are
        ``ids[indptr[q]:indptr[q + 1]]``, in ascending id.  With ``return_similarity=True`` the
        similarity s stands in place of the distance; with ``count_only=True`` only ``indptr`` is
        returned and one pass over the pairs is made instead of two.  More than ``max_pairs`` hits in
        all is a RuntimeError that names the total (nothing of that size is allocated first).

        ``s(i, j)`` and ``s(j, i)`` are the same bits, so the hit graph of the whole index is
        symmetric.  The result does not depend on ``set_slab_rows``, on the documents scored beside a
        document or on how the index was filled, and two calls agree bitwise.  Nothing is drawn.

        ``radius=0`` finds a duplicate only where the two rows' own dot rounds to at least 1, which a
        unit-length row in floating point need not give: look for duplicates with a small positive
        radius (1e-6 is far above the rounding of a distance at any K)."""
        self._live()                                         # (a closed index is reported before a bad radius)
        radius = float(radius)
        if not (radius >= 0.0 and math.isfinite(radius)):
            raise ValueError("`radius` should be finite and not negative.")
        if ids is not None and gamma is not None:
            raise ValueError("Give `ids` or `gamma`, not both.")
        max_pairs = operator.index(max_pairs)
        if max_pairs < 1:
            raise ValueError("`max_pairs` should be positive.")
        rows, g, M = self._scored(ids, gamma, self._size())
        indptr = np.empty(M + 1, dtype=np.int64)
        if count_only:
            self._neighbors(radius, rows, g, False, 0, indptr, None, None)
            return indptr
        capacity = min(max_pairs, max(16 * M, 1 << 20))
        while True:
            hit = np.empty(capacity, dtype=np.int64)
            val = np.empty(capacity, dtype=np.float64)
            self._neighbors(radius, rows, g, return_similarity, capacity, indptr, hit, val)
            total = int(indptr[M])
            if total <= capacity:
                return indptr, hit[:total].copy(), val[:total].copy()
            if total > max_pairs:
                raise RuntimeError("%d pairs lie within the radius, more than `max_pairs` (%d)." % (total, max_pairs))
            capacity = total                                         # (the second call: the exact size)

    def dbscan(self, radius, min_samples=5, max_pairs=1 << 26, return_core=False):
        """Density-based groups of the indexed documents (DBSCAN; Ester et al. 1996) under
        ``neighbors_within(radius)``: no number of clusters is named, and outliers are.  A document is
        a *core* iff its hits plus itself number at least ``min_samples``.  The clusters are the
        connected components of the core documents under the hit graph, numbered from 0 by ascending
        smallest core id.  A document that is no core but has a core among its hits (a border
        document) takes the cluster of its nearest core hit, in the order (distance ascending, id
        ascending).  Every other document is noise, labelled -1.

        Returns the labels, int32 of length ``len(index)``; with ``return_core=True`` also the boolean
        array of the core documents.  The cores come from one ``count_only`` pass; the hits are then
        read in chunks of consecutive ids of at most ``max_pairs`` pairs each (a single document with
        more hits than that is a RuntimeError), and the labels are the same bits whatever ``max_pairs``
        is.  The rest is host arithmetic.  ``silhouette`` takes these labels once noise is given a
        label of its own, for instance ``np.where(labels < 0, labels.max() + 1, labels)``."""
        self._live()
        min_samples = operator.index(min_samples)
        if min_samples < 1:
            raise ValueError("`min_samples` should be positive.")
        max_pairs = operator.index(max_pairs)
        if max_pairs < 1:
            raise ValueError("`max_pairs` should be positive.")
        counts = np.diff(self.neighbors_within(radius, count_only=True))
        N = counts.shape[0]
        core = counts + 1 >= min_samples
        parent = np.arange(N, dtype=np.int64)
        nearest = np.full(N, -1, dtype=np.int64)             # a border document's nearest core hit
        before = np.concatenate(([0], np.cumsum(counts)))   # the pairs of the documents before each id
        first = 0
        while first < N:
            # the longest run of consecutive ids from `first` that holds at most max_pairs pairs
            last = int(np.searchsorted(before, before[first] + max_pairs, side="right")) - 1
            last = max(last, first + 1)                      # (one document with more: the call raises)
            if before[last] > before[first]:
                scored = np.arange(first, last, dtype=np.int64)
                indptr, hit, dist = self.neighbors_within(radius, ids=scored, max_pairs=max_pairs)
                rows = np.repeat(scored, np.diff(indptr))
                to_core = core[hit]
                link = to_core & core[rows]
                _union(parent, rows[link], hit[link])
                border = to_core & ~core[rows]
                _nearest(nearest, rows[border], hit[border], dist[border])
            first = last
        return _dbscan_labels(parent, core, nearest, return_core)

    # -- the spanning tree (csrc/mst_kernels.h) --------------------------------------
    def _min_samples(self, min_samples, N):
        min_samples = operator.index(min_samples)
        if not 1 <= min_samples <= min(N, MAX_TOP_N):
            raise RuntimeError("`min_samples` should lie between 1 and min(len(index), %d)." % MAX_TOP_N)
        return min_samples

    def _sweep(self, comp, core):
        """One sweep on the device: per document its lightest edge to another component, ``(best_j,
        best_w)``, int64 (-1: none) and float64."""
        N = comp.shape[0]
        best_j = np.empty(N, dtype=np.int64)
        best_w = np.empty(N, dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_docindex_mst_sweep(self._live(), comp.ctypes.data,
                                                       None if core is None else core.ctypes.data,
                                                       best_j.ctypes.data, best_w.ctypes.data))
        return best_j, best_w

    def spanning_tree(self, min_samples=1, return_core=False):
        """The minimum spanning tree of the complete graph on the indexed documents.  With
        ``min_samples=1`` the weight of the edge (i, j) is the index's own distance ``d(i, j)`` -- the
        tree of single linkage; with ``min_samples >= 2`` it is the mutual-reachability distance of
        HDBSCAN* (Campello, Moulavi & Sander 2013), ``max(d(i, j), core[i], core[j])``, where
        ``core[i]`` is the distance to document i's (min_samples - 1)-th nearest other document
        (``nearest_neighbors(min_samples - 1)``): the document itself counts as the first of its
        neighbourhood, as in ``dbscan`` and scikit-learn.  ``1 <= min_samples <= min(len(index),
        100)``, else RuntimeError.

        Returns ``(u, v, w)``: int64, int64 and float64 of length N - 1 with ``u < v``, the edges sorted
        by ``(w, u, v)`` (one document: three empty arrays); with ``return_core=True`` also the core
        distances, float64 of length N (zeros for ``min_samples=1``).  Edges are compared in that
        same order, a strict total one since ``d(i, j)`` and ``d(j, i)`` are the same bits, so the
        tree is THE minimum spanning tree under it: equal weights, which mutual reachability makes
        in bulk, leave no choice.

        Boruvka's algorithm: every round one sweep on the device finds each document's lightest edge
        to another component (nothing of size N x N exists), the host joins every component along its
        lightest such edge; at most ceil(log2 N) rounds.  The result does not depend on
        ``set_slab_rows`` or on how the index was filled, and two calls agree bitwise.  Nothing is
        drawn."""
        self._live()
        N = self._size()
        min_samples = self._min_samples(min_samples, N)
        core = None
        if min_samples > 1:
            core = np.ascontiguousarray(self.nearest_neighbors(min_samples - 1)[1][:, -1])
        parent = np.arange(N, dtype=np.int64)
        comp = np.arange(N, dtype=np.int32)
        parts, left = [], N
        for _ in range(max(N - 1, 0).bit_length()):         # ceil(log2 N) rounds
            if left == 1:
                break
            lo, hi, w = _boruvka_edges(comp, *self._sweep(comp, core))
            parts.append((lo, hi, w))
            _union(parent, lo, hi)
            comp = _roots(parent).astype(np.int32)           # (a tree's root is its smallest member)
            left = len(np.unique(comp))
        tree = _sorted_edges(parts)
        if left != 1 or len(tree[0]) != N - 1:
            raise RuntimeError("internal error: the spanning tree did not close in ceil(log2 N) rounds.")
        if return_core:
            return tree + (np.zeros(N, dtype=np.float64) if core is None else core,)
        return tree

    def single_linkage(self, min_samples=1):
        """The single-linkage hierarchy of the indexed documents from ``spanning_tree(min_samples)``, as
        the (N - 1) x 4 float64 linkage matrix of SciPy: row t merges the clusters ``Z[t, 0] <
        Z[t, 1]`` at height ``Z[t, 2]``, the tree's t-th edge weight, into cluster N + t of
        ``Z[t, 3]`` documents; the merges are in the tree's edge order.
        ``scipy.cluster.hierarchy.dendrogram`` and ``fcluster`` take it as it is, ``cut_linkage``
        cuts it."""
        N = self._size()
        return _linkage(*self.spanning_tree(min_samples), N)

    @staticmethod
    def cut_linkage(Z, num_clusters=None, distance=None):
        """The flat groups of a linkage matrix ``Z`` (N - 1 rows): with ``num_clusters`` after its first
        N - num_clusters merges, with ``distance`` after every merge of height ``<= distance``;
        exactly one of the two, else ValueError.  Returns int32 labels of length N, numbered from 0
        by ascending smallest member id, as ``dbscan`` numbers its clusters."""
        if (num_clusters is None) == (distance is None):
            raise ValueError("Give exactly one of `num_clusters` and `distance`.")
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[1] != 4:
            raise ValueError("`Z` should be a linkage matrix of four columns.")
        N = Z.shape[0] + 1
        if num_clusters is not None:
            num_clusters = operator.index(num_clusters)
            if not 1 <= num_clusters <= N:
                raise ValueError("`num_clusters` should lie between 1 and %d." % N)
            merges = N - num_clusters
        else:
            distance = float(distance)
            if math.isnan(distance):
                raise ValueError("`distance` should be a number.")
            merges = int(np.count_nonzero(Z[:, 2] <= distance))
            if np.any(Z[merges:, 2] <= distance):
                raise ValueError("`Z` should hold its merges in ascending height.")
        return _cut(Z, merges)

    def hdbscan(self, min_cluster_size=5, min_samples=None, selection="eom", allow_single_cluster=False,
                return_info=False):
        """Density-based groups of the indexed documents that need no radius (HDBSCAN*; Campello,
        Moulavi & Sander 2013), from ``spanning_tree(min_samples)`` under mutual reachability:
        the single-linkage hierarchy of that tree is condensed -- walking it from the top with
        ``lambda = 1 / max(w, 2 ** -52)``, a split is *true* when both sides hold at least
        ``min_cluster_size`` documents and starts two new clusters; otherwise the documents of a side
        that is too small leave the cluster at that lambda and the cluster goes on -- each cluster
        gets the stability ``sum over its documents of (lambda_leave - lambda_birth)``, and the
        clusters are selected by ``'eom'`` (excess of mass: a cluster is kept when its stability is at
        least the sum of the best below it) or ``'leaf'`` (the leaves of the condensed tree).  Equal
        weights split one edge at a time in the tree's edge order.  The root is selected only with
        ``allow_single_cluster=True``.

        ``min_samples=None`` means ``min_cluster_size``, capped by ``spanning_tree``'s limit
        ``min(len(index), 100)``.  ``min_cluster_size >= 2``, else ValueError.  A weight below one ulp
        of 1 is the rounding of equal rows (see ``neighbors_within``), hence the floor of lambda.

        Returns int32 labels, -1 for noise, the clusters numbered from 0 by ascending smallest member
        id; every document that was in a selected cluster at its birth carries its label.  With
        ``return_info=True`` also a dict: ``probabilities`` (float64, N: lambda of the document over the
        largest lambda of its cluster, 0 for noise), ``stabilities`` (float64, one per returned
        cluster) and ``tree``, the ``(u, v, w)`` used.  The tree comes from the device, the rest is
        host arithmetic."""
        self._live()
        min_cluster_size, selection = _hdbscan_arguments(min_cluster_size, selection)
        N = self._size()
        if min_samples is None:
            min_samples = min(min_cluster_size, N, MAX_TOP_N)
        min_samples = self._min_samples(min_samples, N)
        tree = self.spanning_tree(min_samples)
        labels, prob, stab = _hdbscan_labels(*tree, N, min_cluster_size, selection, allow_single_cluster)
        if not return_info:
            return labels
        return labels, {"probabilities": prob, "stabilities": stab, "tree": tree}

    # -- topic prevalence against document metadata (csrc/effects_kernels.h) ---------
    def group_prevalence(self, labels, weights=None, num_groups=None, return_variance=False, ddof=1):
        """The mean topic proportions of each group of a labelling -- that of ``cluster``, ``dbscan``,
        ``hdbscan`` or any the caller brings (a source, an author, a class).  Returns ``(mean,
        counts)``: ``mean`` float64 K x G in Fortran order like ``cluster``'s centroids, ready for
        ``query_gamma``, ``recommend_gamma`` or ``words_near``, column g being ``S_g / W_g`` with
        ``S_gk = sum_{d in g} w_d theta_dk`` and ``W_g = sum w_d``; ``counts`` int64, the members of
        each group whatever their weights.  A group with ``W_g = 0`` gets a NaN column.

        ``labels``: N integers; -1 leaves a document out; values below -1 or at or above
        ``num_groups`` (default ``max(labels) + 1``) are a ValueError; ``1 <= num_groups <= 4095``,
        else RuntimeError.  ``weights``: N finite values >= 0, not all zero (document lengths give
        token-weighted shares), or None.  With ``return_variance=True`` also ``variance`` (K x G):
        ``(SS_gk / W_g) n_g / (n_g - ddof)`` with ``SS_gk = sum w_d (theta_dk - mean_gk)^2`` and
        ``n_g`` the members of weight > 0 -- without weights ``SS / (n_g - ddof)`` -- and NaN where
        ``n_g - ddof <= 0``.

        A group's members are added by ascending id in chunks of 256, so its column depends on its
        members' rows, their weights and K alone: not on the other groups, their numbering,
        ``num_groups``, ``set_slab_rows`` or how the index was filled.  Nothing of size N x K leaves
        the device."""
        N = len(self)
        lab, G = _group_labels(labels, N, num_groups)
        w = _effects_weights(weights, N)
        handle = self._live()
        mean = np.empty((self._K, G), dtype=np.float64, order="F")
        wsum = np.empty(G, dtype=np.float64)
        counts = np.empty(G, dtype=np.int64)
        ss = np.empty((self._K, G), dtype=np.float64, order="F") if return_variance else None
        _ffi.check(_ffi.lib().trlda_docindex_group_moments(handle, lab.ctypes.data, G,
                                                           None if w is None else w.ctypes.data, mean.ctypes.data,
                                                           wsum.ctypes.data, counts.ctypes.data,
                                                           ss.ctypes.data if return_variance else None))
        if not return_variance:
            return mean, counts
        return mean, counts, _group_variance(ss, wsum, _positive_counts(lab, w, G), ddof, w is not None)

    def topic_trends(self, times, bins=10, weights=None, return_variance=False):
        """Topics over time: ``group_prevalence`` of the documents binned by ``times`` (N values).
        ``bins``: an integer gives that many equal-width bins over the finite times, the last one
        closed, as ``np.histogram`` does; an ascending array is taken as the bins' edges.  Times that
        are not finite or lie outside the edges are left out.  Returns ``(edges, mean, counts)``
        (``mean`` K x bins), with ``return_variance=True`` also the variance."""
        edges, lab = _time_labels(times, bins)
        rest = self.group_prevalence(lab, weights=weights, num_groups=len(edges) - 1,
                                     return_variance=return_variance)
        return (edges,) + tuple(rest)

    def _residuals(self, handle, Z, w, coef):
        """rss (K) of the design Z (N x P, C order) under the coefficients ``coef`` (P x K)."""
        rss = np.empty(self._K, dtype=np.float64)
        rows = np.ascontiguousarray(coef.T)
        _ffi.check(_ffi.lib().trlda_docindex_regress_residuals(handle, Z.ctypes.data, Z.shape[1],
                                                               None if w is None else w.ctypes.data,
                                                               rows.ctypes.data, rss.ctypes.data))
        return rss

    def topic_effects(self, X, weights=None, intercept=True):
        """The least-squares regression of the topic proportions theta (N x K) on covariates ``X``
        (N x P float64, finite, one row per indexed document in id order; a vector is one column):
        the effect of what is known about the documents on topic prevalence.  With ``intercept`` the
        design is ``Z = [1 | X]``; it has ``1 <= P' <= 256`` columns.  ``weights``: N finite values
        >= 0, not all zero, or None.

        Returns a dict: ``coef`` (P' x K), ``stderr`` and ``tvalues`` (P' x K), ``rss`` (K),
        ``sigma2 = rss / dof`` (K), ``dof = nobs - P'``, ``nobs`` (the rows of weight > 0), ``gram``
        (``Z^T W Z``, P' x P') and ``cov_unscaled`` (its inverse), and with an intercept ``tss`` (the
        weighted sum of squares about the weighted mean, K) and ``r2 = 1 - rss / tss``.  With
        ``dof <= 0`` ``sigma2``, ``stderr`` and ``tvalues`` are NaN.  A rank-deficient design is a
        ValueError.

        The Gram matrix and ``Z^T W theta`` are formed on the device and solved on the host after
        equilibration; the residuals are then formed explicitly on the device from the returned
        coefficients, not from the products.  Nothing of size N x K leaves the device or is written
        on it."""
        N = len(self)
        intercept = bool(intercept)
        Z = _design(X, N, intercept)
        w = _effects_weights(weights, N)
        nobs = N if w is None else int(np.count_nonzero(w > 0.0))
        P = Z.shape[1]
        if nobs < P:
            raise ValueError(RANK_DEFICIENT)
        handle = self._live()
        gram = np.empty((P, P), dtype=np.float64)
        cross = np.empty((P, self._K), dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_docindex_regress_products(handle, Z.ctypes.data, P,
                                                              None if w is None else w.ctypes.data,
                                                              gram.ctypes.data, cross.ctypes.data))
        coef, _ = _effects_solve(gram, cross)
        rss = self._residuals(handle, Z, w, coef)
        tss = None
        if intercept:
            tss = self._residuals(handle, np.ones((N, 1), dtype=np.float64), w, (cross[0] / gram[0, 0])[None, :])
        return _effects_closing(gram, cross, rss, tss, nobs, intercept)

    # -- classification from topic proportions (csrc/classify_kernels.h) -------------
    def set_classify_slab(self, rows):
        """A/B switch: rows of scratch per slab of the classifier's evaluations, rounded down to whole
        chunks (0: default, what 256 MiB hold).  Results do not depend on it."""
        _ffi.check(_ffi.lib().trlda_docindex_set_classify_slab(self._live(), operator.index(rows)))

    def _classify_set(self, handle, lab, C, w):
        """The labels and weights of a fit to the device, once: (weight sum, counts)."""
        omega = np.zeros(1, dtype=np.float64)
        counts = np.zeros(C, dtype=np.int64)
        _ffi.check(_ffi.lib().trlda_docindex_classify_set(handle, lab.ctypes.data, C,
                                                          None if w is None else w.ctypes.data, omega.ctypes.data,
                                                          counts.ctypes.data))
        return float(omega[0]), counts

    def _classify_eval(self, handle, W):
        """(loss_sum, grad_sum C x K) at the coefficients W (C x K) under the labels that are set."""
        W = np.ascontiguousarray(W, dtype=np.float64)
        loss = np.zeros(1, dtype=np.float64)
        grad = np.empty(W.shape, dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_docindex_classify_eval(handle, W.ctypes.data, loss.ctypes.data, grad.ctypes.data))
        return float(loss[0]), grad

    def classifier_loss(self, coef, labels, weights=None, num_classes=None):
        """The device's part of ``fit_classifier`` on its own: ``(loss_sum, grad_sum, weight_sum)`` of
        the multinomial logistic regression of ``labels`` on theta at the coefficients ``coef``
        (C x K).  With ``z_dc = sum_k theta_dk coef_ck`` and ``p_d = softmax(z_d)``: ``loss_sum = sum_d
        w_d (log sum_c exp(z_dc) - z_{d,y_d})``, ``grad_sum`` (C x K) ``= sum_d w_d (p_dc - [c = y_d])
        theta_dk`` and ``weight_sum = sum_d w_d``, each over the documents with a label >= 0: the sums
        are unnormalised and carry no penalty.  Labels and weights as for ``fit_classifier``.  Two
        calls agree bitwise, whatever ``set_classify_slab`` says and however the index was filled."""
        N = len(self)
        lab, C = _class_labels(labels, N, num_classes)
        w = _effects_weights(weights, N)
        W = _coefficients(coef, self._K, C)
        handle = self._live()
        try:
            omega, _ = self._classify_set(handle, lab, C, w)
            loss, grad = self._classify_eval(handle, W)
        finally:
            _ffi.lib().trlda_docindex_classify_clear(handle)
        return loss, grad, omega

    def fit_classifier(self, labels, num_classes=None, l2=1e-4, weights=None, max_iter=200, tol=1e-6, init=None):
        """Multinomial logistic regression of a label on the indexed documents' topic proportions
        (Blei, Ng & Jordan 2003, section 7.2): the coefficients ``W`` (C x K) that minimise ``F(W) = (1 /
        Omega) sum_d w_d (log sum_c exp(z_dc) - z_{d,y_d}) + (l2 / 2) |W|_F^2`` with ``z_dc = sum_k
        theta_dk W_ck`` and ``Omega = sum_d w_d``, over the documents with ``y_d >= 0``.  There is no
        separate intercept: theta sums to 1, so W contains one.

        ``labels``: N integers -- those of ``cluster``, ``dbscan``, ``hdbscan`` or any the caller
        brings; -1 leaves a document out; values below -1 or at or above ``num_classes`` (default
        ``max(labels) + 1``) are a ValueError; ``2 <= num_classes <= 128``, else RuntimeError.  A class
        without members is allowed: only the penalty acts on its row.  ``weights``: N finite values
        >= 0, not all zero, or None; no labelled document of positive weight is a ValueError.  ``l2``
        must be finite and positive (ValueError): F is then l2-strongly convex and the optimum unique.

        The loss and its gradient are formed on the device (``classifier_loss``); labels and weights
        go there once, and per evaluation C x K doubles go up and 1 + C x K come down.  The optimiser
        is ``lbfgs_minimize`` on the host, from ``init`` (C x K) or zeros, deterministic.  Returns a
        dict: ``coef`` (C x K), ``loss`` (F) and ``grad_norm`` (the largest absolute entry of F's
        gradient) at return, ``iterations``, ``evaluations``, ``converged`` (``grad_norm <= tol``;
        False at ``max_iter`` or when the line search can no longer decrease F -- never an error),
        ``nobs`` (the labelled documents of weight > 0), ``counts`` (int64, the members of each class)
        and ``l2``.  Nothing is drawn."""
        N = len(self)
        lab, C = _class_labels(labels, N, num_classes)
        w = _effects_weights(weights, N)
        l2 = _penalty(l2)
        max_iter = operator.index(max_iter)
        tol = float(tol)
        if max_iter < 0 or not tol >= 0.0:
            raise ValueError("`max_iter` and `tol` should not be negative.")
        W0 = np.zeros((C, self._K), dtype=np.float64) if init is None else _coefficients(init, self._K, C)
        nobs = int(np.count_nonzero(lab >= 0 if w is None else (lab >= 0) & (w > 0.0)))
        if nobs < 1:
            raise ValueError("No labelled document has a positive weight.")
        handle = self._live()
        try:
            omega, counts = self._classify_set(handle, lab, C, w)

            def fun(W):
                loss, grad = self._classify_eval(handle, W)
                return loss / omega + 0.5 * l2 * float(np.sum(W * W)), grad / omega + l2 * W
            fit = lbfgs_minimize(fun, W0, max_iter=max_iter, tol=tol)
        finally:
            _ffi.lib().trlda_docindex_classify_clear(handle)
        fit.update(nobs=nobs, counts=counts, l2=l2)
        return fit

    def predict(self, coef, gamma=None, ids=None, return_proba=False):
        """The class of each scored document under the coefficients ``coef`` (C x K, as
        ``fit_classifier`` returns them): the argmax of the logits ``z_dc = sum_k theta_dk coef_ck``,
        equal logits going to the smaller class id.  int32.  Scored are all indexed documents
        (``gamma`` and ``ids`` both None), the documents ``ids`` (any order, repeats allowed), or new
        documents given by their ``gamma`` (K x M; no E-step); both together are a ValueError.  A
        document gets the same bits whether it is indexed or passed by its gamma.  With
        ``return_proba=True`` also the softmax of the logits, float64 M x C."""
        if ids is not None and gamma is not None:
            raise ValueError("Give `ids` or `gamma`, not both.")
        W = _coefficients(coef, self._K)
        C = W.shape[0]
        handle = self._live()
        N = self._size()
        rows, g, M = self._scored(ids, gamma, N)
        labels = np.empty(M, dtype=np.int32)
        proba = np.empty((M, C), dtype=np.float64) if return_proba else None
        _ffi.check(_ffi.lib().trlda_docindex_classify_predict(handle, W.ctypes.data, C,
                                                              None if g is None else g.ctypes.data, M,
                                                              None if rows is None else rows.ctypes.data,
                                                              labels.ctypes.data,
                                                              proba.ctypes.data if return_proba else None))
        return (labels, proba) if return_proba else labels

    def knn_predict(self, labels, gamma=None, ids=None, top_n=10, weighting="uniform", num_classes=None,
                    return_votes=False):
        """The baseline classifier: the class most of a document's ``top_n`` nearest indexed
        documents carry.  ``labels`` as for ``fit_classifier`` (-1: the document does not vote).  New
        documents are given by ``gamma`` (K x M) and searched with ``query_gamma``; indexed documents
        (``ids``, or all of them) take their neighbours from ``nearest_neighbors``, which leaves the
        own id out: leave-one-out classification.  ``weighting='uniform'`` counts a vote as 1,
        ``'similarity'`` as the neighbour's similarity s; the votes are added in rank order, ties go
        to the smaller class id, and a document none of whose neighbours votes gets -1.  Host
        arithmetic on the two searches' results.  int32; with ``return_votes=True`` also the votes
        (M x C float64)."""
        if weighting not in ("uniform", "similarity"):
            raise ValueError("`weighting` should be 'uniform' or 'similarity'.")
        if ids is not None and gamma is not None:
            raise ValueError("Give `ids` or `gamma`, not both.")
        N = len(self)
        lab, C = _class_labels(labels, N, num_classes)
        if gamma is not None:
            nearest, sim = self.query_gamma(gamma, top_n=top_n, return_similarity=True)
        else:
            rows = _silhouette_ids(ids, N)
            nearest, sim = self.nearest_neighbors(top_n=top_n, return_similarity=True)
            if rows is not None:
                nearest, sim = nearest[rows], sim[rows]
        pred, votes = knn_votes(nearest, sim, lab, C, weighting)
        return (pred, votes) if return_votes else pred

    # -- the map (csrc/tsne_kernels.h) ----------------------------------------------
    def set_tsne_tile(self, rows):
        """A/B switch: rows per workgroup of the map's repulsion kernel (0: default).  Results do not
        depend on it."""
        _ffi.check(_ffi.lib().trlda_docindex_set_tsne_tile(self._live(), operator.index(rows)))

    def _size(self):
        N = int(_ffi.lib().trlda_docindex_size(self._live()))
        if N < 1:
            raise RuntimeError("The index is empty.")
        return N

    def nearest_neighbors(self, top_n=10, return_similarity=False, block_rows=0):
        """The k-nearest-neighbour graph of the index on itself: for every indexed document its
        ``top_n`` nearest *other* documents in ``query``'s total order (s descending, id ascending),
        its own id removed -- by id, so documents with equal rows find each other.  Returns ``(ids,
        dist)``, int64 and float64 of shape (N, top_n); with ``return_similarity=True`` the
        similarity s in place of the distance.  ``1 <= top_n <= min(N - 1, 99)``, else RuntimeError.
        The table's own rows are the query rows, ``block_rows`` at a time (0: automatic): no gamma
        makes a round trip and the table is not copied.  The result does not depend on
        ``block_rows``, on ``set_slab_rows`` or on how the index was filled."""
        handle = self._live()
        N = self._size()
        top_n = operator.index(top_n)
        block_rows = operator.index(block_rows)
        if not 1 <= top_n <= min(N - 1, MAX_NEIGHBORS):
            raise RuntimeError("`top_n` should lie between 1 and min(len(index) - 1, %d)." % MAX_NEIGHBORS)
        if block_rows < 0:
            raise ValueError("`block_rows` should not be negative.")
        ids = np.empty((N, top_n), dtype=np.int64)
        sim = np.empty((N, top_n), dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_docindex_nearest(handle, top_n, block_rows, ids.ctypes.data, sim.ctypes.data))
        return self._result(ids, sim, return_similarity)

    def affinities(self, perplexity=30.0, return_conditional=False, block_rows=0):
        """The t-SNE affinities of the indexed documents: per document the conditional distribution
        ``p_{j|i} = exp(-beta_i d_j) / sum`` over its ``k = min(N - 1, floor(3 * perplexity))`` nearest
        neighbours, ``d_j = D_ij - D_i,first`` with ``D_ij = max(0, 1 - s_ij)`` (the squared Hellinger
        distance, or the cosine distance), ``beta_i`` calibrated on the device so that the row's
        entropy is ``log(perplexity)``; then ``P_ij = (p_{j|i} + p_{i|j}) / (2 N)`` on the union
        pattern, on the host.  ``1 <= perplexity <= 33``, else ValueError.  A row with ``k <=
        perplexity`` is uniform over its k neighbours (beta 0); a row whose m nearest are exactly tied
        with ``m >= perplexity`` is uniform over those m (beta +inf).

        Returns ``(indptr, ids, p)``: a CSR of N rows, int64, int64 and float64, ascending id within a
        row, bitwise symmetric, summing to 1 up to rounding.  ``return_conditional=True`` returns
        ``(ids N x k, p N x k, beta N)`` as the device left them, in ``nearest_neighbors``' order."""
        handle = self._live()
        N = self._size()
        perplexity = _perplexity(perplexity)
        block_rows = operator.index(block_rows)
        if block_rows < 0:
            raise ValueError("`block_rows` should not be negative.")
        k = min(N - 1, int(math.floor(3.0 * perplexity)))
        ids = np.empty((N, k), dtype=np.int64)
        p = np.empty((N, k), dtype=np.float64)
        beta = np.zeros(N, dtype=np.float64)
        if N > 1:
            _ffi.check(_ffi.lib().trlda_docindex_affinities(handle, perplexity, block_rows, ids.ctypes.data,
                                                            p.ctypes.data, beta.ctypes.data))
        return (ids, p, beta) if return_conditional else _symmetrise(ids, p)

    def embedding_gradient(self, Y, affinities, exaggeration=1.0):
        """The t-SNE gradient and KL divergence of the map ``Y`` (N x 2) under ``affinities`` (the CSR
        ``(indptr, ids, p)`` of ``affinities()`` or any valid one for this N): with ``q_ij = 1 / (1 +
        |y_i - y_j|^2)``, ``Z = sum_{i != j} q_ij``, ``grad_i = 4 (exaggeration * sum_j P_ij q_ij (y_i -
        y_j) - sum_{j != i} q_ij^2 (y_i - y_j) / Z)`` and ``kl = sum_{P_ij > 0} P_ij log(P_ij Z / q_ij)``
        (P without the exaggeration).  All N^2 pairs are formed, in float64 and a fixed order: two calls
        agree bitwise, whatever ``set_tsne_tile`` says.  Returns ``(grad N x 2, kl)``."""
        handle = self._live()
        N = self._size()
        y = _map(Y, N, "Y")
        indptr, ids, p = _affinities(affinities, N)
        exaggeration = float(exaggeration)
        if not math.isfinite(exaggeration):
            raise ValueError("`exaggeration` should be finite.")
        grad = np.zeros((N, 2), dtype=np.float64)
        kl = C.c_double(0.0)
        if N > 1:
            _ffi.check(_ffi.lib().trlda_docindex_tsne_gradient(handle, indptr.ctypes.data, ids.ctypes.data,
                                                               p.ctypes.data, y.ctypes.data, exaggeration,
                                                               grad.ctypes.data, C.byref(kl)))
        return grad, kl.value

    def _pca_start(self, N):
        """The PCA start of a map: theta^ - mean projected on the two leading eigenvectors of the
        scatter, scaled so that the first column's standard deviation is 1e-4."""
        mean, scatter = self._moments()
        axes = _pca_axes(scatter, N)
        y = np.empty((N, 2), dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_docindex_tsne_project(self._live(), mean.ctypes.data, axes.ctypes.data,
                                                          y.ctypes.data))
        return y

    def embed(self, perplexity=30.0, num_iterations=750, init="pca", learning_rate="auto", early_exaggeration=12.0,
              exaggeration_iterations=250, momentum=(0.5, 0.8), affinities=None, return_info=False):
        """A 2-D map of the indexed documents by exact t-SNE (van der Maaten & Hinton 2008) in the
        index's own measure: ``affinities(perplexity)`` (or the CSR given as ``affinities``), then
        ``num_iterations`` steps of ``embedding_gradient`` with gains and momentum, all on the device
        with one wait at the end.  Iteration t uses ``early_exaggeration`` and ``momentum[0]`` while
        ``t < exaggeration_iterations``, then 1 and ``momentum[1]``; elementwise ``same = (g > 0) ==
        (v > 0)``, ``gain = same ? 0.8 gain : gain + 0.2``, ``gain = max(gain, 0.01)``, ``v = momentum v -
        learning_rate gain g``, ``y += v``; then the column means are subtracted.
        ``learning_rate='auto'`` is ``max(N / early_exaggeration / 4, 50)``.

        ``init='pca'`` starts from theta^ minus its mean projected on the two leading eigenvectors of
        ``topic_covariance`` (each signed so that its largest-magnitude component is positive; the
        eigenvectors come from ``numpy.linalg.eigh`` on the host, the projection runs on the device),
        scaled so that the first column's standard deviation is 1e-4; an N x 2 array is taken as it is.
        The repulsion is exact -- all N^2 pairs every iteration, no Barnes-Hut or FFT approximation -- and
        every sum has a fixed order, so two calls agree bitwise.  Nothing is drawn.

        Returns Y, float64 N x 2; with ``return_info=True`` also a dict: ``kl`` (float64,
        ``num_iterations``: the KL divergence before each update), ``iterations``, ``learning_rate``.
        One indexed document gives ``[[0, 0]]``."""
        handle = self._live()
        N = self._size()
        num_iterations = operator.index(num_iterations)
        exaggeration_iterations = operator.index(exaggeration_iterations)
        if num_iterations < 0 or exaggeration_iterations < 0:
            raise ValueError("`num_iterations` and `exaggeration_iterations` should not be negative.")
        early_exaggeration = float(early_exaggeration)
        if not (early_exaggeration > 0.0 and math.isfinite(early_exaggeration)):
            raise ValueError("`early_exaggeration` should be finite and positive.")
        try:
            mom0, mom1 = (float(v) for v in momentum)
        except (TypeError, ValueError):
            raise ValueError("`momentum` should be a pair of numbers.")
        if not (math.isfinite(mom0) and math.isfinite(mom1)):
            raise ValueError("`momentum` should be finite.")
        if isinstance(learning_rate, str):
            if learning_rate != "auto":
                raise ValueError("`learning_rate` should be 'auto' or a number.")
            lr = max(N / early_exaggeration / 4.0, 50.0)
        else:
            lr = float(learning_rate)
            if not (lr > 0.0 and math.isfinite(lr)):
                raise ValueError("`learning_rate` should be finite and positive.")
        if isinstance(init, str):
            if init != "pca":
                raise ValueError("`init` should be 'pca' or an N x 2 array.")
            y = None
        else:
            y = _map(init, N, "init").copy()
        if affinities is None:
            perplexity = _perplexity(perplexity)
        else:
            affinities = _affinities(affinities, N)
        # (every argument has been checked: the device comes in from here)
        kl = np.zeros(num_iterations, dtype=np.float64)
        if N == 1:
            y = np.zeros((1, 2), dtype=np.float64)
        else:
            indptr, ids, p = self.affinities(perplexity) if affinities is None else affinities
            if y is None:
                y = self._pca_start(N)
            _ffi.check(_ffi.lib().trlda_docindex_tsne_run(handle, indptr.ctypes.data, ids.ctypes.data, p.ctypes.data,
                                                          y.ctypes.data, num_iterations, exaggeration_iterations,
                                                          early_exaggeration, lr, mom0, mom1, kl.ctypes.data))
        if not return_info:
            return y
        return y, {"kl": kl, "iterations": num_iterations, "learning_rate": lr}


def _perplexity(perplexity):
    perplexity = float(perplexity)
    if not 1.0 <= perplexity <= MAX_PERPLEXITY:
        raise ValueError("`perplexity` should lie between 1 and %d." % MAX_PERPLEXITY)
    return perplexity


def _map(Y, N, name):
    """A map as contiguous float64 N x 2, or the documented error."""
    try:
        y = np.ascontiguousarray(Y, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("`%s` should be of type `ndarray`." % name)
    if y.shape != (N, 2):
        raise ValueError("`%s` should be of shape (%d, 2)." % (name, N))
    if not np.all(np.isfinite(y)):
        raise ValueError("`%s` should be finite." % name)
    return y


def _affinities(affinities, N):
    """``(indptr, ids, p)`` as contiguous int64, int64, float64 for a map of N documents, or ValueError."""
    try:
        indptr, ids, p = affinities
    except (TypeError, ValueError):
        raise ValueError("`affinities` should be the triple (indptr, ids, p).")
    indptr, ids, p = np.asarray(indptr), np.asarray(ids), np.asarray(p)
    if indptr.dtype.kind not in "iu" or ids.dtype.kind not in "iu" or p.dtype.kind not in "fiu":
        raise ValueError("`affinities` should hold integer `indptr` and `ids` and real `p`.")
    if indptr.ndim != 1 or indptr.shape[0] != N + 1:
        raise ValueError("`affinities` were built for %d documents, not %d." % (max(indptr.size - 1, 0), N))
    if ids.ndim != 1 or p.ndim != 1 or ids.shape != p.shape:
        raise ValueError("`affinities`: `ids` and `p` should be one-dimensional and of one length.")
    if int(indptr[0]) != 0 or int(indptr[-1]) != ids.shape[0] or np.any(np.diff(indptr) < 0):
        raise ValueError("`affinities`: `indptr` should rise from 0 to len(ids).")
    if ids.shape[0] and (int(ids.min()) < 0 or int(ids.max()) >= N):
        raise ValueError("`affinities`: ids should lie between 0 and %d." % (N - 1))
    p = np.ascontiguousarray(p, dtype=np.float64)
    if not (np.all(np.isfinite(p)) and np.all(p >= 0.0)):
        raise ValueError("`affinities`: p should be finite and not negative.")
    return np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(ids, dtype=np.int64), p


def _symmetrise(ids, p):
    """The closing arithmetic of ``affinities``: ``P_ij = (p_{j|i} + p_{i|j}) / (2 N)`` on the union
    pattern of the conditional rows (ids, p: N x k), as a CSR with ascending id within a row."""
    N, k = ids.shape
    rows = np.repeat(np.arange(N, dtype=np.int64), k)
    cols = ids.reshape(-1)
    r = np.concatenate((rows, cols))
    c = np.concatenate((cols, rows))
    v = np.concatenate((p.reshape(-1), p.reshape(-1)))
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    if not len(r):
        return np.zeros(N + 1, dtype=np.int64), np.empty(0, dtype=np.int64), np.empty(0, dtype=np.float64)
    head = np.flatnonzero(np.concatenate(([True], (r[1:] != r[:-1]) | (c[1:] != c[:-1]))))
    # (a pair holds one or two terms: their sum is the same bits in either order)
    P = np.add.reduceat(v, head) / (2.0 * N)
    indptr = np.searchsorted(r[head], np.arange(N + 1, dtype=np.int64)).astype(np.int64)
    return indptr, np.ascontiguousarray(c[head]), P


def _pca_axes(scatter, N):
    """The two leading eigenvectors of the scatter matrix (2 x K), each signed so that its
    largest-magnitude component is positive, scaled so that the first projection's standard
    deviation ``sqrt(l_1 / N)`` becomes 1e-4 (a scatter without spread: zeros)."""
    K = scatter.shape[0]
    w, V = np.linalg.eigh(scatter)
    axes = np.zeros((2, K), dtype=np.float64)
    for c in range(min(2, K)):
        a = V[:, K - 1 - c]
        axes[c] = a if a[np.argmax(np.abs(a))] > 0 else -a
    top = float(w[K - 1])
    return np.ascontiguousarray(axes * (1e-4 / math.sqrt(top / N) if top > 0.0 else 0.0))


def _document_labels(labels, N):
    """(labels, smallest, largest) of one integer label per document of an index of N, or the documented
    error; what `labels` may hold is the caller's to check, before it narrows them to int32."""
    lab = np.asarray(labels)
    if lab.dtype.kind not in "iu":
        raise TypeError("`labels` should be an array of integers.")
    if N < 1:
        raise RuntimeError("The index is empty.")
    if lab.ndim != 1 or lab.shape[0] != N:
        raise RuntimeError("`labels` should hold one label per indexed document (%d)." % N)
    low, high = int(lab.min()), int(lab.max())
    return lab, low, high


def _silhouette_labels(labels, N):
    """(labels as contiguous int32, C) of ``silhouette``'s labels for an index of N documents, or the
    documented error; no device is needed."""
    lab, low, high = _document_labels(labels, N)
    if low < 0 or high >= MAX_CLUSTERS:
        raise RuntimeError("`labels` should lie between 0 and %d." % (MAX_CLUSTERS - 1))
    if low == high:                                          # (the smallest is also the largest: one cluster)
        raise ValueError("A silhouette needs at least two clusters with members.")
    return np.ascontiguousarray(lab, dtype=np.int32), high + 1


def _silhouette_ids(ids, N):
    """``silhouette``'s ids as contiguous int64 (None: every document), or the documented error."""
    if ids is None:
        return None
    rows = np.asarray(ids)
    if rows.dtype.kind not in "iu":
        raise TypeError("`ids` should be an array of integers.")
    if rows.ndim != 1 or rows.shape[0] < 1:
        raise RuntimeError("`ids` should be a one-dimensional array of at least one id.")
    if int(rows.min()) < 0 or int(rows.max()) >= N:
        raise RuntimeError("`ids` should be ids of indexed documents, between 0 and %d." % (N - 1))
    return np.ascontiguousarray(rows, dtype=np.int64)


def _roots(parent):
    """Union-find: every entry of ``parent`` (in place) becomes the root of its tree."""
    while True:
        up = parent[parent]
        if np.array_equal(up, parent):
            return parent
        parent[:] = up


def _union(parent, a, b):
    """Union-find over the edges (a[i], b[i]), all at once: the larger of two roots is hung under the
    smaller until no edge joins two trees, so a tree's root is its smallest member."""
    while len(a):
        ra, rb = _roots(parent)[a], parent[b]
        apart = ra != rb
        a, b = a[apart], b[apart]
        np.minimum.at(parent, np.maximum(ra, rb)[apart], np.minimum(ra, rb)[apart])


def _nearest(nearest, rows, hit, dist):
    """Per document of ``rows`` its first hit in the order (distance ascending, id ascending), into
    ``nearest``; the three arrays hold one entry per (document, hit) pair."""
    if not len(rows):
        return
    order = np.lexsort((hit, dist, rows))
    rows, hit = rows[order], hit[order]
    head = np.concatenate(([True], rows[1:] != rows[:-1]))
    nearest[rows[head]] = hit[head]


def _dbscan_labels(parent, core, nearest, return_core=False):
    """The closing arithmetic of ``dbscan``: the cores' trees numbered by ascending root (a tree's
    smallest member), a border document under its nearest core hit, noise -1."""
    root = _roots(parent)
    labels = np.full(len(core), -1, dtype=np.int32)
    labels[core] = np.unique(root[core], return_inverse=True)[1].astype(np.int32)
    border = np.flatnonzero(nearest >= 0)
    labels[border] = labels[nearest[border]]
    return (labels, core) if return_core else labels


def _boruvka_edges(comp, best_j, best_w):
    """One round of Boruvka's algorithm on the host: from every document's lightest edge to another
    component (``best_j``, -1 without one, and its weight) each component's lightest in the order
    (w, lo, hi), an edge chosen from both of its ends kept once.  Returns ``(lo, hi, w)``."""
    N = comp.shape[0]
    rows = np.flatnonzero(best_j >= 0)
    if not len(rows):
        return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64), np.empty(0, dtype=np.float64)
    j = best_j[rows]
    lo, hi, w, c = np.minimum(rows, j), np.maximum(rows, j), best_w[rows], comp[rows]
    order = np.lexsort((hi, lo, w, c))
    c = c[order]
    pick = order[np.concatenate(([True], c[1:] != c[:-1]))]
    once = np.unique(lo[pick] * N + hi[pick], return_index=True)[1]
    pick = pick[once]
    return lo[pick], hi[pick], w[pick]


def _sorted_edges(parts):
    """The rounds' edges as one ``(u, v, w)`` sorted by (w, u, v)."""
    if not parts:
        return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64), np.empty(0, dtype=np.float64)
    u, v, w = (np.concatenate(p) for p in zip(*parts))
    order = np.lexsort((v, u, w))
    return u[order].astype(np.int64), v[order].astype(np.int64), w[order].astype(np.float64)


def _linkage(u, v, w, N):
    """The linkage matrix (N - 1 x 4, SciPy's convention) of the spanning tree ``(u, v, w)`` on N
    documents: the edges in the order (w, u, v), edge t joining the clusters of its two ends into
    cluster N + t.  One pass of union-find over the N - 1 edges; an edge list that is no spanning tree
    is a ValueError."""
    u, v, w = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64), np.asarray(w, dtype=np.float64)
    if not (u.shape == v.shape == w.shape == (N - 1,)):
        raise ValueError("A spanning tree of %d documents has %d edges." % (N, N - 1))
    if N > 1 and (min(u.min(), v.min()) < 0 or max(u.max(), v.max()) >= N):
        raise ValueError("An edge names a document outside [0, %d)." % N)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    order = np.lexsort((hi, lo, w))
    top = list(range(2 * N - 1))                             # union-find over the clusters, path halving
    size = [1] * N + [0] * (N - 1)
    Z = np.empty((N - 1, 4), dtype=np.float64)
    for t, (a, b, h) in enumerate(zip(lo[order].tolist(), hi[order].tolist(), w[order].tolist())):
        while top[a] != a:
            top[a] = top[top[a]]
            a = top[a]
        while top[b] != b:
            top[b] = top[top[b]]
            b = top[b]
        if a == b:
            raise ValueError("The edges close a cycle: not a spanning tree.")
        top[a] = top[b] = N + t
        size[N + t] = size[a] + size[b]
        Z[t] = (min(a, b), max(a, b), h, size[N + t])
    return Z


def _numbered(keys):
    """(labels, kept): int32 labels of the keys -- the distinct keys >= 0 numbered from 0 by ascending
    first position, which is the smallest member id, a negative key -1 -- and the keys in label order."""
    keys = np.asarray(keys, dtype=np.int64)
    labels = np.full(len(keys), -1, dtype=np.int32)
    at = np.flatnonzero(keys >= 0)
    if not len(at):
        return labels, np.empty(0, dtype=np.int64)
    uniq, first, inv = np.unique(keys[at], return_index=True, return_inverse=True)
    by_first = np.argsort(first)
    rank = np.empty(len(uniq), dtype=np.int32)
    rank[by_first] = np.arange(len(uniq), dtype=np.int32)
    labels[at] = rank[inv.reshape(-1)]
    return labels, uniq[by_first]


def _cut(Z, merges):
    """The labels after the first ``merges`` merges of the linkage matrix Z."""
    N = Z.shape[0] + 1
    parent = np.arange(2 * N - 1, dtype=np.int64)
    new = N + np.arange(merges, dtype=np.int64)
    parent[Z[:merges, 0].astype(np.int64)] = new
    parent[Z[:merges, 1].astype(np.int64)] = new
    return _numbered(_roots(parent)[:N])[0]


def _hdbscan_arguments(min_cluster_size, selection):
    min_cluster_size = operator.index(min_cluster_size)
    if min_cluster_size < 2:
        raise ValueError("`min_cluster_size` should be at least 2.")
    if selection not in ("eom", "leaf"):
        raise ValueError("`selection` should be 'eom' or 'leaf'.")
    return min_cluster_size, selection


LAMBDA_FLOOR = 2.0 ** -52                    # weights below one ulp of 1 are the rounding of equal rows


def _condense(Z, N, min_cluster_size):
    """The condensed tree of the linkage matrix Z (N >= 2), walked from the root down, parents before
    children.  Cluster 0 is the root, born at lambda 0.  At a node of height w, ``lambda = 1 /
    max(w, 2 ** -52)``: two sides of at least ``min_cluster_size`` documents start two new clusters
    born at lambda; otherwise a side that is too small leaves the cluster at lambda, all its
    documents with it, and the other side carries the cluster on.  Returns ``(cluster, lam)`` per
    document -- the cluster it left and the lambda it left at -- and per cluster ``(parent, birth,
    size)``, children after parents."""
    left, right = Z[:, 0].astype(np.int64).tolist(), Z[:, 1].astype(np.int64).tolist()
    lam = (1.0 / np.maximum(Z[:, 2], LAMBDA_FLOOR)).tolist()
    size = [1] * N + Z[:, 3].astype(np.int64).tolist()
    own = [0] * (2 * N - 1)                                  # the cluster a node lies in
    gone = [False] * (2 * N - 1)                             # has the node left it, and at which lambda
    out = [0.0] * (2 * N - 1)
    cparent, birth, csize = [-1], [0.0], [N]
    for t in range(N - 2, -1, -1):
        node = N + t
        c, a, b = own[node], left[t], right[t]
        if gone[node]:
            for ch in (a, b):
                own[ch], gone[ch], out[ch] = c, True, out[node]
        elif size[a] >= min_cluster_size and size[b] >= min_cluster_size:
            for ch in (a, b):
                own[ch] = len(cparent)
                cparent.append(c)
                birth.append(lam[t])
                csize.append(size[ch])
        else:
            for ch in (a, b):
                own[ch] = c
                if size[ch] < min_cluster_size:
                    gone[ch], out[ch] = True, lam[t]
    return (np.array(own[:N], dtype=np.int64), np.array(out[:N], dtype=np.float64),
            np.array(cparent, dtype=np.int64), np.array(birth, dtype=np.float64), np.array(csize, dtype=np.int64))


def _hdbscan_labels(u, v, w, N, min_cluster_size, selection="eom", allow_single_cluster=False):
    """The closing arithmetic of ``hdbscan``: the spanning tree ``(u, v, w)`` under mutual reachability
    in, ``(labels int32, probabilities, stabilities)`` out; no device is needed."""
    min_cluster_size, selection = _hdbscan_arguments(min_cluster_size, selection)
    if N == 1:
        if allow_single_cluster:
            return np.zeros(1, dtype=np.int32), np.ones(1), np.zeros(1)
        return np.full(1, -1, dtype=np.int32), np.zeros(1), np.zeros(0)
    cluster, lam, cparent, birth, csize = _condense(_linkage(u, v, w, N), N, min_cluster_size)
    C = len(cparent)
    kids = np.arange(1, C)
    # sum over a cluster's documents of lambda_leave - lambda_birth: those that left it, and those that
    # went on into its two children at the children's birth
    stab = np.bincount(cluster, weights=lam - birth[cluster], minlength=C)
    stab += np.bincount(cparent[kids], weights=csize[kids] * (birth[kids] - birth[cparent[kids]]), minlength=C)
    split = np.zeros(C, dtype=bool)
    split[cparent[kids]] = True
    if selection == "leaf":
        chosen = ~split
    else:
        chosen = np.ones(C, dtype=bool)
        best, below = stab.tolist(), [0.0] * C               # the best of a subtree; the sum over the children
        for c in range(C - 1, -1, -1):
            if split[c] and below[c] > best[c]:
                chosen[c], best[c] = False, below[c]
            if c:
                below[cparent[c]] += best[c]
    if not allow_single_cluster:
        chosen[0] = False
    # a document carries the topmost chosen cluster above the one it left
    rep = np.full(C, -1, dtype=np.int64)
    for c in range(C):
        above = rep[cparent[c]] if c else -1
        rep[c] = above if above >= 0 else (c if chosen[c] else -1)
    keys = rep[cluster]
    labels, kept = _numbered(keys)
    prob = np.zeros(N, dtype=np.float64)
    at = np.flatnonzero(keys >= 0)
    peak = np.zeros(C, dtype=np.float64)
    np.maximum.at(peak, keys[at], lam[at])
    ok = at[peak[keys[at]] > 0.0]
    prob[ok] = lam[ok] / peak[keys[ok]]
    return labels, prob, stab[kept]


def _group_labels(labels, N, num_groups=None):
    """(labels as contiguous int32, G) of ``group_prevalence``'s labels for an index of N documents, or
    the documented error; no device is needed."""
    lab, low, high = _document_labels(labels, N)
    G = max(high + 1, 1) if num_groups is None else operator.index(num_groups)
    if not 1 <= G <= MAX_CLUSTERS - 1:
        raise RuntimeError("`num_groups` should lie between 1 and %d." % (MAX_CLUSTERS - 1))
    if low < -1 or high >= G:
        raise ValueError("`labels` should lie between -1 (left out) and `num_groups` - 1.")
    return np.ascontiguousarray(lab, dtype=np.int32), G


def _effects_weights(weights, N):
    """``weights`` as contiguous float64 (None: no weights), or the documented error."""
    if weights is None:
        return None
    try:
        w = np.array(weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("`weights` should be of type `ndarray`.")
    if w.ndim != 1 or w.shape[0] != N:
        raise RuntimeError("`weights` should hold one weight per indexed document (%d)." % N)
    if not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError("`weights` should be finite and not negative.")
    if not np.any(w > 0.0):
        raise ValueError("`weights` should not all be zero.")
    return np.ascontiguousarray(w)


def _positive_counts(lab, w, G):
    """n_g (float64, G): the members of each group of weight > 0 (all of them without weights)."""
    keep = lab >= 0 if w is None else (lab >= 0) & (w > 0.0)
    return np.bincount(lab[keep], minlength=G).astype(np.float64)


def _group_variance(ss, wsum, npos, ddof, weighted):
    """The closing arithmetic of ``group_prevalence``'s variance on the device's sums (K x G):
    ``(SS / W) n / (n - ddof)``, without weights ``SS / (n - ddof)``; NaN where ``n - ddof <= 0``."""
    rest = npos - ddof
    with np.errstate(divide="ignore", invalid="ignore"):
        var = (ss / wsum[None, :]) * npos[None, :] / rest[None, :] if weighted else ss / rest[None, :]
    var = np.asfortranarray(var)
    var[:, ~(rest > 0)] = np.nan
    return var


def _time_labels(times, bins=10):
    """(edges float64, labels int32) of ``topic_trends``: the bin of each time as ``np.histogram``
    counts it -- half-open bins, the last one closed -- and -1 for a time that is not finite or lies
    outside the edges.  An integer ``bins`` gives equal-width edges over the finite times."""
    try:
        t = np.array(times, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("`times` should be of type `ndarray`.")
    if t.ndim != 1:
        raise RuntimeError("`times` should be a one-dimensional array.")
    finite = np.isfinite(t)
    if np.ndim(bins) == 0:
        count = operator.index(bins)
        if count < 1:
            raise ValueError("`bins` should be at least 1.")
        if not finite.any():
            raise ValueError("`times` holds no finite value to place the bins by.")
        edges = np.histogram_bin_edges(t[finite], count)
    else:
        try:
            edges = np.array(bins, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError("`bins` should be an integer or an array of edges.")
        if edges.ndim != 1 or edges.shape[0] < 2:
            raise RuntimeError("`bins` should hold at least two edges.")
        if not np.all(np.isfinite(edges)) or np.any(np.diff(edges) < 0):
            raise ValueError("The edges in `bins` should be finite and ascending.")
    lab = np.searchsorted(edges, t, side="right") - 1
    lab[t == edges[-1]] = len(edges) - 2
    with np.errstate(invalid="ignore"):
        lab[~finite | (t < edges[0]) | (t > edges[-1])] = -1
    return edges, lab.astype(np.int32)


RANK_DEFICIENT = "the design matrix is rank deficient"


def _design(X, N, intercept):
    """The design Z (N x P', float64, C order) of ``topic_effects``, or the documented error."""
    if X is None:
        raise TypeError("`X` should be of type `ndarray`.")
    try:
        x = np.array(X, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("`X` should be of type `ndarray`.")
    if N < 1:
        raise RuntimeError("The index is empty.")
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    if x.ndim != 2 or x.shape[0] != N:
        raise RuntimeError("`X` should hold one row per indexed document (%d)." % N)
    P = x.shape[1] + (1 if intercept else 0)
    if not 1 <= P <= MAX_DESIGN_COLUMNS:
        raise RuntimeError("The design should have between 1 and %d columns, the intercept included."
                           % MAX_DESIGN_COLUMNS)
    if not np.all(np.isfinite(x)):
        raise ValueError("`X` should be finite.")
    Z = np.empty((N, P), dtype=np.float64)
    if intercept:
        Z[:, 0] = 1.0
    Z[:, P - x.shape[1]:] = x
    return Z


def _effects_solve(gram, cross):
    """(coef P' x K, cov_unscaled P' x P') of the normal equations ``G b = C``: equilibrated by
    ``D = diag(G)^-1/2``, ``D G D`` solved in float64, ``coef = D solve``.  ValueError where the
    equilibrated Gram matrix is not positive definite or its smallest eigenvalue is at or below
    ``P' 2^-52`` times the largest."""
    G = np.asarray(gram, dtype=np.float64)
    Cx = np.asarray(cross, dtype=np.float64)
    P = G.shape[0]
    diag = np.diag(G)
    if not (np.all(np.isfinite(G)) and np.all(diag > 0.0)):
        raise ValueError(RANK_DEFICIENT)
    d = 1.0 / np.sqrt(diag)
    A = G * d[:, None] * d[None, :]
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        raise ValueError(RANK_DEFICIENT)
    ev = np.linalg.eigvalsh(A)
    if not ev[0] > P * 2.0 ** -52 * ev[-1]:
        raise ValueError(RANK_DEFICIENT)
    coef = d[:, None] * np.linalg.solve(A, d[:, None] * Cx)
    inv = np.linalg.solve(A, np.eye(P))
    inv = 0.5 * (inv + inv.T)
    return coef, d[:, None] * inv * d[None, :]


def _effects_closing(gram, cross, rss, tss, nobs, intercept):
    """The closing arithmetic of ``topic_effects`` on the device's sums: ``gram`` (P' x P'), ``cross``
    (P' x K), ``rss`` (K) and, with an intercept, ``tss`` (K); ``nobs`` the rows of weight > 0."""
    gram = np.asarray(gram, dtype=np.float64)
    cross = np.asarray(cross, dtype=np.float64)
    rss = np.asarray(rss, dtype=np.float64)
    P, K = cross.shape
    nobs = int(nobs)
    if nobs < P:
        raise ValueError(RANK_DEFICIENT)
    coef, cov = _effects_solve(gram, cross)
    dof = nobs - P
    if dof > 0:
        sigma2 = rss / float(dof)
        stderr = np.sqrt(sigma2[None, :] * np.diag(cov)[:, None])
        with np.errstate(divide="ignore", invalid="ignore"):
            tvalues = coef / stderr
    else:
        sigma2 = np.full(K, np.nan)
        stderr = np.full((P, K), np.nan)
        tvalues = np.full((P, K), np.nan)
    out = {"coef": coef, "stderr": stderr, "tvalues": tvalues, "rss": rss, "sigma2": sigma2, "dof": dof,
           "nobs": nobs, "gram": gram, "cov_unscaled": cov}
    if intercept:
        tss = np.asarray(tss, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["tss"], out["r2"] = tss, 1.0 - rss / tss
    return out


def _class_labels(labels, N, num_classes=None):
    """(labels as contiguous int32, C) of the classifiers' labels for an index of N documents, or the
    documented error; no device is needed."""
    lab, low, high = _document_labels(labels, N)
    C = high + 1 if num_classes is None else operator.index(num_classes)
    if not 2 <= C <= MAX_CLASSES:
        raise RuntimeError("`num_classes` should lie between 2 and %d." % MAX_CLASSES)
    if low < -1 or high >= C:
        raise ValueError("`labels` should lie between -1 (left out) and `num_classes` - 1.")
    return np.ascontiguousarray(lab, dtype=np.int32), C


def _coefficients(coef, K, C=None):
    """``coef`` as contiguous float64 C x K, or the documented error."""
    try:
        W = np.array(coef, dtype=np.float64, order="C")
    except (TypeError, ValueError):
        raise TypeError("`coef` should be of type `ndarray`.")
    if W.ndim != 2 or W.shape[1] != K or (C is not None and W.shape[0] != C):
        raise RuntimeError("`coef` should hold one row of %d coefficients per class." % K)
    if not 2 <= W.shape[0] <= MAX_CLASSES:
        raise RuntimeError("The number of classes should lie between 2 and %d." % MAX_CLASSES)
    if not np.all(np.isfinite(W)):
        raise ValueError("`coef` should be finite.")
    return np.ascontiguousarray(W)


def _penalty(l2):
    l2 = float(l2)
    if not (l2 > 0.0 and math.isfinite(l2)):
        raise ValueError("`l2` should be finite and positive.")
    return l2


def lbfgs_minimize(fun, W0, max_iter=200, tol=1e-6, memory=LBFGS_MEMORY):
    """L-BFGS (Nocedal 1980; the two-loop recursion with ``memory`` pairs, the first direction scaled
    by ``s.y / y.y``) with a backtracking line search, on float64 arrays of any one shape:
    ``fun(W) -> (F, grad)``.  Deterministic: every inner product is ``np.sum(a * b)``.

    The step t starts at 1 (``1 / |grad|_2``, capped at 1, while the memory is empty) and is halved
    until ``F(W + t d) <= F(W) + 1e-4 t grad.d`` (Armijo).  Near the optimum the decrease of F falls
    below its rounding -- about ``|grad|^2 / (2 l2)`` against ``2^-52 F`` -- long before the gradient
    stops shrinking, so a step whose F differs from F(W) by no more than ``64 * 2^-52 |F|`` is also
    taken when it shrinks the slope, ``|grad(W + t d).d| <= 0.9 |grad.d|`` (the approximate Wolfe
    condition of Hager & Zhang 2005).  A direction that is not a descent direction, or a search that
    fails after 40 halvings, drops the memory and tries the steepest descent once; if that fails too
    the search can no longer decrease F and the loop ends.

    Stops at ``max |grad| <= tol`` (``converged``), at ``max_iter`` iterations or at the failed
    search.  Returns a dict: ``coef``, ``loss``, ``grad_norm`` (max |grad|), ``iterations``,
    ``evaluations``, ``converged``."""
    W = np.array(W0, dtype=np.float64)
    F, g = fun(W)
    F, g = float(F), np.asarray(g, dtype=np.float64)
    evaluations, iterations = 1, 0
    S, Y, RHO = [], [], []
    eps = 64.0 * 2.0 ** -52
    while iterations < max_iter and not float(np.max(np.abs(g))) <= tol:
        stepped = False
        for attempt in (0, 1):
            if attempt == 1:
                if not S:
                    break
                S, Y, RHO = [], [], []
            q = g.copy()
            alphas = []
            for s, y, rho in zip(reversed(S), reversed(Y), reversed(RHO)):
                a = rho * float(np.sum(s * q))
                alphas.append(a)
                q = q - a * y
            if S:
                q = q * (float(np.sum(S[-1] * Y[-1])) / float(np.sum(Y[-1] * Y[-1])))
            for (s, y, rho), a in zip(zip(S, Y, RHO), reversed(alphas)):
                b = rho * float(np.sum(y * q))
                q = q + s * (a - b)
            d = -q
            slope = float(np.sum(g * d))
            if not slope < 0.0:
                continue
            t = 1.0 if S else min(1.0, 1.0 / math.sqrt(float(np.sum(g * g))))
            for _ in range(40):
                Wn = W + t * d
                Fn, gn = fun(Wn)
                Fn, gn = float(Fn), np.asarray(gn, dtype=np.float64)
                evaluations += 1
                if math.isfinite(Fn) and np.all(np.isfinite(gn)):
                    if Fn <= F + 1e-4 * t * slope:
                        stepped = True
                    elif abs(Fn - F) <= eps * max(abs(F), abs(Fn)) and \
                            abs(float(np.sum(gn * d))) <= 0.9 * abs(slope):
                        stepped = True
                if stepped:
                    break
                t *= 0.5
            if stepped:
                break
        if not stepped:
            break
        s, y = Wn - W, gn - g
        sy = float(np.sum(s * y))
        if sy > 0.0:
            S.append(s)
            Y.append(y)
            RHO.append(1.0 / sy)
            if len(S) > memory:
                S.pop(0), Y.pop(0), RHO.pop(0)
        W, F, g = Wn, Fn, gn
        iterations += 1
    grad_norm = float(np.max(np.abs(g)))
    return {"coef": W, "loss": F, "grad_norm": grad_norm, "iterations": iterations, "evaluations": evaluations,
            "converged": bool(grad_norm <= tol)}


def knn_votes(nearest, sim, labels, num_classes, weighting="uniform"):
    """The vote of ``knn_predict``: ``nearest`` (M x T ids of labelled documents in rank order, a
    negative id: no neighbour), ``sim`` (M x T similarities), ``labels`` (-1: no vote).  Returns
    ``(pred int32 M, votes float64 M x num_classes)``.  The votes are added one rank after the other,
    each rank as one vectorised step over all documents; ties go to the smaller class id; a document
    without a voting neighbour gets -1."""
    nearest = np.asarray(nearest, dtype=np.int64)
    sim = np.asarray(sim, dtype=np.float64)
    labels = np.asarray(labels)
    M, T = nearest.shape
    votes = np.zeros((M, num_classes), dtype=np.float64)
    voted = np.zeros(M, dtype=bool)
    rows = np.arange(M)
    for j in range(T):
        nb = nearest[:, j]
        lab = np.where(nb >= 0, labels[np.maximum(nb, 0)], -1)
        v = lab >= 0
        add = sim[:, j] if weighting == "similarity" else np.ones(M)
        votes[rows[v], lab[v]] = votes[rows[v], lab[v]] + add[v]
        voted |= v
    pred = np.argmax(votes, axis=1).astype(np.int32)
    pred[~voted] = -1
    return pred, votes


def _correlation(scatter):
    """The closing arithmetic of ``topic_correlations`` on the scatter matrix S (host, K x K)."""
    var = np.diag(scatter)
    sd = np.sqrt(np.maximum(var, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        # (the two roots apart: S_ii S_jj underflows where sqrt(S_ii) sqrt(S_jj) does not)
        corr = np.clip(scatter / (sd[:, None] * sd[None, :]), -1.0, 1.0)
    flat = ~(var > 0.0)
    corr[np.arange(len(var)), np.arange(len(var))] = 1.0
    corr[flat, :] = np.nan
    corr[:, flat] = np.nan
    return corr
