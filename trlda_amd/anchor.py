"""``WordCooccurrence``: the word co-occurrence matrix of a corpus stream on the device -- what
``LDA.anchor_words``, ``recover_topics`` and ``initialize_spectral`` work from (csrc/anchor_kernels.h,
DESIGN.md 3.36; Arora et al. 2013).  No reference counterpart."""
import ctypes as C
import operator

import numpy as np

from . import _ffi

DEFAULT_MAX_BYTES = 16 << 30


class WordCooccurrence(object):
    """A device-resident accumulator of Arora's unbiased second-moment estimator: a document with
    counts ``c`` and ``n = sum(c) >= 2`` adds ``((int64) c_w c_v - [w = v] c_w) / (double)(n (n - 1))``
    to ``Q[w, v]`` for every pair of its entries -- an exact integer, then one division.  Documents with
    ``n < 2`` are skipped and counted; the counters (``doc_freq``, ``word_count``, ``num_documents``,
    ``num_tokens``) cover the documents that contributed.

    Row ``w`` of Q belongs to one workgroup per batch, which walks the documents that hold ``w`` in
    ascending order: every (document, pair) is one addition, in document order across the stream, and
    no floating-point atomics are used.  So Q is symmetric bit for bit, does not depend on how the
    corpus is cut into batches, and a plain loop over the documents restates it exactly.

    Q and (from the first ``anchor_words`` / ``recover_topics`` on) one work copy of the same size live
    on the device, rows of ``ceil(V / 4) * 4`` doubles; a vocabulary whose two matrices exceed
    ``max_bytes`` (default 16 GiB) raises RuntimeError naming the bytes needed, before anything is
    allocated.  Made by ``model.word_cooccurrence``; closed with the model."""

    def __init__(self, model, max_bytes=DEFAULT_MAX_BYTES):
        self._handle = None
        _ffi.require_gpu()
        if getattr(model, "_handle", None) is None:
            raise RuntimeError("The model has been closed.")
        max_bytes = operator.index(max_bytes)
        if max_bytes < 0:
            raise RuntimeError("`max_bytes` should not be negative.")
        self._model = model
        self._V = model.num_words
        handle = _ffi.vp()
        _ffi.check(_ffi.lib().trlda_anchor_create(model._handle, max_bytes, C.byref(handle)))
        self._handle = handle
        self._has_doc_freq = True
        model._register_index(self)

    @classmethod
    def from_matrix(cls, model, Q, doc_freq=None, max_bytes=DEFAULT_MAX_BYTES):
        """An accumulator holding the given symmetric, non-negative, finite V x V matrix (anything else
        raises RuntimeError) and, unless None, ``doc_freq`` (V non-negative integers).  Without
        ``doc_freq`` every word with a positive row sum is a candidate of ``anchor_words``."""
        try:
            q = np.ascontiguousarray(Q, dtype=np.float64)
        except (TypeError, ValueError):
            raise RuntimeError("`Q` should be a square matrix of floats.")
        V = model.num_words
        if q.shape != (V, V):
            raise RuntimeError("`Q` should have shape (num_words, num_words).")
        df = None
        if doc_freq is not None:
            df = np.ascontiguousarray(doc_freq)
            if df.shape != (V,) or not np.issubdtype(df.dtype, np.integer):
                raise RuntimeError("`doc_freq` should hold num_words integers.")
            df = np.ascontiguousarray(df, dtype=np.int64)
        self = cls(model, max_bytes)
        try:
            _ffi.check(_ffi.lib().trlda_anchor_load(self._live(), q.ctypes.data,
                                                    None if df is None else df.ctypes.data))
        except Exception:
            self.close()
            raise
        self._has_doc_freq = df is not None
        return self

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_handle", None):
            _ffi.lib().trlda_anchor_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self._handle:
            raise RuntimeError("The accumulator has been closed.")
        return self._handle

    # -- feeding ----------------------------------------------------------------------------------
    def add(self, docs):
        """Adds a batch (a list of documents, ``DocumentList``, ``CSRDocuments`` or a ``DeviceBatch``
        of this model) or an iterator of batches, as ``topic_coherence`` takes them.  A batch with a
        negative count, or one that lists a word twice in a document, raises RuntimeError and adds
        nothing.  Returns the accumulator."""
        handle = self._live()
        model = self._model
        for part in (docs if hasattr(docs, "__next__") else (docs,)):
            batch, owned = model._batch(part)
            try:
                _ffi.check(_ffi.lib().trlda_anchor_add(handle, batch.handle))
            finally:
                if owned:
                    batch.close()
        return self

    # -- reading ----------------------------------------------------------------------------------
    def _counts(self):
        V = self._V
        df, wc, counters = (np.empty(V, dtype=np.int64), np.empty(V, dtype=np.int64),
                            np.empty(3, dtype=np.int64))
        _ffi.check(_ffi.lib().trlda_anchor_counts(self._live(), df, wc, counters))
        return df, wc, counters

    @property
    def num_words(self):
        return self._V

    @property
    def has_doc_freq(self):
        return self._has_doc_freq

    @property
    def doc_freq(self):
        """int64, per word the contributing documents that hold it with a positive count."""
        return self._counts()[0]

    @property
    def word_count(self):
        """int64, per word the sum of its counts over the contributing documents."""
        return self._counts()[1]

    @property
    def num_documents(self):
        """Documents that contributed (``n >= 2``)."""
        return int(self._counts()[2][0])

    @property
    def num_skipped(self):
        """Documents skipped (``n < 2``)."""
        return int(self._counts()[2][1])

    @property
    def num_tokens(self):
        """The sum of the counts of the contributing documents."""
        return int(self._counts()[2][2])

    def read(self, rows=None):
        """Rows of Q (all of them, V x V, when ``rows`` is None), float64, C order."""
        V = self._V
        if rows is None:
            out = np.empty((V, V), dtype=np.float64)
            _ffi.check(_ffi.lib().trlda_anchor_read(self._live(), None, V, out.ctypes.data))
            return out
        try:
            ids = np.asarray(rows)
        except (TypeError, ValueError):
            raise RuntimeError("`rows` should be a one-dimensional array of word ids.")
        if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
            raise RuntimeError("`rows` should be a one-dimensional array of word ids.")
        if ids.size and (ids.min() < 0 or ids.max() >= V):
            raise RuntimeError("Word id out of range in `rows`.")
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.empty((len(ids), V), dtype=np.float64)
        _ffi.check(_ffi.lib().trlda_anchor_read(self._live(), ids.ctypes.data, len(ids), out.ctypes.data))
        return out

    def row_sums(self):
        """``(r, total)``: the row sums of Q and their sum.  Every sum of n values is taken in one
        order: with 256 partial sums, partial sum t adds the values t, t + 256, ... in ascending
        order starting from +0, then the partial sums are folded as ``p[t] += p[t + s]`` for
        s = 128, 64, ..., 1 (``total`` is that sum of ``r``)."""
        r = np.empty(self._V, dtype=np.float64)
        total = C.c_double(0.0)
        _ffi.check(_ffi.lib().trlda_anchor_row_sums(self._live(), r.ctypes.data, C.byref(total)))
        return r, float(total.value)

    def word_probabilities(self):
        """``p_w = sum_v Q[w, v] / sum(Q)``, the sums in the order ``row_sums`` documents, one
        division each.  An empty accumulator raises RuntimeError."""
        r, total = self.row_sums()
        if not total > 0.0:
            raise RuntimeError("The co-occurrence matrix is empty.")
        return r / total

    def _set_gram_lds(self, mode):
        """0: the solver holds G in LDS up to 128 anchors (default); 1: never.  Same bits."""
        _ffi.check(_ffi.lib().trlda_anchor_set_gram_lds(self._live(), int(mode)))
