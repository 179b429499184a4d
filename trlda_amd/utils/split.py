"""Splitting documents into an observed and a held-out part, for the held-out predictive
log-likelihood (``LDA.predictive_log_likelihood``)."""
import ctypes as C

import numpy as np

from .. import _ffi
from ..documents import CSRDocuments, DocumentList, as_csr


def _keep(csr, counts):
    """The entries of ``csr`` whose count in ``counts`` is positive, in their order."""
    keep = counts > 0
    doc = np.repeat(np.arange(len(csr), dtype=np.int64), np.diff(csr.indptr))
    indptr = np.zeros(len(csr) + 1, dtype=np.int64)
    np.cumsum(np.bincount(doc[keep], minlength=len(csr)), out=indptr[1:])
    return DocumentList(CSRDocuments(indptr, csr.ids[keep], counts[keep]))


def split_documents(docs, heldout=0.2):
    """Splits every document's tokens into ``(observed, heldout)``, two ``DocumentList`` of the
    same length: each token goes to the held-out part with probability ``heldout`` (binomial
    thinning of every entry's count).  Each part keeps the entries' order and drops those whose
    count in it is 0.  The random numbers are numpy's Philox keyed by two draws of the seeded
    stream (``trlda_amd.seed`` makes a split reproducible).  ``docs``: a list of documents, a
    ``DocumentList`` or ``CSRDocuments``."""
    heldout = float(heldout)
    if not 0.0 <= heldout <= 1.0:
        raise ValueError("`heldout` should lie in [0, 1].")
    csr = as_csr(docs)
    counts = csr.cnts.astype(np.int64)
    if (counts < 0).any():
        raise ValueError("Word counts should not be negative.")
    key = C.c_uint64(0)
    _ffi.check(_ffi.lib().trlda_rng_draw_key(C.byref(key)))
    rng = np.random.Generator(np.random.Philox(key=key.value))
    held = rng.binomial(counts, heldout)
    return _keep(csr, counts - held), _keep(csr, held)
