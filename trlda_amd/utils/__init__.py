"""``trlda_amd.utils`` -- the data-format helpers on either side of the E-step, and the reference's
utilities (python/utils/__init__.py)."""
from .load_documents import load_documents, load_documents_csr  # noqa: F401
from .load_users import load_users, load_users_as_dict  # noqa: F401
from .special import polygamma, random_select, sample_dirichlet  # noqa: F401
from .synthetic import make_corpus, csr_to_docs, docs_to_csr  # noqa: F401
from .split import split_documents  # noqa: F401

__all__ = ["load_documents", "load_documents_csr", "load_users", "load_users_as_dict", "random_select",
           "sample_dirichlet", "polygamma", "make_corpus", "csr_to_docs", "docs_to_csr", "split_documents"]
