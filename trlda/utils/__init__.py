"""``trlda.utils`` (reference python/utils/__init__.py): the loaders (python/utils/load_documents.py,
load_users.py) and the utilities of src/utils.cpp -- polygamma and sample_dirichlet on the GPU,
random_select on the seeded stream."""
from trlda_amd.utils import load_documents, load_documents_csr  # noqa: F401
from trlda_amd.utils import load_users, load_users_as_dict  # noqa: F401
from trlda_amd.utils import polygamma, random_select, sample_dirichlet  # noqa: F401

__all__ = ["load_documents", "load_users", "load_users_as_dict", "random_select", "sample_dirichlet",
           "polygamma", "load_documents_csr"]
