"""``trlda`` -- the reference's import path, served by the MI355X implementation.

The reference package (python/__init__.py:1-9) exposes ``trlda.seed`` and the subpackages
``trlda.models`` (python/models/__init__.py:1-5) and ``trlda.utils``
(python/utils/__init__.py); each name here is the corresponding object of ``trlda_amd``, so a
script written against the reference -- its README example, say -- runs unchanged:

    from trlda.models import OnlineLDA
    from trlda.utils import load_documents

Only the accelerated path exists, together with Gibbs inference on the GPU
(``update_variables(docs, inference_method='gibbs')``) and sampling
documents from a model on the GPU (``sample``).
``predictive_log_likelihood`` scores a model on held-out words on the GPU.
``trlda.utils`` has all six of the reference's names: ``polygamma`` of an array and
``sample_dirichlet`` run on the GPU, ``random_select`` draws from the seeded stream as the
reference does, and ``load_users`` / ``load_users_as_dict`` read rating files (DESIGN.md
section 3.13).
"""
__license__ = 'MIT License <http://www.opensource.org/licenses/mit-license.php>'
__docformat__ = 'epytext'

from trlda_amd import __version__, seed  # noqa: F401

__all__ = ["seed", "models", "utils"]
