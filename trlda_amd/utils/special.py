"""``polygamma``, ``sample_dirichlet`` and ``random_select`` of ``trlda.utils`` (reference
python/src/utilsinterface.cpp over src/utils.cpp): scalars on the host, arrays on the GPU
(csrc/polygamma.h, csrc/dirichlet_kernels.h), the selection on the seeded stream (host_rng.cpp)."""
import ctypes as C
import operator

import numpy as np

from .. import _ffi


def _device(device):
    if device is None:
        from ..models import _default_device
        return _default_device()
    return int(device)


def _int32(value):
    """The binding's "i": an integer that fits in a C int."""
    value = operator.index(value)
    if not -2 ** 31 <= value < 2 ** 31:
        raise OverflowError("signed integer is greater than maximum")
    return value


def _is_gpu_tensor(x):
    if not type(x).__module__.startswith("torch"):
        return False
    import torch
    return isinstance(x, torch.Tensor) and x.device.type == "cuda"


def polygamma(n, x):
    """The polygamma function: psi(x) for n < 1, (-1)^(n+1) n! zeta(n+1, x) for n >= 1
    (src/utils.cpp:107-123).

    A Python ``float`` or ``int`` (``np.float64`` included) gives a ``float``, evaluated on the host.
    Anything else is converted to a float64 array and evaluated on the GPU: a 1-D array of length N
    gives an (N, 1) array and a 2-D array keeps its shape, both Fortran-ordered, as the reference's
    binding returns them; other ranks raise ``RuntimeError``.  A float64 torch tensor on the GPU
    gives a new tensor of the same shape on its device, without a copy through the host.  Host and
    device values are the same bits."""
    n = _int32(n)
    if isinstance(x, (float, int)):
        return float(_ffi.lib().trlda_polygamma(n, float(x)))
    if _is_gpu_tensor(x):
        import torch
        if x.dtype != torch.float64:
            raise RuntimeError("Can only handle tensors of double values.")
        xc = x.contiguous()
        y = torch.empty_like(xc)
        torch.cuda.current_stream(xc.device).synchronize()
        _ffi.check(_ffi.lib().trlda_polygamma_device(n, xc.numel(), C.c_void_p(xc.data_ptr()),
                                                     C.c_void_p(y.data_ptr()), xc.device.index))
        return y
    try:
        arr = np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("`x` should be of type `ndarray`.")
    if arr.ndim == 1:
        arr = arr.reshape(-1, 1)
    elif arr.ndim != 2:
        raise RuntimeError("Can only handle one- and two-dimensional arrays.")
    src = np.asfortranarray(arr)
    out = np.empty(src.shape, dtype=np.float64, order="F")
    if src.size:
        _ffi.check(_ffi.lib().trlda_polygamma_host(n, src.size, src.ctypes.data, out.ctypes.data,
                                                   _device(None)))
    return out


def sample_dirichlet(m, n, alpha, device=None):
    """An m x n float64 array (Fortran-ordered) whose columns are draws from Dirichlet(alpha 1_m)
    (src/utils.cpp:251-266), drawn on the GPU (``device``: the models' default when None).

    The random numbers are Philox keyed by two draws of the seeded stream, so ``trlda.seed`` makes a
    call reproducible, and column j does not depend on n.  ``RuntimeError``
    for m or n < 0 and for alpha not > 0 or not finite."""
    m, n = _int32(m), _int32(n)
    alpha = float(alpha)
    out = np.empty((max(m, 0), max(n, 0)), dtype=np.float64, order="F")
    _ffi.check(_ffi.lib().trlda_sample_dirichlet_host(m, n, alpha, out.ctypes.data if out.size else None,
                                                      _device(device)))
    return out


def random_select(k, n):
    """k of the indices 0 .. n-1, chosen with the seeded stream exactly as the reference's
    randomSelect draws them (src/utils.cpp:351-378), as an ascending list."""
    k, n = _int32(k), _int32(n)
    out = np.zeros(max(min(k, n), 1), dtype=np.int32)          # (the C call checks k and n)
    _ffi.check(_ffi.lib().trlda_random_select(k, n, out))
    return [int(v) for v in out[:k]] if k > 0 else []
