"""The NumPy restatement of the left-to-right sampler (tests/l2r_host.py) on its own, without a
GPU: it estimates the enumerated marginal of a short document without bias in the 'particle'
combination, its two combinations coincide at one particle, and the sequential sampler is exact on
single-token documents."""
import functools
import math

import numpy as np
import pytest

import l2r_host as lh
from marginal_host import exact_log_marginal

T_BOUND = 9.0
REPLICATES = 20000

# the document of test_gpu_marginal.py::test_exact_marginal_of_a_short_document
LAM = np.array([[5., 1., 2., .5], [1., 4., 1., 3.], [2., 2., 6., 1.]])
ALPHA = np.array([0.5, 0.2, 1.0])
DOC = [(0, 2), (1, 1), (2, 2), (3, 1)]
WORDS = [0, 0, 1, 2, 2, 3]


def _exact():
    return exact_log_marginal(LAM / LAM.sum(axis=1)[:, None], ALPHA, WORDS)


@functools.lru_cache(maxsize=None)
def _replicates(R, resample, key, reps=REPLICATES):
    """The p tables of `reps` copies of the document, copy i at index i of a batch: N x reps x R."""
    inv = 1.0 / LAM.sum(axis=1)
    P = lh.table(DOC, LAM, inv, ALPHA, np.arange(reps * R), key, resample)
    P = P.reshape(len(WORDS), reps, R)
    P.flags.writeable = False                                # (shared among the tests)
    return P


@pytest.mark.parametrize("R,resample", [(1, True), (1, False), (4, True), (4, False)])
def test_particle_combination_is_unbiased(R, resample):
    """R_i = exp(loglik_i - exact) over 20 000 replicates (index i supplies independent streams):
    their mean is within t = 9 SE of 1, SE from the spread of the means of 20 groups of 1 000.
    Observed |mean - 1| / SE: R = 1 resample 0.33 (mean 0.99879, SE 3.7e-3), R = 1 sequential 1.77
    (0.99459, 3.1e-3), R = 4 resample 1.29 (0.99740, 2.0e-3), R = 4 sequential 2.55 (1.00248, 9.8e-4).
    An independent NumPy version had given 0.78, 0.66, 0.15 and 0.76."""
    ll = lh.combine(_replicates(R, resample, 0x1234567 + R), "particle")
    ratio = np.exp(ll - _exact())
    groups = ratio.reshape(20, -1).mean(axis=1)
    se = groups.std(ddof=1) / math.sqrt(20)
    print("R=%d resample=%s: mean %.6f SE %.3e |mean - 1| / SE %.3f" %
          (R, resample, ratio.mean(), se, abs(ratio.mean() - 1) / se))
    assert se > 0 and abs(ratio.mean() - 1.0) <= T_BOUND * se, (ratio.mean(), se)


def test_position_combination_is_recorded_not_asserted():
    """Wallach's per-position mean over R = 4 particles, as published: mean(loglik) - exact was
    -0.046 in the independent version and is -0.0469 here (resample; the 'particle' form gives
    -0.0356 on the same tables, the Jensen gap of an unbiased estimate of p), and the mean of
    exp(loglik - exact) is 0.9844 +- 0.0019, 8.1 SE from 1 (the independent version: 0.9854 +-
    0.0019): the form is biased, the bias does not shrink with R, and nothing is
    asserted on it beyond its being a finite number below 0."""
    P = _replicates(4, True, 0x1234567 + 4)
    pos, par = lh.combine(P, "position"), lh.combine(P, "particle")
    exact = _exact()
    ratio = np.exp(pos - exact)
    se = ratio.reshape(20, -1).mean(axis=1).std(ddof=1) / math.sqrt(20)
    print("position R=4: mean(ll) - exact %.4f (particle %.4f); mean ratio %.4f SE %.2e t %.1f" %
          (pos.mean() - exact, par.mean() - exact, ratio.mean(), se, abs(ratio.mean() - 1) / se))
    assert np.all(np.isfinite(pos)) and np.all(pos < 0)


@pytest.mark.parametrize("resample", [True, False])
def test_one_particle_both_combinations_are_the_same_bits(resample):
    P = _replicates(1, resample, 99, reps=500)
    a, b = lh.combine(P, "particle"), lh.combine(P, "position")
    assert np.array_equal(a, b)
    rng = np.random.RandomState(3)
    K, V = 70, 30
    lam = rng.gamma(.5, 1., (K, V)) + .01
    docs = [[(int(w), int(c)) for w, c in zip(rng.randint(0, V, 9), rng.randint(0, 3, 9))], [], [(4, 0)]]
    indptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])])
    ids = np.array([w for d in docs for w, _ in d])
    cnts = np.array([c for d in docs for _, c in d])
    out, tokens = lh.left_to_right(indptr, ids, cnts, lam, np.full(K, .1), 7, 1, resample)
    assert np.array_equal(out["particle"], out["position"])
    assert out["particle"][1] == 0.0 and out["particle"][2] == 0.0       # no tokens: exactly 0
    assert tokens.tolist() == [float(cnts[:9].sum()), 0., 0.]


@pytest.mark.parametrize("seed", [1, 2, 77])
def test_sequential_sampler_on_single_token_documents(seed):
    """One token, no resampling: the histogram's total is sum_k beta_kw alpha_k whatever is drawn,
    so loglik = log(sum_k beta_kw alpha_k / A) for every particle and both combinations."""
    rng = np.random.RandomState(5)
    K, V, R = 100, 40, 3
    lam = rng.gamma(.5, 1., (K, V)) + .01
    alpha = rng.gamma(2., .1, K) + .02
    beta = lam / lam.sum(axis=1)[:, None]
    indptr = np.arange(V + 1)
    ids, cnts = np.arange(V), np.ones(V, dtype=np.int64)
    out, tokens = lh.left_to_right(indptr, ids, cnts, lam, alpha, seed * 0x9E3779B97F4A7C15 % 2 ** 64, R, False)
    want = np.log((beta * alpha[:, None]).sum(axis=0) / alpha.sum())
    for how in ("particle", "position"):
        assert np.max(np.abs(out[how] - want) / np.abs(want)) < 1e-12, how
    assert np.all(tokens == 1.0)


def test_symbol_and_method_exist(hip_lib):
    from trlda_amd import _ffi
    from trlda_amd.models import LDA
    assert "trlda_model_left_to_right" in _ffi.EXPORTED_SYMBOLS
    assert hasattr(hip_lib, "trlda_model_left_to_right")
    assert callable(LDA.left_to_right)
    blob = open(_ffi.LIB_PATH, "rb").read()
    assert b"l2r_docs_kernel" in blob and b"l2r_finish_kernel" in blob


def test_arguments_are_refused_before_any_device_work():
    from trlda_amd import _ffi
    from trlda_amd.models import OnlineLDA
    m = OnlineLDA.__new__(OnlineLDA)             # no constructor: nothing here may reach the library
    m._K, m._V, m._handle = 3, 4, None
    for bad in ("wallach", "", None, 3):
        with pytest.raises(TypeError, match="combine"):
            m.left_to_right([DOC], combine=bad)
    with pytest.raises(RuntimeError, match="num_particles"):
        m.left_to_right([DOC], num_particles=0)
    with pytest.raises(RuntimeError, match="2\\^32"):
        m.left_to_right([DOC, DOC], num_particles=2 ** 31)
    with pytest.raises(TypeError):
        m.left_to_right([DOC], num_particles=2.5)
    m._K = 1025
    with pytest.raises(_ffi.TrldaError, match="1024 topics") as info:
        m.left_to_right([DOC])
    assert info.value.code == _ffi.ERR_ARG


def test_kernels_do_not_spill_vector_registers(hip_lib):
    """The five per-lane variants of l2r_docs_kernel (1, 2, 4, 8, 16 topics per lane) keep everything
    in registers: 59, 76, 108, 172 and 300 of the 512 a wave of a four-wave workgroup may have (the
    last: 256 architectural ones and 44 accumulation registers), no scratch."""
    import os
    from helpers import kernel_resources
    from trlda_amd import _ffi
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    res = {k: v for k, v in kernel_resources(_ffi.LIB_PATH).items() if "l2r_docs_kernel" in k}
    assert len(res) == 5, sorted(res)
    for name, f in res.items():
        assert f["vgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_count"] <= 512, (name, f)
