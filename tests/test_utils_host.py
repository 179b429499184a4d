"""trlda.utils on the host: scalar polygamma against the reference (f14), the binding's argument
rules, random_select against glibc's rand() itself, load_users / load_users_as_dict against the
reference's loader (f15), the six exported names, and the new kernels' registers."""
import ctypes
import os

import numpy as np
import pytest

from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _class(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 0, np.where(v == np.inf, 1, np.where(v == -np.inf, 2, 3)))


def _cancels(n, x):
    """Negative half-integers below -1 at even n >= 2: the terms (x + i)^-(n+1) cancel in pairs
    (+-2^(n+1) and the rest), and any direct sum -- the reference's included -- returns rounding
    noise there; those points are compared by class only."""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return (n >= 2) & (n % 2 == 0) & (x < -1) & (np.mod(x, 1.0) == 0.5)


# ---- polygamma ------------------------------------------------------------------------------
def test_scalar_polygamma_matches_the_reference(hip_lib):
    from trlda.utils import polygamma
    f = golden("f14_polygamma")
    x = f["x"]
    for row, n in enumerate(f["n"]):
        n = int(n)
        ref = f["y"][row]
        ours = np.array([polygamma(n, float(v)) for v in x])
        assert np.array_equal(_class(ours), _class(ref)), (n, x[_class(ours) != _class(ref)])
        fin = np.isfinite(ref) & ~_cancels(n, x)
        err = np.abs(ours[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
        assert err.max() <= 1e-13, (n, x[fin][np.argmax(err)], err.max())


def test_scalar_digamma_reflects_far_below_zero(hip_lib):
    # below -2^20 psi reflects, as the reference's digamma does; for n >= 1 the reference's zeta
    # would sum |x| terms one by one, and the library declines (nan)
    from trlda.utils import polygamma
    f = golden("f14_polygamma")
    for row, n in enumerate(f["n_far"]):
        ours = np.array([polygamma(int(n), float(v)) for v in f["x_far"]])
        ref = f["y_far"][row]
        assert np.all(np.isfinite(ours))
        assert np.max(np.abs(ours - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-13, (n, ours, ref)
    assert np.isnan(polygamma(1, -2e6 - 0.5)) and polygamma(1, -1048575.5) < np.inf
    assert polygamma(0, -2.0 ** 40) == np.inf                     # a pole stays a pole


def test_polygamma_known_values(hip_lib):
    # values of psi, psi' and psi'' from tables of the functions (the reference checks the same
    # numbers to seven places); here to 1e-12 relative
    from trlda.utils import polygamma
    known = {(0, .1): -10.423754940411076, (0, 1.): -0.5772156649015329, (0, 120.): 4.783319289118516,
             (1, .01): 10001.621213528313, (1, .1): 101.43329915079276, (1, .4): 7.275356590529597,
             (1, 11.): 0.09516633568168575, (2, 14.): -0.005479465690312488}
    for (n, x), y in known.items():
        assert abs(polygamma(n, x) - y) <= 1e-12 * abs(y), (n, x, polygamma(n, x), y)
    assert polygamma(1, 1) == pytest.approx(np.pi ** 2 / 6, rel=1e-15)
    assert polygamma(0, 0.0) == np.inf and polygamma(2, -3) == -np.inf and polygamma(3, -3) == np.inf
    assert np.isnan(polygamma(1, np.nan)) and polygamma(1, np.inf) == 0.0


def test_polygamma_argument_types(hip_lib):
    from trlda.utils import polygamma
    for x in (2, 2.0, np.float64(2.0), True):
        y = polygamma(1, x)
        assert type(y) is float and y == polygamma(1, float(x))
    with pytest.raises(TypeError):
        polygamma(1.5, 2.0)                      # n is an int ("i")
    with pytest.raises(TypeError):
        polygamma(1, "x")
    with pytest.raises(RuntimeError, match="one- and two-dimensional"):
        polygamma(1, np.ones((2, 2, 2)))
    with pytest.raises(RuntimeError, match="one- and two-dimensional"):
        polygamma(1, np.int64(3))                # not a Python int: a 0-d array
    # empty arrays need no device
    for shape, want in (((0,), (0, 1)), ((0, 3), (0, 3)), ((3, 0), (3, 0))):
        out = polygamma(1, np.empty(shape))
        assert out.shape == want and out.flags.f_contiguous and out.dtype == np.float64


# ---- random_select ---------------------------------------------------------------------------
def _libc():
    libc = ctypes.CDLL("libc.so.6")
    libc.rand.restype = ctypes.c_int
    libc.srand.argtypes = [ctypes.c_uint]
    return libc


def _select_with_libc(libc, k, n):
    """randomSelect restated on glibc's own rand(); returns (indices, number of draws)."""
    draws = 0
    if k <= n // 2:
        chosen = set()
        while len(chosen) < k:
            draws += 1
            chosen.add(libc.rand() % n)
        return sorted(chosen), draws
    left = set(range(n))
    while len(left) > k:
        draws += 1
        left.discard(libc.rand() % n)
    return sorted(left), draws


def _state(hip_lib):
    s = np.zeros(33, dtype=np.uint32)
    hip_lib.trlda_rng_get_state(s)
    return s


@pytest.mark.parametrize("k,n", [(3, 10), (5, 10), (6, 10), (10, 10), (0, 10), (0, 0), (0, 1), (1, 1),
                                 (11, 121), (110, 121), (1, 2), (2, 3), (400, 1000), (999, 1000)])
def test_random_select_is_the_reference_on_glibc_rand(hip_lib, k, n):
    import trlda
    from trlda.utils import random_select
    libc = _libc()
    for seed in (1, 77, 2 ** 31 + 5):
        libc.srand(seed)
        want, draws = _select_with_libc(libc, k, n)
        nxt = [libc.rand() for _ in range(3)]
        trlda.seed(seed)
        got = random_select(k, n)
        assert got == want and all(type(v) is int for v in got)
        after = _state(hip_lib)
        # the next draws of the stream are glibc's next draws: random_select(1, 2^31 - 1) is one
        # rand() % (2^31 - 1)
        assert [random_select(1, 2 ** 31 - 1)[0] for _ in range(3)] == [v % (2 ** 31 - 1) for v in nxt]
        # and the state is the one `draws` single draws reach
        trlda.seed(seed)
        for _ in range(draws):
            random_select(1, 2 ** 31 - 1)
        assert np.array_equal(_state(hip_lib), after)


def test_random_select_errors_and_their_order(hip_lib):
    import trlda
    from trlda.utils import random_select
    trlda.seed(3)
    before = _state(hip_lib)
    with pytest.raises(RuntimeError, match="k must be smaller than n."):
        random_select(10, 4)
    with pytest.raises(RuntimeError, match="k must be smaller than n."):
        random_select(-1, -5)                    # k > n is checked first
    with pytest.raises(RuntimeError, match="n and k must be non-negative."):
        random_select(-1, 4)
    with pytest.raises(RuntimeError, match="n and k must be non-negative."):
        random_select(-3, -2)
    with pytest.raises(TypeError):
        random_select(1.0, 4)
    with pytest.raises(RuntimeError, match="k must be smaller than n."):
        random_select(2 ** 31 - 1, 5)            # refused before any k-sized allocation
    assert np.array_equal(_state(hip_lib), before)          # a refused call draws nothing
    assert set(random_select(8, 8)) == set(range(8))


# ---- load_users -----------------------------------------------------------------------------
def _flatten(batches):
    sizes = [len(b) for b in batches]
    users = [u for b in batches for u in (b.values() if isinstance(b, dict) else b)]
    keys = [k for b in batches if isinstance(b, dict) for k in b.keys()]
    pairs = np.array([t for u in users for t in u], dtype=np.int64).reshape(-1, 2)
    return sizes, [len(u) for u in users], pairs[:, 0], pairs[:, 1], keys


CASES = [("all_t4", None, False, 4, 0), ("all_t3", None, False, 3, 0), ("all_t0", None, False, 0, 0),
         ("b3_t4", 3, False, 4, 0), ("b4_t0", 4, False, 0, 0), ("b50_t3", 50, False, 3, 0),
         ("s2_t4_seed1", 2, True, 4, 1), ("s1_t0_seed2", 1, True, 0, 2), ("s1_t3_seed5", 1, True, 3, 5),
         ("s3_t0_seed7", 3, True, 0, 7)]


@pytest.mark.parametrize("name,batch_size,stochastic,threshold,seed", CASES)
@pytest.mark.parametrize("form", ["list", "dict"])
def test_load_users_matches_the_reference(tmp_path, name, batch_size, stochastic, threshold, seed, form):
    from trlda.utils import load_users, load_users_as_dict
    f = golden("f15_users")
    path = tmp_path / "ratings.txt"
    path.write_bytes(f["text"].tobytes())
    fn = load_users if form == "list" else load_users_as_dict
    np.random.seed(seed)
    res = fn(str(path), batch_size=batch_size, stochastic=stochastic, threshold=threshold)
    batches = list(res) if batch_size else [res]
    want_type = list if form == "list" else dict
    assert all(isinstance(b, want_type) or b == [] for b in batches)
    sizes, lens, items, ratings, keys = _flatten(batches)
    p = "%s_%s_" % (name, form)
    assert sizes == f[p + "sizes"].tolist()
    assert lens == f[p + "lens"].tolist()
    assert np.array_equal(items, f[p + "items"]) and np.array_equal(ratings, f[p + "ratings"])
    if form == "dict":
        assert keys == f[p + "uids"].tolist()


def test_load_users_feed_update_parameters_shapes(tmp_path):
    from trlda_amd.documents import as_csr
    from trlda.utils import load_users
    f = golden("f15_users")
    path = tmp_path / "ratings.txt"
    path.write_bytes(f["text"].tobytes())
    users = load_users(str(path), threshold=0)
    csr = as_csr(users)
    assert len(csr) == len(users)
    assert int(np.asarray(csr.cnts).sum()) == sum(r for u in users for _, r in u)


def test_dirichlet_restated_order_sees_a_different_order():
    """The bitwise check of the device's column sums (test_gpu_utils.py) can tell orders apart:
    on random weights the kernels' order and a plain left-to-right sum differ in some column."""
    from dirichlet_host import column_sums
    rng = np.random.default_rng(2)
    for m in (100, 1024, 5000):
        W = rng.random((m, 200))
        plain = np.array([sum(W[:, j].tolist()) for j in range(W.shape[1])])
        assert not np.array_equal(column_sums(W), plain), m
        assert np.allclose(column_sums(W), plain, rtol=1e-13)


# ---- the surface and the kernels ------------------------------------------------------------
def test_trlda_utils_exports_the_reference_names():
    import trlda.utils
    import trlda_amd.utils
    names = ["load_documents", "load_users", "load_users_as_dict", "random_select", "sample_dirichlet",
             "polygamma"]
    for mod in (trlda.utils, trlda_amd.utils):
        for name in names:
            assert callable(getattr(mod, name)) and name in mod.__all__, (mod, name)
    assert trlda.utils.sample_dirichlet is trlda_amd.utils.sample_dirichlet


def test_new_kernels_have_no_scratch_and_no_spills(hip_lib):
    from helpers import kernel_resources
    from trlda_amd import _ffi
    res = kernel_resources(_ffi.LIB_PATH)
    mine = {k: v for k, v in res.items() if "polygamma_kernel" in k or "dirichlet_" in k}
    assert len(mine) == 7, sorted(mine)
    for name, f in mine.items():
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["vgpr_count"] <= 128, (name, f)
