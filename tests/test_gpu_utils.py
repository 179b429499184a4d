"""trlda.utils on the GPU: polygamma of arrays and tensors (csrc/polygamma.h) against the
reference (f14) and bitwise against the host scalar; sample_dirichlet (csrc/dirichlet_kernels.h)
against its NumPy restatement, its determinism rules, its random stream, its errors and its law;
random_select after a model has drawn ahead."""
import ctypes as C

import numpy as np
import pytest

from helpers import golden

pytestmark = pytest.mark.gpu


def _class(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 0, np.where(v == np.inf, 1, np.where(v == -np.inf, 2, 3)))


def _state():
    from trlda_amd import _ffi
    s = np.zeros(33, dtype=np.uint32)
    _ffi.lib().trlda_rng_get_state(s)
    return s


def _key():
    from trlda_amd import _ffi
    key = C.c_uint64(0)
    _ffi.check(_ffi.lib().trlda_rng_draw_key(C.byref(key)))
    return key.value


# ---- polygamma ------------------------------------------------------------------------------
def test_polygamma_arrays_match_the_reference_and_the_host_bitwise(hip_lib):
    from test_utils_host import _cancels
    from trlda.utils import polygamma
    f = golden("f14_polygamma")
    x = f["x"]
    for row, n in enumerate(f["n"]):
        n = int(n)
        ref = f["y"][row]
        dev = polygamma(n, x)
        assert dev.shape == (len(x), 1) and dev.flags.f_contiguous
        dev = dev[:, 0]
        assert np.array_equal(_class(dev), _class(ref)), n
        fin = np.isfinite(ref) & ~_cancels(n, x)
        err = np.abs(dev[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
        assert err.max() <= 1e-13, (n, err.max())
        host = np.array([polygamma(n, float(v)) for v in x])
        # the same code on both sides: the same bits, nan included (n = 0 as well)
        assert np.array_equal(dev.view(np.uint64), host.view(np.uint64)), (n, x[dev != host])


def test_digamma_far_below_zero_on_the_device(hip_lib):
    from trlda.utils import polygamma
    f = golden("f14_polygamma")
    x = f["x_far"]
    for row, n in enumerate(f["n_far"]):
        dev = polygamma(int(n), x)[:, 0]
        ref = f["y_far"][row]
        assert np.max(np.abs(dev - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-13
        host = np.array([polygamma(int(n), float(v)) for v in x])
        assert np.array_equal(dev.view(np.uint64), host.view(np.uint64))


def test_polygamma_random_arguments_bitwise_host_and_device(hip_lib):
    from trlda.utils import polygamma
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.uniform(-60, 60, 3000), np.exp(rng.uniform(-30, 30, 3000))])
    for n in (0, 1, 2, 4, 7, 30):
        dev = polygamma(n, x)[:, 0]
        host = np.array([polygamma(n, float(v)) for v in x])
        assert np.array_equal(dev.view(np.uint64), host.view(np.uint64)), n


def test_polygamma_orders_and_shapes(hip_lib):
    from trlda.utils import polygamma
    rng = np.random.default_rng(5)
    a = rng.uniform(0.1, 30.0, (7, 5))
    for src in (np.ascontiguousarray(a), np.asfortranarray(a), a[:, ::1].T.T):
        out = polygamma(1, src)
        assert out.shape == (7, 5) and out.flags.f_contiguous
        want = np.array([[polygamma(1, float(v)) for v in r] for r in a])
        assert np.array_equal(out, want)
    ints = polygamma(2, np.array([1, 2, 3]))                 # converted to float64
    assert ints.shape == (3, 1) and np.array_equal(ints[:, 0], [polygamma(2, float(v)) for v in (1, 2, 3)])
    lst = polygamma(0, [0.5, 1.5])
    assert lst.shape == (2, 1)
    strided = np.arange(1.0, 41.0).reshape(4, 10)[:, ::3]   # not contiguous: copied
    assert np.array_equal(polygamma(1, strided), polygamma(1, np.ascontiguousarray(strided)))


def test_polygamma_tensor_stays_on_the_device(hip_lib):
    torch = pytest.importorskip("torch")
    from trlda.utils import polygamma
    g = torch.Generator(device="cuda").manual_seed(7)
    t = torch.rand(2 ** 22, device="cuda", dtype=torch.float64, generator=g) * 40.0 - 5.0
    for n in (0, 1, 3):
        y = polygamma(n, t)
        assert isinstance(y, torch.Tensor) and y.device == t.device and y.shape == t.shape
        assert y.dtype == torch.float64
        ref = polygamma(n, t.cpu().numpy())[:, 0]
        assert np.array_equal(y.cpu().numpy().view(np.uint64), ref.view(np.uint64))
    t2 = t[:1000].reshape(10, 100)
    y2 = polygamma(1, t2)
    assert y2.shape == (10, 100)
    assert np.array_equal(y2.cpu().numpy(), polygamma(1, t2.cpu().numpy()))
    with pytest.raises(RuntimeError, match="double"):
        polygamma(1, t.float())


def test_polygamma_second_opinion_scipy(hip_lib):
    special = pytest.importorskip("scipy.special")
    from trlda.utils import polygamma
    x = np.concatenate([np.linspace(0.05, 50.0, 400), np.logspace(-3, 6, 200)])
    for n in (0, 1, 2, 3, 6):
        dev = polygamma(n, x)[:, 0]
        want = special.polygamma(n, x)
        err = np.abs(dev - want) / np.maximum(np.abs(want), 1.0)
        assert err.max() < 1e-13, (n, err.max())


# ---- sample_dirichlet ------------------------------------------------------------------------
SHAPES = [(1, 5), (2, 100), (5, 100), (64, 3), (65, 3), (1024, 4), (1025, 4), (5000, 3), (100000, 2)]


@pytest.mark.parametrize("m,n", SHAPES)
def test_sample_dirichlet_matches_the_restatement(hip_lib, m, n):
    import trlda
    from dirichlet_host import sample_dirichlet as restated
    from trlda.utils import sample_dirichlet
    for alpha in (0.1, 2.5):
        trlda.seed(1000 + m)
        key = _key()
        trlda.seed(1000 + m)
        out = sample_dirichlet(m, n, alpha)
        assert out.shape == (m, n) and out.flags.f_contiguous and out.dtype == np.float64
        want = restated(m, n, alpha, key)
        assert np.all(np.isfinite(out)) and np.all(out >= 0)
        assert np.max(np.abs(out - want) / np.maximum(want, 1e-300)) < 1e-12 or \
            np.max(np.abs(out - want)) < 1e-15, (m, n, alpha)
        assert np.max(np.abs(out.sum(axis=0) - 1.0)) < 1e-12


@pytest.mark.parametrize("m,n", [(1, 7), (5, 33), (64, 9), (65, 9), (1024, 5), (1025, 5), (9000, 3), (100000, 2)])
def test_sample_dirichlet_summation_order_is_bitwise(hip_lib, m, n):
    """The device's own W and S (the test hook stops before the divide): S restated from W in the
    kernels' order is the same bits, and W / S is the call's output, bit for bit."""
    import trlda
    from dirichlet_host import column_sums
    from trlda_amd import _ffi
    from trlda.utils import sample_dirichlet
    trlda.seed(70 + m)
    key = _key()
    W = np.empty((m, n), order="F")
    S = np.empty(n)
    _ffi.check(_ffi.lib().trlda_debug_dirichlet_sums(m, n, 0.4, key, W.ctypes.data, S.ctypes.data, 0))
    assert np.all(W.max(axis=0) == 1.0)
    assert np.array_equal(column_sums(W).view(np.uint64), S.view(np.uint64))
    trlda.seed(70 + m)
    out = sample_dirichlet(m, n, 0.4)
    assert np.array_equal((W / S).view(np.uint64), out.view(np.uint64))


def test_sample_dirichlet_more_columns_than_one_launch(hip_lib):
    """n past 4 (2^24 - 1) columns: the wave path splits into two launches (2^24 - 1 workgroups
    of 256 at most); the last columns are the restatement's and every column is a simplex point."""
    import trlda
    from dirichlet_host import sample_dirichlet as restated
    from trlda.utils import sample_dirichlet
    n = 2 ** 26 + 5
    trlda.seed(90)
    key = _key()
    trlda.seed(90)
    out = sample_dirichlet(2, n, 0.5)
    assert out.shape == (2, n)
    assert np.all(out >= 0.0) and np.all(out <= 1.0)
    assert np.max(np.abs(out.sum(axis=0) - 1.0)) < 1e-12
    cols = np.array([0, 1, 4 * (2 ** 24 - 1) - 1, 4 * (2 ** 24 - 1), 4 * (2 ** 24 - 1) + 1, n - 2, n - 1])
    want = restated(2, n, 0.5, key, columns=cols)
    assert np.max(np.abs(out[:, cols] - want)) < 1e-15


@pytest.mark.parametrize("m", [3, 1024, 1025, 9000])
def test_sample_dirichlet_columns_do_not_depend_on_n(hip_lib, m):
    import trlda
    from trlda.utils import sample_dirichlet
    trlda.seed(21)
    wide = sample_dirichlet(m, 9, 0.3)
    trlda.seed(21)
    narrow = sample_dirichlet(m, 4, 0.3)
    assert np.array_equal(wide[:, :4], narrow)


def test_sample_dirichlet_stream_and_reproducibility(hip_lib):
    import trlda
    from trlda.utils import sample_dirichlet
    trlda.seed(8)
    a = sample_dirichlet(10, 50, 1.0)
    b = sample_dirichlet(10, 50, 1.0)
    trlda.seed(8)
    assert np.array_equal(sample_dirichlet(10, 50, 1.0), a)
    assert not np.array_equal(a, b)
    for m, n in ((10, 50), (0, 5), (5, 0), (0, 0), (3000, 2)):
        trlda.seed(9)
        _key()
        want = _state()
        trlda.seed(9)
        out = sample_dirichlet(m, n, 0.5)
        assert out.shape == (m, n)
        assert np.array_equal(_state(), want), (m, n)          # exactly two draws


def test_sample_dirichlet_edges(hip_lib):
    import trlda
    from trlda.utils import sample_dirichlet
    trlda.seed(4)
    tiny = sample_dirichlet(50, 400, 1e-3)
    assert not np.isnan(tiny).any() and np.max(np.abs(tiny.sum(axis=0) - 1.0)) < 1e-12
    big = sample_dirichlet(2000, 3, 1e-3)
    assert not np.isnan(big).any() and np.max(np.abs(big.sum(axis=0) - 1.0)) < 1e-12
    assert np.array_equal(sample_dirichlet(1, 7, 0.2), np.ones((1, 7)))
    assert sample_dirichlet(0, 3, 1.0).shape == (0, 3) and sample_dirichlet(3, 0, 1.0).shape == (3, 0)
    before = _state()
    for args in ((-1, 3, 1.0), (3, -1, 1.0), (3, 3, 0.0), (3, 3, -1.0), (3, 3, np.inf), (3, 3, np.nan)):
        with pytest.raises(RuntimeError):
            sample_dirichlet(*args)
    assert np.array_equal(_state(), before)                    # a refused call draws nothing
    out = sample_dirichlet(4, 6, 2.0, device=0)
    assert out.shape == (4, 6)


def test_sample_dirichlet_law(hip_lib):
    from scipy.stats import ks_2samp
    import trlda
    from trlda.utils import sample_dirichlet
    N = 20000
    for K in (2, 5, 10):
        for alpha in (.1, .5, 1., 4., 50.):
            trlda.seed(K * 100 + int(alpha * 10))
            s = sample_dirichlet(K, N, alpha)
            mean = 1.0 / K
            var = mean * (1 - mean) / (K * alpha + 1)
            m_hat = s.mean(axis=1)
            v_hat = s.var(axis=1)
            m4 = ((s - m_hat[:, None]) ** 4).mean(axis=1)
            assert np.all(np.abs(m_hat - mean) < 5 * np.sqrt(var / N)), (K, alpha, m_hat)
            assert np.all(np.abs(v_hat - var) < 5 * np.sqrt((m4 - v_hat ** 2) / N)), (K, alpha, v_hat, var)
            rng = np.random.RandomState(K * 1000 + int(alpha * 10))
            other = rng.dirichlet(np.full(K, alpha), size=N).T
            assert ks_2samp(other.ravel(), s.ravel())[1] > 1e-6, (K, alpha)


# ---- random_select after a model drew ahead -------------------------------------------------
def test_random_select_after_a_model_drew_ahead(hip_lib):
    import trlda
    from trlda_amd import _ffi
    from trlda_amd.documents import CSRDocuments
    from trlda_amd.models import OnlineLDA
    from trlda_amd.utils.synthetic import make_corpus
    from trlda.utils import random_select
    docs = CSRDocuments(*make_corpus(32, 300, seed=3, mean_unique=20))
    picks = []
    for ahead in (1, 0):
        trlda.seed(31)
        model = OnlineLDA(num_words=300, num_topics=8, num_documents=1000, device=0)
        _ffi.check(_ffi.lib().trlda_model_set_draw_ahead(model._handle, ahead))
        model.update_parameters(docs, max_iter_tr=1, max_iter_inference=10)
        picks.append((random_select(7, 100), random_select(90, 100), _state()))
    assert picks[0][0] == picks[1][0] and picks[0][1] == picks[1][1]
    assert np.array_equal(picks[0][2], picks[1][2])
