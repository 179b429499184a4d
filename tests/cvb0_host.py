"""NumPy restatement of CVB0 as csrc/cvb0_kernels.h pins it (a helper module, not a test file).

It follows the header's contract step by step: lane l of a document's wave holds topics
l*KPL .. l*KPL + KPL - 1 (topics >= K are zeros), a "wave sum" is the lane-local sequential sum
over those KPL values followed by the kernel's butterfly (gibbs_host.wave_allsum), and every +, -,
x and / is one rounded fp64 operation -- which is what NumPy's element-wise arithmetic does.  Given
the same e table, alpha, documents, theta0, max_iter and threshold it reproduces theta, the
statistics and the iteration counts of the kernels bit for bit.

Also: the mean-field (VI) fixed point of one document on the same table, for comparisons.
"""
import numpy as np

from gibbs_host import WAVE, kpl_of, wave_allsum


def wave_sum(v, kpl):
    """v: WAVE * kpl values in topic order.  Lane-local sequential sums (from 0), then the butterfly."""
    s = np.zeros(WAVE)
    lanes = v.reshape(WAVE, kpl)
    for q in range(kpl):
        s = s + lanes[:, q]
    return wave_allsum(s)


def _pad(x, kpl):
    out = np.zeros(WAVE * kpl)
    out[:len(x)] = x
    return out


class Document:
    """The state of one document: phi per kept entry, n, and the sweeps done."""

    def __init__(self, e, alpha, words, counts, theta0=None):
        e = np.asarray(e, dtype=np.float64)
        self.K = e.shape[0]
        self.kpl = kpl_of(self.K)
        self.alpha = _pad(np.asarray(alpha, dtype=np.float64), self.kpl)
        keep = [i for i, c in enumerate(counts) if c > 0]
        self.words = [int(words[i]) for i in keep]
        self.counts = [float(int(counts[i])) for i in keep]
        self.N = sum(int(counts[i]) for i in keep)
        self.e = [_pad(e[:, w], self.kpl) for w in self.words]
        th = self.alpha if theta0 is None else _pad(np.asarray(theta0, dtype=np.float64), self.kpl)
        self.n = np.zeros(WAVE * self.kpl)
        self.phi = []
        self.iters = 0
        self.delta = np.inf
        for c, col in zip(self.counts, self.e):
            a = th * col
            s = wave_sum(a, self.kpl)
            self._check(s)
            inv = 1.0 / s
            phi = a * inv
            self.n = self.n + c * phi
            self.phi.append(phi)

    @staticmethod
    def _check(s):
        if not (s > 0.0 and np.isfinite(s)):
            raise RuntimeError("CVB0: a token's topic weights sum to zero or are not finite.")

    def sweep(self):
        """One Gauss-Seidel sweep; returns delta = (wave sum of |n - nprev|) / K."""
        nprev = self.n.copy()
        for p, (c, col) in enumerate(zip(self.counts, self.e)):
            old = self.phi[p]
            t = self.n - old
            a = (self.alpha + t) * col
            S = wave_sum(a, self.kpl)
            self._check(S)
            inv = 1.0 / S
            new = a * inv
            self.n = (self.n - c * old) + c * new
            self.phi[p] = new
        self.iters += 1
        self.delta = wave_sum(np.abs(self.n - nprev), self.kpl) / float(self.K)
        return self.delta

    def run(self, max_iter, threshold):
        if not self.phi:
            return
        while self.iters < max_iter:
            if self.sweep() < threshold:
                break

    def theta(self):
        denom = wave_sum(self.alpha, self.kpl) + float(self.N)
        return ((self.alpha + self.n) / denom)[:self.K]


def cvb0(e, alpha, indptr, ids, cnts, theta0, max_iter, threshold):
    """The whole call: (theta K x B, sstats K x V, iters B int32, each document's final delta --
    inf where no sweep ran)."""
    e = np.asarray(e, dtype=np.float64)
    K, V = e.shape
    B = len(indptr) - 1
    theta = np.zeros((K, B), order="F")
    sstats = np.zeros((K, V), order="F")
    iters = np.zeros(B, dtype=np.int32)
    deltas = np.full(B, np.inf)
    # documents in batch order, entries in order: the word-major order of the batch index
    for d in range(B):
        lo, hi = int(indptr[d]), int(indptr[d + 1])
        doc = Document(e, alpha, ids[lo:hi], cnts[lo:hi], None if theta0 is None else np.asarray(theta0)[:, d])
        doc.run(max_iter, threshold)
        theta[:, d] = doc.theta()
        iters[d] = doc.iters
        deltas[d] = doc.delta
        for w, c, phi in zip(doc.words, doc.counts, doc.phi):
            sstats[:, w] = sstats[:, w] + c * phi[:K]
    return theta, sstats, iters, deltas


def vi_expected_counts(e, alpha, words, max_iter=10000, tol=1e-15):
    """Mean-field VI of one document whose tokens have word ids `words`, on the table e: the fixed
    point gamma = alpha + sum_i phi_i, phi_i ~ exp(psi(gamma)) e[:, w_i].  Returns
    E[n] = gamma - alpha."""
    from scipy.special import digamma
    e = np.asarray(e, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    gamma = alpha + len(words) / float(len(alpha))
    for _ in range(max_iter):
        w = np.exp(digamma(gamma))[:, None] * e[:, words]
        phi = w / w.sum(axis=0)
        new = alpha + phi.sum(axis=1)
        done = np.max(np.abs(new - gamma)) < tol
        gamma = new
        if done:
            break
    return gamma - alpha
