"""NumPy / longdouble restatement of the spectral initialisation (csrc/anchor_kernels.h, DESIGN.md
3.36): the co-occurrence matrix, the fixed-order sums, FastAnchorWords with its near-tie report and
a running error bound, RecoverL2, the rounding allowances for G, H and the Frank-Wolfe gap, and the
planted separable inputs.

Rounding bounds are written in the usual form |fl(sum_i x_i y_i) - sum_i x_i y_i| <= gamma(n) sum_i
|x_i| |y_i| with gamma(n) = n u / (1 - n u), u = 2^-53, n the number of rounded operations an
element passes through."""
import numpy as np

U = 2.0 ** -53
LANES = 256                                     # the partial sums of a fixed-order sum
NEAR_TIE = 1e-9                                 # a relative margin below this is reported, not failed


def gamma(n):
    return n * U / (1.0 - n * U)


def sum_depth(n):
    """additions an element of a fixed-order sum of n values passes through, at most"""
    return -(-n // LANES) + 8


# ---- stage 1: the matrix -------------------------------------------------------------------------

def cooccurrence(batches, V):
    """Q and the counters of a stream of CSR batches: a plain loop over the documents.  Per document
    every element of Q receives at most one addition (its ids are distinct), so adding the block at
    once is the loop itself."""
    Q = np.zeros((V, V))
    doc_freq, word_count = np.zeros(V, np.int64), np.zeros(V, np.int64)
    docs = skipped = tokens = 0
    for csr in batches:
        for d in range(len(csr.indptr) - 1):
            lo, hi = csr.indptr[d], csr.indptr[d + 1]
            ids, c = csr.ids[lo:hi].astype(np.int64), csr.cnts[lo:hi].astype(np.int64)
            assert len(np.unique(ids)) == len(ids) and (c >= 0).all()
            n = int(c.sum())
            if n < 2:
                skipped += 1
                continue
            docs += 1
            tokens += n
            num = np.outer(c, c) - np.diag(c)                  # exact integers
            Q[np.ix_(ids, ids)] += num.astype(np.float64) / float(n * (n - 1))
            doc_freq[ids[c > 0]] += 1
            word_count[ids] += c
    return Q, doc_freq, word_count, docs, skipped, tokens


def fixed_sum(X):
    """The sum of each row of X (rows x n) in the device's order: partial sum t adds the values
    t, t + 256, ... ascending, then p[t] += p[t + s] for s = 128, ..., 1."""
    X = np.atleast_2d(X)
    acc = np.zeros((X.shape[0], LANES), dtype=X.dtype)
    for c0 in range(0, X.shape[1], LANES):
        blk = X[:, c0:c0 + LANES]
        acc[:, :blk.shape[1]] += blk
    s = LANES // 2
    while s:
        acc[:, :s] += acc[:, s:2 * s]
        s //= 2
    return acc[:, 0].copy()


def row_sums(Q):
    r = fixed_sum(Q)
    return r, fixed_sum(r[None, :])[0]


def normalise(Q, r):
    pos = r > 0
    return np.where(pos[:, None], Q / np.where(pos, r, 1)[:, None], 0)


def default_min_doc_freq(num_documents):
    return max(2, -(-5 * num_documents // 1000))


# ---- stage 2: FastAnchorWords ---------------------------------------------------------------------

def anchor_words(Q, num, candidates=None, dtype=np.float64):
    """(ids, winner norm^2, runner-up norm^2, bound): the device's operations in `dtype`.  In float64
    this is the device's arithmetic operation for operation; in longdouble it gives the figures the
    device's scores are held against, and `bound[0][r]` / `bound[1][r]` then bound |float64 score -
    this score| of round r's winner / runner-up (inf where there is no runner-up), each from its own
    row's eps in the recursion below.

    The recursion carries eps_w >= |x^_w - x_w|_2 for every candidate row (x^ the float64 row, x
    this one), with ns = sum_depth(V):
      start     x = q / r: r carries gamma(ns), the division u:        eps = (gamma(ns) + 2u) |x|
      round 0   x' = x_w - x_a:                                        eps' = eps_w + eps_a + u |x'|
      later     u = x_a / |x_a|: normalising a perturbed vector moves it by at most 2 eps_a / |x_a|,
                the norm's sum, the root and the division add gamma(ns + 3):
                                                                       eta = 2 eps_a / |x_a| + gamma(ns + 3)
                d = x_w . u:     dd = (eps_w + gamma(ns + 1) (|x_w| + eps_w)) (1 + eta) + |x_w| eta
                x' = x_w - d u:  eps' = eps_w + dd (1 + eta) + |d| eta + 2u ((|d| + dd) (1 + eta) + |x'| + eps_w)
      score     fl(|x^|^2) against |x|^2:   gamma(ns + 1) (|x| + eps)^2 + 2 |x| eps + eps^2
    """
    Q = np.asarray(Q, dtype=dtype)
    V = Q.shape[0]
    ns = sum_depth(V)
    r = fixed_sum(Q)
    W = normalise(Q, r)
    norm2 = fixed_sum(W * W)
    cand = (r > 0) if candidates is None else (np.asarray(candidates, bool) & (r > 0))
    cand = cand.copy()
    eps = (gamma(ns) + 2 * U) * np.sqrt(norm2)
    ids, score, runner, bound, rbound = [], [], [], [], []

    def score_bound(w):
        nw = np.sqrt(norm2[w])
        with np.errstate(over="ignore", invalid="ignore"):
            return gamma(ns + 1) * (nw + eps[w]) ** 2 + 2 * nw * eps[w] + eps[w] ** 2
    for rnd in range(num):
        idx = np.flatnonzero(cand)
        order = np.lexsort((idx, -norm2[idx]))
        a = idx[order[0]]
        ids.append(int(a))
        score.append(norm2[a])
        runner.append(norm2[idx[order[1]]] if len(idx) > 1 else dtype(-1))
        na = np.sqrt(norm2[a])
        bound.append(score_bound(a))
        rbound.append(score_bound(idx[order[1]]) if len(idx) > 1 else np.inf)
        cand[a] = False
        if rnd + 1 == num:
            break
        rows = np.flatnonzero(cand)
        X = W[rows]
        nx = np.sqrt(norm2[rows])
        if rnd == 0:
            Y = X - W[a]
            n2 = fixed_sum(Y * Y)
            eps[rows] = eps[rows] + eps[a] + U * np.sqrt(n2)
        else:
            u = W[a] / na
            d = fixed_sum(X * u)
            Y = X - d[:, None] * u
            n2 = fixed_sum(Y * Y)
            eta = 2 * eps[a] / na + gamma(ns + 3)
            ew = eps[rows]
            with np.errstate(over="ignore", invalid="ignore"):
                dd = (ew + gamma(ns + 1) * (nx + ew)) * (1 + eta) + nx * eta
            with np.errstate(over="ignore", invalid="ignore"):  # (after many rounds the bound says nothing: inf)
                eps[rows] = ew + dd * (1 + eta) + abs(d) * eta + \
                    2 * U * ((abs(d) + dd) * (1 + eta) + np.sqrt(n2) + ew)
        W[rows] = Y
        norm2[rows] = n2
    return (np.array(ids, np.int32), np.array(score, dtype), np.array(runner, dtype),
            np.array([bound, rbound], np.longdouble))


def near_ties(score, runner):
    """The rounds whose winner leads the runner-up by less than NEAR_TIE relative: [(round, margin)]."""
    out = []
    for r, (s, t) in enumerate(zip(score, runner)):
        if t >= 0 and s > 0 and (s - t) / s < NEAR_TIE:
            out.append((r, float((s - t) / s)))
    return out


# ---- stage 3: RecoverL2 ---------------------------------------------------------------------------

def project_simplex(Vv):
    """rows of Vv onto the simplex (sort-based, exact)"""
    n = Vv.shape[1]
    s = -np.sort(-Vv, axis=1)
    css = np.cumsum(s, axis=1) - 1
    k = np.arange(1, n + 1)
    ok = s - css / k > 0
    rho = n - np.argmax(ok[:, ::-1], axis=1)
    tau = css[np.arange(len(Vv)), rho - 1] / rho
    return np.maximum(Vv - tau[:, None], 0)


def products(Wbar, anchors):
    """H = Wbar Wbar_S' and G = its anchors' rows, in Wbar's dtype"""
    H = Wbar @ Wbar[anchors].T
    return H, H[anchors]


def gap_of(X, G, H):
    """the Frank-Wolfe gap x . g - min g, g = 2 (G x - h), per row"""
    g = 2 * (X @ G - H)
    return (X * g).sum(axis=1) - g.min(axis=1)


def recover(Wbar, anchors, tol=1e-7, max_iter=2000):
    """(x, iterations, relative gaps): the solver of anchor_solve_kernel in Wbar's dtype, every word
    stopping on its own.  Iterates are not meant to match the device's: solutions are."""
    dt = Wbar.dtype
    H, G = products(Wbar, anchors)
    A = len(anchors)
    qq = (Wbar * Wbar).sum(axis=1)
    L = 2 * np.abs(G).sum(axis=1).max()
    live = np.flatnonzero(qq > 0)
    X = np.full((len(Wbar), A), dt.type(1) / A, dtype=dt)
    iters = np.zeros(len(Wbar), np.int32)
    gaps = np.zeros(len(Wbar), dt)
    x = X[live].copy()
    y = x.copy()
    t = np.ones(len(live), dt)
    h = H[live]
    for it in range(1, max_iter + 1):
        if len(live) == 0:
            break
        xn = project_simplex(y - 2 * (y @ G - h) / L)
        gap = gap_of(xn, G, h)
        done = (gap <= tol * qq[live]) | (it == max_iter)
        turn = ((y - xn) * (xn - x)).sum(axis=1) > 0
        tn = (1 + np.sqrt(1 + 4 * t * t)) / 2
        beta = np.where(turn, 0, (t - 1) / tn)
        t = np.where(turn, 1, tn)
        y = xn + beta[:, None] * (xn - x)
        x = xn
        fin = np.flatnonzero(done)
        X[live[fin]] = x[fin]
        iters[live[fin]] = it
        gaps[live[fin]] = gap[fin] / qq[live[fin]]
        keep = ~done
        live, x, y, t, h = live[keep], x[keep], y[keep], t[keep], h[keep]
    return X, iters, gaps


def topics_of(X, p):
    """(beta K x V, pi): column k of x_wk p_w normalised over the words, and its mass"""
    M = X * p[:, None]
    pi = M.sum(axis=0)
    return (M / np.where(pi > 0, pi, 1)).T, pi


def gap_allowance(Wbar, anchors, tol):
    """What the device's own rounding may add to a word's gap over |Wbar_w|^2, per word (Wbar: the
    float64 rows the device holds, taken as exact here; everything below in longdouble).

    All entries are non-negative, so sum |x| |y| of a product is the product itself.
      H, G    V products, each through at most V + 4 additions of the tile product's chains:
              |H^ - H| <= gamma(V + 4) H,  |G^ - G| <= gamma(V + 4) G
      G x     A fused steps:  gamma(A) max G   (x on the simplex)
      g = 2 (G x - h):  |g^ - g| <= 2 (gamma(V + 4) (max G + max h) + (gamma(A) + 2u) (max G + max h))
      gap = x . g - min g:  both terms move by at most max |g^ - g|; the device's dot product adds
              gamma(A / 64 + 8) max |g|, max |g| <= 2 (max G + max h)
      |Wbar_w|^2 on the device: gamma(sum_depth(V) + 1), times tol
    """
    W = Wbar.astype(np.longdouble)
    H, G = products(W, anchors)
    V, A = H.shape
    qq = (W * W).sum(axis=1)
    m = G.max() + H.max(axis=1)
    dg = 2 * (gamma(V + 4) + gamma(A) + 2 * U) * m
    absolute = 2 * dg + gamma(A // 64 + 8) * 2 * m + tol * gamma(sum_depth(V) + 1) * qq
    return np.where(qq > 0, absolute / np.where(qq > 0, qq, 1), 0)


# ---- the planted inputs ---------------------------------------------------------------------------

def planted(K, V, seed=0, alpha_scale=0.1):
    """(Q, beta, anchors): an exactly separable second-moment matrix.  beta from Dirichlet(0.05) +
    1e-6; K distinct anchor words, word k with mass 0.05 (0.5 + k / 2K) in topic k and 0 elsewhere;
    rows renormalised; R = E[theta theta'] in closed form for alpha_k = alpha_scale (1 + k / K);
    Q = beta' R beta (symmetrised, so that it is symmetric bit for bit).  With alpha_scale = 0.1 the
    sum of alpha grows with K and the anchors' rows of Qbar grow alike (at K = 512 each is 98.6 % the
    same mixture, and G is so ill-conditioned that no first-order solver gets to 1e-7 in thousands of
    iterations); a smaller alpha_scale keeps the sum, and the conditioning, that of a small K."""
    rng = np.random.RandomState(seed)
    beta = rng.dirichlet(np.full(V, 0.05), size=K) + 1e-6
    anchors = np.sort(rng.permutation(V)[:K])
    rng.shuffle(anchors)
    beta[:, anchors] = 0.0
    beta[np.arange(K), anchors] = 0.05 * (0.5 + np.arange(K) / (2.0 * K))
    beta /= beta.sum(axis=1, keepdims=True)
    alpha = alpha_scale * (1 + np.arange(K) / float(K))
    a0 = alpha.sum()
    R = (np.outer(alpha, alpha) + np.diag(alpha)) / (a0 * (a0 + 1))
    Q = beta.T @ R @ beta
    Q = (Q + Q.T) / 2
    return Q, beta, anchors.astype(np.int32)


def total_variation(beta_hat, beta, anchors_hat, anchors):
    """max over the topics of half the L1 distance; topic k of beta_hat is the planted topic whose
    anchor is anchors_hat[k]"""
    where = {int(a): k for k, a in enumerate(anchors)}
    perm = [where[int(a)] for a in anchors_hat]
    return float(0.5 * np.abs(np.asarray(beta_hat, np.longdouble) - beta[perm]).sum(axis=1).max())
