"""NumPy restatement of the classification of indexed documents from their topic proportions
(csrc/classify_kernels.h).  theta^ is tests/topicdocs_host.theta_hat of the stored rows,
so on the device's own rows it is the device's bit for bit.  On it, in np.longdouble: the logits, the
loss, the rows r, the gradient, F and its gradient; a full-Hessian Newton solver for small K C; the
predictions with a near-tie report; a brute-force k-nearest-neighbour vote; and the first-order rounding
bounds the GPU tests hold the device to.

The model.  z_dc = sum_k theta^_dk W_ck, l_d = log sum_c exp(z_dc) - z_{d,y_d}, p_d = softmax(z_d),
r_dc = w_d (p_dc - [c = y_d]); loss_sum = sum_d w_d l_d and grad_sum = R^T Theta^ over the documents with
y_d >= 0, Omega = sum_d w_d over them, F = loss_sum / Omega + (l2 / 2) |W|_F^2."""
import numpy as np

import effects_host as eh
import topicdocs_host as th

LD = np.longdouble
U = 2.0 ** -53
TINY = 2.0 ** -1022
ULP_EXP = 1                                    # device exp, in ulps (DESIGN.md 3.35 says where it is from)
ULP_LOG = 1                                    # device log, in ulps
theta_hat = th.theta_hat


def _weights(weights, labels):
    """w_d in longdouble with the left-out documents' weights set to zero."""
    labels = np.asarray(labels)
    w = np.ones(len(labels), dtype=LD) if weights is None else np.asarray(weights, dtype=np.float64).astype(LD)
    return np.where(labels >= 0, w, LD(0))


def forward(theta, W, labels=None, weights=None):
    """In longdouble: a dict of z (N x C), m (N), t = z - m, e = exp(t), S, p, and with labels l (N; 0
    for a left-out document), r (N x C) and w (N; 0 for a left-out document)."""
    t_ = np.asarray(theta, dtype=np.float64).astype(LD)
    w_ = np.asarray(W, dtype=np.float64).astype(LD)
    z = t_.dot(w_.T)
    m = z.max(axis=1)
    t = z - m[:, None]
    e = np.exp(t)
    S = e.sum(axis=1)
    out = {"z": z, "m": m, "t": t, "e": e, "S": S, "p": e / S[:, None]}
    if labels is not None:
        labels = np.asarray(labels)
        w = _weights(weights, labels)
        y = np.maximum(labels, 0)
        rows = np.arange(len(labels))
        l = np.where(labels >= 0, (np.log(S) + m) - z[rows, y], LD(0))
        hot = np.zeros(z.shape, dtype=LD)
        hot[rows[labels >= 0], labels[labels >= 0]] = 1
        out.update(l=l, w=w, r=w[:, None] * (out["p"] - hot))
    return out


def loss_grad(theta, W, labels, weights=None):
    """(loss_sum, grad_sum C x K, Omega) in longdouble."""
    f = forward(theta, W, labels, weights)
    t_ = np.asarray(theta, dtype=np.float64).astype(LD)
    return (f["w"] * f["l"]).sum(), f["r"].T.dot(t_), f["w"].sum()


def objective(theta, W, labels, weights, l2):
    """(F, grad F) in longdouble at the float64 or longdouble coefficients W."""
    Wl = np.asarray(W).astype(LD)
    t_ = np.asarray(theta, dtype=np.float64).astype(LD)
    labels = np.asarray(labels)
    w = _weights(weights, labels)
    z = t_.dot(Wl.T)
    m = z.max(axis=1)
    e = np.exp(z - m[:, None])
    S = e.sum(axis=1)
    y = np.maximum(labels, 0)
    rows = np.arange(len(labels))
    l = (np.log(S) + m) - z[rows, y]
    hot = np.zeros(z.shape, dtype=LD)
    hot[rows[labels >= 0], labels[labels >= 0]] = 1
    r = w[:, None] * (e / S[:, None] - hot)
    omega = w.sum()
    return (w * l).sum() / omega + LD(l2) / 2 * (Wl * Wl).sum(), r.T.dot(t_) / omega + LD(l2) * Wl


def fun64(theta, labels, weights, l2):
    """fun(W) -> (F, grad) in float64 NumPy: what drives the package's optimiser on the CPU."""
    t = np.asarray(theta, dtype=np.float64)
    labels = np.asarray(labels)
    w = np.where(labels >= 0, 1.0 if weights is None else np.asarray(weights, dtype=np.float64), 0.0)
    rows = np.arange(len(labels))
    keep = labels >= 0
    omega = w.sum()

    def fun(W):
        z = t.dot(W.T)
        m = z.max(axis=1)
        e = np.exp(z - m[:, None])
        S = e.sum(axis=1)
        l = (np.log(S) + m) - z[rows, np.maximum(labels, 0)]
        r = e / S[:, None]
        r[rows[keep], labels[keep]] -= 1.0
        r *= w[:, None]
        return float((w * l).sum() / omega + 0.5 * l2 * (W * W).sum()), r.T.dot(t) / omega + l2 * W
    return fun


def hessian(theta, W, labels, weights, l2):
    """The Hessian of F at W, float64, (C K) x (C K) in the order of W.ravel()."""
    t = np.asarray(theta, dtype=np.float64)
    labels = np.asarray(labels)
    w = np.asarray(_weights(weights, labels), dtype=np.float64)
    p = np.asarray(forward(theta, W)["p"], dtype=np.float64)
    C, K = np.asarray(W).shape
    a = w / w.sum()
    H = np.zeros((C, K, C, K))
    for c in range(C):
        for c2 in range(c, C):
            s = a * ((p[:, c] if c == c2 else 0.0) - p[:, c] * p[:, c2])
            block = (t * s[:, None]).T.dot(t)
            H[c, :, c2, :] = block
            H[c2, :, c, :] = block
    H = H.reshape(C * K, C * K)
    return H + l2 * np.eye(C * K)


def newton(theta, labels, weights, l2, C, W0=None, goal=1e-13, max_iter=60):
    """The optimum of F by Newton's method with the full Hessian: the steps are solved in float64, the
    iterate and the gradient are longdouble, and a step that does not lower |grad F|_F is halved.  Returns
    (W longdouble C x K, |grad F|_F), the latter below `goal` or an AssertionError."""
    K = np.asarray(theta).shape[1]
    W = np.zeros((C, K), dtype=LD) if W0 is None else np.asarray(W0).astype(LD)
    _, g = objective(theta, W, labels, weights, l2)
    norm = float(np.sqrt((g * g).sum()))
    for _ in range(max_iter):
        if norm < goal:
            break
        H = hessian(theta, np.asarray(W, dtype=np.float64), labels, weights, l2)
        step = np.linalg.solve(H, np.asarray(g, dtype=np.float64).ravel()).reshape(C, K).astype(LD)
        t = LD(1)
        for _ in range(30):
            Wn = W - t * step
            _, gn = objective(theta, Wn, labels, weights, l2)
            nn = float(np.sqrt((gn * gn).sum()))
            if nn < norm:
                break
            t = t / 2
        W, g, norm = Wn, gn, nn
    assert norm < goal, norm
    return W, norm


# -- predictions ---------------------------------------------------------------------------------------------
def predict(theta, W):
    """(labels int32 N, p longdouble N x C, near): the first class of largest longdouble logit, and the
    near-tie report -- the documents whose two largest logits are closer than twice their logit bound,
    for which the device may rightly answer otherwise."""
    f = forward(theta, W)
    z = f["z"]
    N, C = z.shape
    classes = np.arange(C)
    labels = np.empty(N, dtype=np.int32)
    gap = np.empty(N, dtype=LD)
    for d in range(N):
        order = np.lexsort((classes, -z[d]))
        labels[d] = order[0]
        gap[d] = z[d, order[0]] - z[d, order[1]]
    near = np.flatnonzero(gap < 2 * logit_bound(theta, W).max(axis=1))
    return labels, f["p"], near


def knn_predict(nearest, sim, labels, C, weighting="uniform"):
    """Brute force: per document its neighbours in rank order, one vote after the other in float64."""
    nearest = np.asarray(nearest)
    M, T = nearest.shape
    votes = np.zeros((M, C))
    pred = np.full(M, -1, dtype=np.int32)
    for i in range(M):
        voted = False
        for j in range(T):
            nb = int(nearest[i, j])
            if nb < 0 or labels[nb] < 0:
                continue
            votes[i, labels[nb]] = votes[i, labels[nb]] + (float(sim[i, j]) if weighting == "similarity" else 1.0)
            voted = True
        if voted:
            best = 0
            for c in range(1, C):
                if votes[i, c] > votes[i, best]:
                    best = c
            pred[i] = best
    return pred, votes


# -- the bounds, first order in u = 2^-53 ----------------------------------------------------------------------
def logit_bound(theta, W):
    """|z_dev - z| (N x C).  A logit is a chain of Kp / 4 matrix instructions from +0, each adding four
    products to the running value; however the four are grouped, a sum of Kp products errs by at most
    (Kp + 4) u sum_k |theta^_dk W_ck| -- the form effects_host.rss_bound uses for its fit (the 4: the
    zero tail and the grouping by four)."""
    t = np.abs(np.asarray(theta, dtype=np.float64))
    w = np.abs(np.asarray(W, dtype=np.float64))
    Kp = -(-t.shape[1] // 4) * 4
    return (Kp + 4) * U * t.dot(w.T)


def _softmax_bounds(theta, W):
    """(f, ez N, rel_e N x C, rel_S N): the relative errors of e_c and of S.

    l and p do not change when another number m' stands for m, so the device's m -- one of its own
    logits -- carries no error of its own.  t_c = z_c - m: |dt_c| <= ez + u |t_c| with ez the document's
    largest logit bound.  e_c = exp(t_c) at ULP_EXP ulps (2 u each): |de_c| / e_c <= |dt_c| + 2 u ULP_EXP
    (+ TINY absolute, where e_c underflows).  S adds C terms one after the other: |dS| / S <= (C - 1) u +
    sum_c |de_c| / S."""
    f = forward(theta, W)
    C = f["z"].shape[1]
    ez = logit_bound(theta, W).max(axis=1)
    t = np.asarray(np.abs(f["t"]), dtype=np.float64)
    e = np.asarray(f["e"], dtype=np.float64)
    S = np.asarray(f["S"], dtype=np.float64)
    rel_e = ez[:, None] + U * t + 2 * U * ULP_EXP
    rel_S = (C - 1) * U + (e * rel_e).sum(axis=1) / S + C * TINY
    return f, ez, rel_e, rel_S


def loss_bound(theta, W, labels, weights=None):
    """|loss_sum_dev - loss_sum|.  Per document l = (log S + m) - z_y: log at ULP_LOG ulps on an argument
    of relative error rel_S, two more roundings, and the error ez of z_y:
        |dl| <= rel_S + 2 u ULP_LOG |log S| + u |log S + m| + u |l| + ez.
    The term w l rounds once more, and the N terms are added in some order: with the allowance of 16 for
    the longdouble side, sum_d w_d |dl_d| + (N + 16) u sum_d w_d l_d."""
    f, ez, _, rel_S = _softmax_bounds(theta, W)
    labels = np.asarray(labels)
    w = np.asarray(_weights(weights, labels), dtype=np.float64)
    S = np.asarray(f["S"], dtype=np.float64)
    m = np.asarray(f["m"], dtype=np.float64)
    l = np.asarray(forward(theta, W, labels, weights)["l"], dtype=np.float64)
    dl = rel_S + 2 * U * ULP_LOG * np.abs(np.log(S)) + U * np.abs(np.log(S) + m) + U * np.abs(l) + ez
    N = len(labels)
    return float((w * dl).sum() + (N + 16) * U * (w * np.abs(l)).sum())


def proba_bound(theta, W):
    """|p_dev - p| (N x C): p_c = e_c / S, one division: p_c (rel_e_c + rel_S + u)."""
    f, _, rel_e, rel_S = _softmax_bounds(theta, W)
    return np.asarray(f["p"], dtype=np.float64) * (rel_e + rel_S[:, None] + U) + TINY


def r_bound(theta, W, labels, weights=None):
    """|r_dev - r| (N x C): r = w (p - [c = y]), a subtraction and a multiply on top of p's error:
    w (|dp| + 2 u |p - [c = y]|).  Exact zeros for a left-out document."""
    labels = np.asarray(labels)
    w = np.asarray(_weights(weights, labels), dtype=np.float64)
    r = np.asarray(forward(theta, W, labels, weights)["r"], dtype=np.float64)
    return w[:, None] * proba_bound(theta, W) + 2 * U * np.abs(r)


def grad_bound(theta, W, labels, weights=None):
    """|grad_sum_dev - grad_sum| (C x K): the cross product of the device's own r with theta^ within
    effects_host.products_bound of |R|^T |Theta^|, plus what the error of r itself carries over,
    sum_d |dr_dc| theta^_dk."""
    t = np.asarray(theta, dtype=np.float64)
    r = np.asarray(forward(theta, W, labels, weights)["r"], dtype=np.float64)
    carried = r_bound(theta, W, labels, weights).T.dot(np.abs(t))
    return eh.products_bound(np.abs(r).T.dot(np.abs(t)), t.shape[0]) + carried
