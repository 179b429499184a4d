"""NumPy restatement of the document groups of a document index (csrc/cluster_kernels.h, DESIGN.md
3.26): spherical k-means on the stored rows (tests/docindex_host.py), which are of unit length,

    assignment:  s(n, c) = sum_k x_nk m_ck, the np.longdouble dot of the rows; label(n) the first c in
                 the total order (s descending, c ascending); the margin s_best - s_second says how
                 far the label is from a different answer
    update:      m_c = S_c / |S_c| with S_c the sum of the rows labelled c, in np.longdouble; a cluster
                 without members keeps its row
    loop:        assign; if this is not the first assignment and no label changed, stop (converged);
                 otherwise, if fewer than max_iter updates have run, update and assign again

and theta^ of a centroid row as tests/topicdocs_host.py recovers it from a stored row, in longdouble:
m * m (hellinger) or m / sum(m) (cosine)."""
import numpy as np

import docindex_host as dh

LD = np.longdouble


def assign(xrows, mrows):
    """(labels int32 N, s_best longdouble N, margin float64 N) of the rows N x K under the centroid
    rows C x K; the margin of a single centroid is inf."""
    x = np.asarray(xrows).astype(LD)
    m = np.asarray(mrows).astype(LD)
    s = x.dot(m.T)
    N, C = s.shape
    order = np.lexsort((np.broadcast_to(np.arange(C), (N, C)), -s), axis=1)
    ranked = np.take_along_axis(s, order, axis=1)
    margin = (ranked[:, 0] - ranked[:, 1]).astype(np.float64) if C > 1 else np.full(N, np.inf)
    return order[:, 0].astype(np.int32), ranked[:, 0], margin


def update(xrows, mrows, labels):
    """The centroid rows C x K (longdouble) of the labelled rows; empty clusters keep theirs."""
    x = np.asarray(xrows).astype(LD)
    out = np.array(mrows, dtype=LD, copy=True)
    for c in range(out.shape[0]):
        members = x[labels == c]
        if len(members):
            S = members.sum(axis=0)
            out[c] = S / np.sqrt((S * S).sum())
    return out


def theta_hat(mrows, measure):
    """Centroid rows C x K -> topic proportions K x C (longdouble)."""
    m = np.asarray(mrows).astype(LD)
    if measure == "hellinger":
        return (m * m).T
    if measure == "cosine":
        return (m / m.sum(axis=1)[:, None]).T
    raise ValueError(measure)


class Run(object):
    """What the loop went through: after assignment j (j updates have run) labels[j], similarity[j]
    (longdouble, N), objective[j] = sum(1 - similarity[j]) and the centroid rows[j] it was made under;
    iterations, converged, and the smallest margin of all assignments."""

    def __init__(self):
        self.labels, self.similarity, self.objective, self.rows = [], [], [], []
        self.iterations, self.converged, self.margin = 0, False, np.inf

    def after(self, max_iter):
        """(j, iterations, converged) of the same loop stopped at max_iter updates: its results are
        those of assignment j."""
        j = min(max_iter, self.iterations)
        return j, j, bool(self.converged and max_iter >= self.iterations)

    def sizes(self, j):
        return np.bincount(self.labels[j], minlength=self.rows[j].shape[0]).astype(np.int64)


def run(xrows, mrows, max_iter=50):
    """The loop on the rows N x K from the centroid rows C x K."""
    out = Run()
    m = np.asarray(mrows).astype(LD)

    def step():
        labels, s, margin = assign(xrows, m)
        out.labels.append(labels)
        out.similarity.append(s)
        out.objective.append((LD(1) - s).sum())
        out.rows.append(m)
        out.margin = min(out.margin, float(margin.min()))

    step()
    while out.iterations < max_iter:
        m = update(xrows, m, out.labels[-1])
        out.iterations += 1
        step()
        if np.array_equal(out.labels[-1], out.labels[-2]):
            out.converged = True
            break
    return out


def run_gamma(gamma, centroids, measure, max_iter=50):
    """The same from gamma (K x N) and the centroids' topic proportions (K x C)."""
    return run(dh.rows(gamma, measure), dh.rows(centroids, measure), max_iter)
