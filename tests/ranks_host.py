"""NumPy restatement of the held-out ranks (csrc/ranks_kernels.h): the scores are those
of tests/recommend_host.py (longdouble from the float64 gamma and lambda), a document's ranking is
``np.lexsort((ids, -s))`` over the words it has not seen, and a relevant word's rank is its position
in that ranking, plus one.  Relevant: the distinct words with a positive count in the held-out part
that the observed part has not seen (an entry (w, c) with c > 0; repeated entries count once).

Besides the ranks a near-tie report: per relevant word the smallest relative gap between its score
and any other candidate's, which tells how far the word's rank is from a different answer."""
import numpy as np

import recommend_host as rh


def ranks(gamma, lam, observed, heldout, s=None):
    """``observed``: (indptr, ids, cnts) of the seen words, or None (every word is a candidate);
    ``heldout``: (indptr, ids, cnts).  Returns ``(indptr int64, words int32, ranks int32, candidates
    int32, scores longdouble, gap float64)``, words per document in ascending id; ``gap`` is inf for a
    word that is its document's only candidate.  ``s``: rh.scores(gamma, lam) where the caller has it."""
    if s is None:
        s = rh.scores(gamma, lam)
    B, V = s.shape
    held = rh.seen(heldout[0], heldout[1], heldout[2], V)
    left_out = rh.seen(observed[0], observed[1], observed[2], V) if observed is not None else np.zeros((B, V), bool)
    ids = np.arange(V)
    indptr, words, out, scores, gap = [0], [], [], [], []
    for d in range(B):
        order = np.lexsort((ids, -s[d]))
        order = order[~left_out[d][order]]
        position = np.full(V, -1, dtype=np.int64)
        position[order] = np.arange(len(order))
        for h in np.flatnonzero(held[d] & ~left_out[d]):
            words.append(h)
            out.append(position[h] + 1)
            scores.append(s[d, h])
            others = order[order != h]
            gap.append(float(np.min(np.abs(s[d, others] - s[d, h]) / s[d, h])) if len(others) else np.inf)
        indptr.append(len(words))
    return (np.array(indptr, dtype=np.int64), np.array(words, dtype=np.int32), np.array(out, dtype=np.int32),
            (V - left_out.sum(axis=1)).astype(np.int32), np.array(scores, dtype=np.longdouble),
            np.array(gap, dtype=np.float64))


def metrics(indptr, ranks, candidates, top_n):
    """The figures of LDA.ranking_metrics by the definitions, one document at a time: each document's
    full ranked list is built as a 0 / 1 relevance vector of length n and scored naively.  Returns the
    dict of ``_ranking_metrics`` (None when no document has a relevant word)."""
    pct, auc, mrr, ap, ndcg = [], [], [], [], []
    recall = {n: [] for n in top_n}
    for d in range(len(indptr) - 1):
        r = ranks[indptr[d]:indptr[d + 1]]
        n = int(candidates[d])
        if len(r) == 0:
            continue
        rel = np.zeros(n, dtype=bool)
        rel[np.asarray(r) - 1] = True
        R = int(rel.sum())
        at = np.flatnonzero(rel)                                   # 0-based positions, ascending
        pct.extend((p / (n - 1) if n > 1 else 0.0) for p in at)
        if n > R:
            # the fraction of (relevant, other) pairs in which the relevant word comes first
            wins = sum(int((~rel[p + 1:]).sum()) for p in at)
            auc.append(wins / (R * (n - R)))
        mrr.append(1.0 / (at[0] + 1))
        ap.append(sum(rel[:p + 1].sum() / (p + 1) for p in at) / R)
        gain = rel / np.log2(np.arange(n) + 2.0)
        ndcg.append(gain.sum() / (1.0 / np.log2(np.arange(R) + 2.0)).sum())
        for top in top_n:
            recall[top].append(rel[:top].sum() / R)
    if not mrr:
        return None
    return {"mean_percentile_rank": float(np.mean(pct)), "auc": float(np.mean(auc)) if auc else float("nan"),
            "mrr": float(np.mean(mrr)), "map": float(np.mean(ap)), "ndcg": float(np.mean(ndcg)),
            "recall": {n: float(np.mean(v)) for n, v in recall.items()}}
