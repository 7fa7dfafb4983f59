"""Full-catalogue ranking metrics from exact ranks (numpy only, no GPU).

CDAE.full_rank_rows returns, for every held-out target of a row, its place in the row's whole list: the number of unrated items
that precede it.  Everything a top-N evaluation reports follows from those integers; nothing here looks at a score.

Conventions (the reference's, evaluation.hpp:183-219, extended to any k): every metric is the mean over the rows WITH targets;
recall@k divides the hits in the first k places by the number of targets (:203-209), map@k divides the sum of the precisions at the
hits by min(k, targets)."""
from __future__ import annotations

import numpy as np

DEFAULT_KS = (1, 5, 10, 20, 50, 100)


def ranking_metrics(target_ptr, ranks, n_unrated, ks=DEFAULT_KS) -> dict:
    """target_ptr [n_rows + 1]: the CSR row pointer of the target sets; ranks [nnz_targets]: rank of every target among its row's
    unrated items, 0 the head of the list (distinct inside a row); n_unrated [n_rows] (or a scalar): num_items - len(rated row).
    -> {"recall@k", "precision@k", "ndcg@k", "map@k" for every k of ks, "mrr", "auc", "rows"}:
      precision@k  hits in the first k places / k
      recall@k     hits in the first k places / targets
      ndcg@k       binary gains: sum over the hits of 1 / log2(rank + 2), over the same sum for min(k, targets) hits at the head
      map@k        sum over the hits of (hits so far / (rank + 1)), over min(k, targets)
      mrr          1 / (best rank + 1)
      auc          the share of (target, unrated non-target) pairs in which the target comes first; a row whose targets are all of
                   its unrated items has no such pair and counts as 1
      rows         the number of rows with targets (what every mean is taken over)."""
    ptr = np.asarray(target_ptr, dtype=np.int64)
    r = np.asarray(ranks).astype(np.int64)
    n_rows = ptr.size - 1
    if ptr.ndim != 1 or n_rows < 0 or ptr[0] != 0 or r.shape != (int(ptr[-1]),):
        raise ValueError("target_ptr / ranks are not a CSR and one rank per target")
    nt_all = np.diff(ptr)
    unrated = np.broadcast_to(np.asarray(n_unrated, dtype=np.int64), (n_rows,))
    if (nt_all < 0).any() or (unrated < nt_all).any() or (r < 0).any():
        raise ValueError("more targets than unrated items, or a negative rank")
    row = np.repeat(np.arange(n_rows), nt_all)
    if (r >= unrated[row]).any():
        raise ValueError("a rank beyond the row's unrated items")
    with_t = nt_all > 0
    n = int(with_t.sum())
    ks = tuple(int(k) for k in ks)
    if any(k < 1 for k in ks):
        raise ValueError("k must be at least 1")
    out = {"rows": n}
    if n == 0:
        raise ValueError("no row has targets")
    order = np.lexsort((r, row))                       # by row, then by rank
    r, row = r[order], row[order]
    if ((np.diff(r) == 0) & (np.diff(row) == 0)).any():
        raise ValueError("two targets of a row share a rank")
    nt = nt_all[with_t].astype(np.float64)
    idx = np.arange(r.size) - ptr[row]                 # targets of the row that come before this one
    gain = 1.0 / np.log2(r + 2.0)
    prec_at_hit = (idx + 1.0) / (r + 1.0)
    ideal = np.r_[0.0, np.cumsum(1.0 / np.log2(np.arange(max(ks)) + 2.0))]

    def mean(per_row):                                 # the reference's loop: each row's term divided by the row count, then added
        return float((per_row / n).sum())

    def per_row(weights):
        return np.bincount(row, weights=weights, minlength=n_rows)[with_t]
    for k in ks:
        hit = (r < k).astype(np.float64)
        hits = per_row(hit)
        top = np.minimum(nt, k)
        out[f"precision@{k}"] = mean(hits / k)
        out[f"recall@{k}"] = mean(hits / nt)
        out[f"ndcg@{k}"] = mean(per_row(hit * gain) / ideal[top.astype(np.int64)])
        out[f"map@{k}"] = mean(per_row(hit * prec_at_hit) / top)
    best = r[ptr[:-1][with_t]]                         # the first of every row after the sort
    out["mrr"] = mean(1.0 / (best + 1.0))
    neg = (unrated[with_t] - nt_all[with_t]).astype(np.float64)
    ahead = per_row((r - idx).astype(np.float64))      # non-targets in front of each target, summed over the row's targets
    pairs = nt * neg
    out["auc"] = mean(np.where(pairs > 0, 1.0 - ahead / np.maximum(pairs, 1.0), 1.0))
    return out
