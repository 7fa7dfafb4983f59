"""Shared by tests/test_filtered_reference.py and tests/test_gpu_rows_filtered.py: the definition of cdae_hip_recommend_rows_filtered
(include/cdae_hip.h) in numpy, and the caller-side pieces of such a call.

Row r's list is the first topk items of its candidate set C_r = allow \\ excl_r (\\ rated_r when exclude_rated) in
cdae_hip_recommend_all's total order: descending score, equal scores by ascending ORIGINAL item id; the surplus places of a row with
|C_r| < topk hold SENTINEL, and -inf as their score.  Neither excl nor allow changes a score."""
import numpy as np

from helpers import SENTINEL


def csr(rows):
    return np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64), (np.concatenate(rows) if len(rows) else np.empty(0)).astype(np.uint32)


def rows_of(ptr, col):
    return [col[ptr[r]:ptr[r + 1]] for r in range(ptr.size - 1)]


def candidate_mask(I, rated_r, excl_r, allow, exclude_rated):
    """bool [I]: the items of C_r"""
    keep = np.ones(I, dtype=bool) if allow is None else np.zeros(I, dtype=bool)
    if allow is not None:
        keep[np.asarray(allow, dtype=np.int64)] = True
    if excl_r is not None:
        keep[np.asarray(excl_r, dtype=np.int64)] = False
    if exclude_rated:
        keep[np.asarray(rated_r, dtype=np.int64)] = False
    return keep


def filtered_topk(S, rated, excl, allow, exclude_rated, topk):
    """S [R, I]: the score of every (row, item), any real dtype; rated: one item array per row; excl: one item array per row, or
    None; allow: one ascending item array for all rows, or None -> (ids uint32 [R, topk], scores float32 [R, topk])."""
    S = np.asarray(S)
    R, I = S.shape
    ids = np.full((R, topk), SENTINEL, dtype=np.uint32)
    sc = np.full((R, topk), -np.inf, dtype=np.float32)
    all_ids = np.arange(I, dtype=np.int64)
    for r in range(R):
        keep = candidate_mask(I, rated[r], None if excl is None else excl[r], allow, exclude_rated)
        c, s = all_ids[keep], S[r][keep]
        if c.size > 4 * topk:                            # only the candidates at or above the topk-th best score can appear
            thr = np.partition(s, c.size - topk)[c.size - topk]
            sel = s >= thr
            c, s = c[sel], s[sel]
        order = np.lexsort((c, -s.astype(np.float64)))[:topk]       # (the scores handed in are exact in fp64: integers, or fp32 values)
        ids[r, :order.size] = c[order]
        sc[r, :order.size] = s[order]
    return ids, sc


def delete_outside(ids, scores, keep_masks, topk):
    """The deletion property: from each row's whole list (ids, scores; SENTINEL places ignored) delete the items outside the row's
    candidate mask and cut at topk -> (ids, scores) padded like filtered_topk's."""
    R = ids.shape[0]
    out = np.full((R, topk), SENTINEL, dtype=np.uint32)
    sc = np.full((R, topk), -np.inf, dtype=np.float32)
    for r in range(R):
        real = ids[r] != SENTINEL
        i, s = ids[r][real], scores[r][real]
        sel = keep_masks[r][i.astype(np.int64)]
        i, s = i[sel][:topk], s[sel][:topk]
        out[r, :i.size] = i
        sc[r, :i.size] = s
    return out, sc
