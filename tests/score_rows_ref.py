"""Numpy expected values for CDAE.score_rows (cdae_hip_score_rows): not a test, the yardstick of tests/test_gpu_score_rows.py,
itself checked against the fp64 oracle by tests/test_score_rows_reference.py."""
import numpy as np


def row_of_position(cand_ptr):
    """row index of every position of a CSR"""
    cand_ptr = np.asarray(cand_ptr, dtype=np.int64)
    return np.repeat(np.arange(cand_ptr.size - 1, dtype=np.int64), np.diff(cand_ptr))


def scores64(z, D, bp, cand_ptr, cand_col):
    """fp64 D[cand_col[p]] . z_r + b'[cand_col[p]] for every position p of the candidate CSR (r: the row p belongs to)"""
    z, D, bp = (np.asarray(a, dtype=np.float64) for a in (z, D, bp))
    r, j = row_of_position(cand_ptr), np.asarray(cand_col, dtype=np.int64)
    K = min(z.shape[1], D.shape[1])
    return np.einsum("pk,pk->p", z[r, :K], D[j, :K]) + bp[j]


def magnitudes64(z, D, bp, cand_ptr, cand_col):
    """sum_k |z_k D_jk| + |b'_j| per position: what the fp32 error bound of one score scales with"""
    return scores64(np.abs(np.asarray(z, dtype=np.float64)), np.abs(np.asarray(D, dtype=np.float64)), np.abs(np.asarray(bp, dtype=np.float64)),
                    cand_ptr, cand_col)


def ranks_of(scores, cand_ptr, cand_col):
    """per row the place of every candidate in cdae_hip_recommend_all's total order (descending score, equal scores by ascending
    item id), 0 the best: uint32 per position"""
    scores, ids = np.asarray(scores), np.asarray(cand_col, dtype=np.int64)
    cand_ptr = np.asarray(cand_ptr, dtype=np.int64)
    out = np.empty(ids.size, dtype=np.uint32)
    for a, b in zip(cand_ptr[:-1], cand_ptr[1:]):
        order = np.lexsort((ids[a:b], -scores[a:b]))
        out[a:b][order] = np.arange(b - a, dtype=np.uint32)
    return out
