"""Shared by tests/test_similar_reference.py and tests/test_gpu_similar_items.py: the definition of cdae_hip_similar_items
(include/cdae_hip.h) in numpy.

Query q's list is the first topk items of C_q = allow \\ excl_q (\\ {q} when exclude_self) in cdae_hip_recommend_all's total order:
descending score, equal scores by ascending ORIGINAL item id; surplus places hold SENTINEL / -inf.  DOT: s(q, i) = T[i] . T[q];
COSINE: s(q, i) = N[i] . N[q] with N = normalise(T), the one order the header states.  The dot products here are fp64 matrix products:
they are the library's fp32 bits only for tables on which every fp32 dot product is exact in any order, which assert_exact_products
checks on the inputs; float tables are compared library against library (COSINE on T == DOT on a handle loaded with normalise(T))."""
import numpy as np

from filtered_ref import filtered_topk


def row_stride(K):
    """cdae_hip_row_stride(): the smallest of 64, 128, 256, 512 floats that holds num_dim"""
    return next(s for s in (64, 128, 256, 512) if K <= s)


def sum_of_squares(T):
    """ss_i in fp64, in the stated order: lane l of 64 owns elements [l NI, (l + 1) NI) of the zero-padded row and adds its squares in
    ascending order; the 64 partials are added as the balanced tree over neighbouring lanes (six pairwise halvings)."""
    T = np.ascontiguousarray(T, dtype=np.float32)
    n, K = T.shape
    NI = row_stride(K) // 64
    P = np.zeros((n, 64 * NI), dtype=np.float64)
    P[:, :K] = T
    P = P.reshape(n, 64, NI)
    p = np.zeros((n, 64), dtype=np.float64)
    for i in range(NI):                                  # sequential over the lane's elements
        p = p + P[:, :, i] * P[:, :, i]
    for _ in range(6):                                   # (p_0 + p_1), (p_2 + p_3), ... then pairs of those
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


def normalise(T):
    """N [n, K] float32: N[i] = T[i] / (float32)sqrt(ss_i), a float32 division; a row with ss_i == 0 becomes +0.0 everywhere"""
    T = np.ascontiguousarray(T, dtype=np.float32)
    ss = sum_of_squares(T)
    norm = np.sqrt(ss).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        N = (T / norm[:, None]).astype(np.float32)
    assert N.dtype == np.float32
    N[ss == 0] = 0.0
    return N


def operand(T, metric):
    if metric not in ("dot", "cosine"):
        raise ValueError(metric)
    T = np.ascontiguousarray(T, dtype=np.float32)
    return normalise(T) if metric == "cosine" else T


def assert_exact_products(M, unit, queries=None):
    """The condition on the INPUTS under which every fp32 dot product of a query row (None: any row) and a row of M is exact in any
    summation order, fused or not: every element is a multiple of `unit` (a power of two), so every product and partial sum is a
    multiple of unit^2, and max_{q, i} sum_k |M_qk M_ik| < 2^24 unit^2, so no partial sum needs more than 24 bits."""
    assert unit > 0 and np.log2(unit) == int(np.log2(unit)), unit
    Q = np.asarray(M, dtype=np.float64) / unit
    assert np.array_equal(Q, np.rint(Q)), "an element is not a multiple of the unit"
    A = np.abs(Q)
    worst = ((A if queries is None else A[np.asarray(queries, dtype=np.int64)]) @ A.T).max(initial=0)
    assert worst < 2 ** 24, worst


def scores(T, queries, metric):
    """S [n_queries, I] float64: s(q, i) for every item; + 0.0 last, as the library adds its bias (a -0.0 becomes +0.0)"""
    M = operand(T, metric).astype(np.float64)
    return M[np.asarray(queries, dtype=np.int64)] @ M.T + 0.0


def lists_of(S, queries, exclude_self, excl, allow, topk):
    """the lists from the scores S [n_queries, I] of every (query, item)"""
    own = [np.array([q], dtype=np.int64) for q in np.asarray(queries, dtype=np.int64).reshape(-1)]      # the "rated" row of query q is {q}
    return filtered_topk(S, own, excl, allow, bool(exclude_self), topk)


def similar_topk(T, queries, metric="cosine", exclude_self=True, excl=None, allow=None, topk=10):
    """T [I, K]; queries: item ids; excl: one item array per query, or None; allow: one ascending item array, or None
    -> (ids uint32 [n_queries, topk], scores float32 [n_queries, topk])"""
    return lists_of(scores(T, queries, metric), queries, exclude_self, excl, allow, topk)
