"""Shared by tests/test_gpu_full_rank.py: the caller-side pieces of a cdae_hip_full_rank_rows call (rated rows, user ids, target
rows that cross the 16-target window) and the expected ranks in integer arithmetic — the position of every target in
helpers.rank_total_order(S, ..., topk = num_items), the documented total order of include/cdae_hip.h."""
import numpy as np

from helpers import SENTINEL, assert_fp32_exact, exact_scores, rank_total_order

NO_USER = 0xFFFFFFFF
TARGET_SIZES = (0, 1, 3, 16, 17, 40)     # per row, in turn: the window of 16 is met exactly and crossed


def csr(rows):
    return np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64), (np.concatenate(rows) if rows else np.empty(0)).astype(np.uint32)


def rows_of(ptr, col):
    return [col[ptr[r]:ptr[r + 1]] for r in range(ptr.size - 1)]


def draw_uids(rng, U, R):
    """users with repeats, a fifth of the rows without a user node"""
    uids = rng.integers(0, U, R).astype(np.uint32)
    uids[rng.random(R) < 0.2] = NO_USER
    return uids


def gathered(M, uids, fill):
    """M[uids], rows of `fill` where the row has no user node"""
    out = np.full((len(uids), M.shape[1]), fill, dtype=M.dtype)
    real = np.asarray(uids) != NO_USER
    out[real] = M[np.asarray(uids)[real].astype(np.int64)]
    return out


def draw_targets(rng, rated_rows, I, all_of=()):
    """Target rows of TARGET_SIZES items in turn (fewer where the row leaves fewer), none of them rated: items 0 and I - 1 wherever
    they are unrated, a few of the lowest and of the highest 40 ids (the `low` and `last` plateaus), the rest anywhere — both lane
    halves (item & 4) of the matrix-core kernel occur in every row of three or more.  all_of: rows whose targets are ALL of their
    unrated items."""
    out = []
    for r, rated in enumerate(rated_rows):
        free = np.setdiff1d(np.arange(I, dtype=np.uint32), rated)
        n = free.size if r in all_of else min(TARGET_SIZES[r % len(TARGET_SIZES)], free.size)
        edge = free[(free == 0) | (free == I - 1)]
        low, high = free[free < 40], free[free >= I - 40]
        pick = np.r_[edge, rng.permutation(low)[:n // 4], rng.permutation(high)[:n // 4], rng.permutation(free)]
        _, first = np.unique(pick, return_index=True)
        out.append(np.sort(pick[np.sort(first)][:n]).astype(np.uint32))
    return out


def positions(order, tptr, tcol, I):
    """rank of every target = its position in its row of `order` (rank_total_order with topk = I)"""
    ranks = np.empty(tcol.size, dtype=np.uint32)
    for r in range(tptr.size - 1):
        n = int((order[r] != SENTINEL).sum())
        pos = np.full(I, -1, dtype=np.int64)
        pos[order[r, :n]] = np.arange(n)
        mine = pos[tcol[tptr[r]:tptr[r + 1]]]
        assert (mine >= 0).all(), "a target is rated"
        ranks[tptr[r]:tptr[r + 1]] = mine
    return ranks


def expected_ranks(p, ptr, col, uids, tptr, tcol):
    """(ranks uint32, scores float32) for integer parameters p (test_gpu_rank_exact.int_model)"""
    R = ptr.size - 1
    u = np.full(R, NO_USER, dtype=np.uint32) if uids is None else uids
    Z, S, D, bq = exact_scores(ptr, col, **dict(p, Wu=gathered(p["Wu"], u, 0.0)))
    assert_fp32_exact(Z, D, bq)                      # a condition on the inputs, checked before the GPU is touched
    I = S.shape[1]
    order = rank_total_order(S, ptr, col, I)
    row = np.repeat(np.arange(R), np.diff(tptr))
    return positions(order, tptr, tcol, I), S[row, tcol.astype(np.int64)].astype(np.float32)
