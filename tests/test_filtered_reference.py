"""CPU: the numpy definition the GPU tests of cdae_hip_recommend_rows_filtered expect (tests/filtered_ref.py) against a brute-force
sort on a hand-sized case — ties, an empty candidate set, fewer candidates than topk — and, without a filter, against
helpers.rank_total_order, the yardstick of every other ranking test."""
import functools

import numpy as np

from filtered_ref import candidate_mask, csr, delete_outside, filtered_topk, rows_of
from helpers import SENTINEL, rank_total_order

I = 12
#                  0  1  2  3  4  5  6  7  8  9 10 11
S = np.array([[3, 1, 3, 0, 3, 2, 2, -1, 3, 0, 1, 2],
              [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
              [5, 4, 3, 2, 1, 0, -1, -2, -3, -4, -5, -6],
              [1, 1, 2, 2, 1, 1, 2, 2, 1, 1, 2, 2]], dtype=np.int64)
RATED = [np.array([0, 5], np.uint32), np.array([], np.uint32), np.array([0, 1, 2], np.uint32), np.array([2, 3, 11], np.uint32)]
EXCL = [np.array([2, 7], np.uint32), np.array([1, 3, 4, 8, 9], np.uint32), np.array([], np.uint32), np.array([3, 6, 10], np.uint32)]
ALLOW = np.array([1, 3, 4, 8, 9], np.uint32)


def brute(S, rated, excl, allow, exclude_rated, topk):
    """the definition, item by item: sort the candidates by the comparison the header states"""
    R = S.shape[0]
    ids = np.full((R, topk), SENTINEL, np.uint32)
    sc = np.full((R, topk), -np.inf, np.float32)
    for r in range(R):
        cand = [j for j in range(S.shape[1])
                if (allow is None or j in set(allow.tolist())) and (excl is None or j not in set(excl[r].tolist()))
                and not (exclude_rated and j in set(rated[r].tolist()))]

        def before(a, b):
            return -1 if (S[r, a] > S[r, b] or (S[r, a] == S[r, b] and a < b)) else 1
        cand.sort(key=functools.cmp_to_key(before))
        for place, j in enumerate(cand[:topk]):
            ids[r, place], sc[r, place] = j, S[r, j]
    return ids, sc


def test_the_reference_is_the_definition_on_a_small_case_with_ties():
    seen_short = seen_empty = False
    for allow in (None, ALLOW, np.array([7], np.uint32), np.arange(I, dtype=np.uint32)):
        for excl in (None, EXCL):
            for exclude_rated in (True, False):
                for topk in (1, 3, 5, 12):
                    got = filtered_topk(S, RATED, excl, allow, exclude_rated, topk)
                    want = brute(S, RATED, excl, allow, exclude_rated, topk)
                    np.testing.assert_array_equal(got[0], want[0])
                    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
                    assert got[0].dtype == np.uint32 and got[1].dtype == np.float32
                    n = (got[0] != SENTINEL).sum(axis=1)
                    seen_empty |= bool((n == 0).any())
                    seen_short |= bool(((n > 0) & (n < topk)).any())
                    assert np.isneginf(got[1][got[0] == SENTINEL]).all()
    assert seen_short and seen_empty
    # row 1 with ALLOW and EXCL: every allowed item is excluded; row 0, no filter: the four 3s by id without the rated 0
    ids, _ = filtered_topk(S, RATED, EXCL, ALLOW, True, 3)
    assert (ids[1] == SENTINEL).all()
    ids, sc = filtered_topk(S, RATED, None, None, True, 4)
    np.testing.assert_array_equal(ids[0], [2, 4, 8, 6])
    np.testing.assert_array_equal(sc[0], [3, 3, 3, 2])
    # a rated item comes back when the rated set is not excluded, and excl still removes it
    ids, _ = filtered_topk(S, RATED, None, None, False, 2)
    np.testing.assert_array_equal(ids[0], [0, 2])
    ids, _ = filtered_topk(S, RATED, [np.array([0], np.uint32)] * 4, None, False, 2)
    np.testing.assert_array_equal(ids[0], [2, 4])


def test_without_a_filter_the_reference_is_rank_total_order():
    rng = np.random.default_rng(2)
    R, items = 50, 203
    big = rng.integers(-3, 4, (R, items))
    rated = [np.sort(rng.choice(items, int(n), replace=False)).astype(np.uint32) for n in rng.integers(0, 60, R)]
    rated[3] = np.setdiff1d(np.arange(items), [4, 100, 202]).astype(np.uint32)
    ptr, col = csr(rated)
    for topk in (1, 10, 24):
        ids, sc = filtered_topk(big, rated, None, None, True, topk)
        np.testing.assert_array_equal(ids, rank_total_order(big, ptr, col, topk))
        # excl takes rank_total_order's deletion set: rated | excl
        excl = [np.sort(rng.choice(items, 20, replace=False)).astype(np.uint32) for _ in range(R)]
        ids2, _ = filtered_topk(big, rated, excl, None, True, topk)
        np.testing.assert_array_equal(ids2, rank_total_order(big, None, None, topk, rated=[np.union1d(a, b) for a, b in zip(rated, excl)]))
    assert [r.tolist() for r in rows_of(ptr, col)] == [r.tolist() for r in rated]


def test_deleting_from_the_whole_list_is_the_filtered_list():
    """delete_outside (what the GPU deletion tests do to recommend_rows' unbounded list) agrees with the definition"""
    whole, whole_sc = filtered_topk(S, RATED, None, None, True, I)
    for allow in (None, ALLOW):
        masks = [candidate_mask(I, RATED[r], EXCL[r], allow, True) for r in range(S.shape[0])]
        got = delete_outside(whole, whole_sc, masks, 3)
        want = filtered_topk(S, RATED, EXCL, allow, True, 3)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
