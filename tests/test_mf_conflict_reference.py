"""CPU: the inputs of tests/test_gpu_mf_tiers.py reach what they are meant to reach (tests/mf_conflict_ref.py).

The in-place loop of mf_user_kernel re-reads an instance's rows when one of the 8 instances before it, in the same 64-instance chunk of
the user, stepped one of them.  The 12-item data set of test_gpu_mf.py never gives a user a second chunk; D40 (40 items, rows of up
to 35) does, and its repeats cover every distance inside the window, at its edge and just beyond it.
"""
import numpy as np
import pytest

import mf_conflict_ref as cr


def test_d40_is_what_the_tests_say_it_is(built):
    d = cr.d40()
    assert d.num_users == 8 and d.num_items == 40
    assert tuple(np.diff(d.train_ptr)) == cr.D40_LENGTHS
    for u in range(d.num_users):
        row = d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]
        assert (np.diff(row.astype(np.int64)) > 0).all() and row.max() < 40


def test_instance_lists_follow_the_loop_order():
    row = np.array([3, 7], dtype=np.uint32)
    neg = np.array([[1, 2], [2, 1]], dtype=np.uint32)
    assert cr.user_instances(row, neg, False) == [(3,), (1,), (2,), (7,), (2,), (1,)]
    assert cr.user_instances(row, neg, True) == [(3, 1), (3, 2), (7, 2), (7, 1)]
    assert cr.repeats(cr.user_instances(row, neg, False)) == [(2, 4), (1, 5)]
    assert cr.repeats(cr.user_instances(row, neg, True)) == [(0, 1), (1, 2), (2, 3), (0, 3)]


def test_negatives_are_never_the_users_positives(built):
    d = cr.d40()
    o = cr.draw_oracle(d, 5)
    for u in range(d.num_users):
        row = d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]
        neg = cr.user_negatives(o, d, 5, 0, u)
        assert neg.shape == (row.size, 5) and neg.max() < 40
        assert not np.intersect1d(neg.ravel(), row).size


@pytest.mark.parametrize("pairwise,num_neg", cr.D40_SETTINGS, ids=lambda v: str(v))
def test_d40_reaches_the_conflict_window_and_a_chunk_boundary(built, pairwise, num_neg):
    """seed 5, epoch 0: every distance 1 .. 10 between two consecutive steps of a row occurs, and a repeat inside the window has its two
    instances in different chunks (19, 24 and 58 of them for IMF num_neg 5, BPR num_neg 5, BPR num_neg 12)."""
    count, straddle = cr.assert_reaches_the_window(cr.d40(), pairwise, num_neg, 5, 0)
    print(f"\nD40 pairwise={pairwise} num_neg={num_neg}: repeats by distance {[count.get(k, 0) for k in range(1, 11)]}, "
          f"{straddle} straddle a chunk boundary")
    if not pairwise:
        assert min(count[k] for k in range(1, 11)) >= 16


@pytest.mark.parametrize("pairwise", [False, True])
def test_the_12_item_set_never_reaches_a_second_chunk(built, pairwise):
    """the gap D40 closes: rows of at most 9 items give at most 54 instances (45 pairs) per user — no chunk boundary, no straddle"""
    for epoch in range(3):
        _, straddle, longest = cr.conflict_profile(cr.d12(), pairwise, 5, 5, epoch)
        assert straddle == 0 and longest <= cr.CHUNK
