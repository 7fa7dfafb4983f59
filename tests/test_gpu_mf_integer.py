"""-m gpu: BIT-EXACT parity of the integer work of an IMF / BPR batch (tier bar: integer / index work is compared with
assert_array_equal, never through fp32 outcomes — tests/test_gpu_integer.py does this for the CDAE sampler).

cdae_hip_debug_sample_batch on an MF handle runs mf_sample_kernel and the batch sort as training would (the sequential schedule, which
reads the user-major list only, sorts for this call alone) and copies the lists back.  Expected values, from the kernel's own
comments (cdae_mf_kernels.hpp) — s the user's slot in the window, row ascending, neg[p][k] the oracle's draw p * num_neg + k:
  IMF  per user, per positive p: item row[p], then neg[p][0 .. num_neg); word = e << 32 | s, e the running example index of the window
  BPR  per user, per p, per k, pair q (running): example 2 q = (row[p], q << 32 | s), example 2 q + 1 = (neg[p][k], q << 32 | s | TARGET_BIT)
and the item-major list is numpy's stable argsort by item of that user-major list, with (0, 0) segments for items without examples.

Windows are in TRAINING POSITIONS: the oracle's draws are taken on the data set renumbered by MF.user_order().

NOT asserted: the two DUP flag bits of sorted_val (masked) and the correction-row numbers (dup_of_pos, dup_of_ex).  mf_user_kernel and
mf_item_kernel read neither, and for BPR dup_of_ex is indexed by pair, not by example.
"""
import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth
import mf_conflict_ref as cr
from test_gpu_mf import in_training_order, make

pytestmark = pytest.mark.gpu

DUP_PREV, DUP_NEXT, TARGET = 1 << 28, 1 << 29, 1 << 30
NO_DUP = np.uint64(0xFFFFFFFFFFFFFFFF & ~(DUP_PREV | DUP_NEXT))
MODELS = [pytest.param(False, id="imf"), pytest.param(True, id="bpr")]


def expected_examples(o, dp, seed, epoch, u0, nb, pairwise):
    """user-major (item, word) lists of the window [u0, u0 + nb) of positions"""
    num_neg = o.cfg.num_neg
    items, words, base = [], [], 0
    for s in range(nb):
        u = u0 + s
        row = dp.train_col[dp.train_ptr[u]:dp.train_ptr[u + 1]].astype(np.uint32)
        neg = cr.user_negatives(o, dp, seed, epoch, u)
        if pairwise:
            q = (np.uint64(base) + np.arange(row.size * num_neg, dtype=np.uint64)) << np.uint64(32)
            items.append(np.stack([np.repeat(row, num_neg), neg.ravel()], axis=1).ravel())
            words.append(np.stack([q | np.uint64(s), q | np.uint64(s | TARGET)], axis=1).ravel())
            base += row.size * num_neg
        else:
            e = (np.uint64(base) + np.arange(row.size * (1 + num_neg), dtype=np.uint64)) << np.uint64(32)
            items.append(np.concatenate([row[:, None], neg], axis=1).ravel())
            words.append(e | np.uint64(s))
            base += row.size * (1 + num_neg)
    return np.concatenate(items).astype(np.uint32), np.concatenate(words).astype(np.uint64)


def handle(d, *, pairwise, B, num_neg=5):
    """an MF handle on d (K = 8: nothing is trained), the data set by training position and a CDAE oracle for the draws on it"""
    m, _ = make(d, K=8, B=B, pairwise=pairwise, loss=cdae_amd.LOG if pairwise else cdae_amd.SQUARE, num_neg=num_neg)
    dp = in_training_order(d, m.user_order())
    return m, dp, cr.draw_oracle(dp, num_neg)


def check_window(m, o, dp, seed, epoch, u0, nb, pairwise):
    got = m.debug_sample_batch(seed, epoch, u0, nb)
    items, words = expected_examples(o, dp, seed, epoch, u0, nb, pairwise)
    nnz = int(dp.train_ptr[u0 + nb] - dp.train_ptr[u0])
    assert items.size == nnz * (2 * o.cfg.num_neg if pairwise else 1 + o.cfg.num_neg) == got["ex_item"].size
    # ---- the user-major list: items and words
    np.testing.assert_array_equal(got["ex_item"], items)
    np.testing.assert_array_equal(got["ex_val"], words)
    # ---- item-major order: a STABLE sort by item of the user-major list
    order = np.argsort(items, kind="stable")
    np.testing.assert_array_equal(got["sorted_item"], items[order])
    np.testing.assert_array_equal(got["sorted_val"] & NO_DUP, words[order])
    # ---- segments
    si = items[order]
    seg_b = np.zeros(dp.num_items, np.uint32)
    seg_e = np.zeros(dp.num_items, np.uint32)
    first = np.flatnonzero(np.r_[True, si[1:] != si[:-1]])
    last = np.flatnonzero(np.r_[si[1:] != si[:-1], True])
    seg_b[si[first]] = first
    seg_e[si[last]] = last + 1
    np.testing.assert_array_equal(got["seg_begin"], seg_b)
    np.testing.assert_array_equal(got["seg_end"], seg_e)
    return items


@pytest.fixture(scope="module")
def tiny(built):
    return synth.generate_shape("tiny", seed=5)


@pytest.mark.parametrize("pairwise", MODELS)
def test_d40_whole_window(built, pairwise):
    """the sequential schedule's window of all 8 users; 40 items: every item has examples, most users draw duplicates"""
    d = cr.d40()
    m, dp, o = handle(d, pairwise=pairwise, B=1)
    for ep in (0, 1):
        items = check_window(m, o, dp, 5, ep, 0, 8, pairwise)
        assert np.unique(items).size == 40
    check_window(m, o, dp, 5, 0, 3, 1, pairwise)              # the one-item user alone
    check_window(m, o, dp, 9, 2, 2, 5, pairwise)              # a window that starts inside the data set: slots are not positions


@pytest.mark.parametrize("num_neg", [1, 5])
@pytest.mark.parametrize("pairwise", MODELS)
def test_sequential_launch_windows(tiny, pairwise, num_neg):
    """batch_users = 1 on 300 users: the launch windows [0, 256) and [256, 300) as training cuts them"""
    m, dp, o = handle(tiny, pairwise=pairwise, B=1, num_neg=num_neg)
    np.testing.assert_array_equal(m.user_order(), np.arange(tiny.num_users))
    check_window(m, o, dp, 7, 0, 0, 256, pairwise)
    check_window(m, o, dp, 7, 1, 256, 44, pairwise)


@pytest.mark.parametrize("pairwise", MODELS)
def test_blocks_in_activity_grouped_order(tiny, pairwise):
    """B = 33: a full block and the last block of three; positions are not user ids, and the draws are keyed by position"""
    m, dp, o = handle(tiny, pairwise=pairwise, B=33)
    order = m.user_order()
    assert not np.array_equal(order, np.arange(tiny.num_users))
    assert not np.array_equal(order[33:66], np.arange(33, 66)) and not np.array_equal(order[297:], np.arange(297, 300))
    check_window(m, o, dp, 3, 0, 33, 33, pairwise)
    check_window(m, o, dp, 3, 1, 297, 3, pairwise)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("pairwise", MODELS)
def test_rows_longer_than_a_unit_of_64_positives(built, pairwise, B):
    """one wavefront of mf_sample_kernel per unit of 64 positives (batches of at most 1024 users): rows of 64, 65, 128, 129 and 257
    positives end exactly at a unit boundary, one past it, and in the fifth unit — at B = 1 (the sequential window, library sort) and
    as one block of five users (bucket_sort_kernel's key scan)"""
    rng = np.random.default_rng(6)
    d = cr.from_rows([np.sort(rng.choice(300, n, replace=False)) for n in (64, 65, 128, 129, 257)], 300)
    m, dp, o = handle(d, pairwise=pairwise, B=B)
    check_window(m, o, dp, 11, 0, 0, 5, pairwise)
    check_window(m, o, dp, 11, 1, 1, 3, pairwise)             # the first unit of the window is a later user's


@pytest.mark.parametrize("pairwise", MODELS)
def test_rows_longer_than_a_unit_of_128_positives(built, pairwise):
    """batch_users = 1200 > 1024: the host cuts units of 128 positives.  Three users with 128, 129 and 257 positives among 1200
    one-item users; the first block (1200 positions, the three long rows first: most active first) is one window."""
    rng = np.random.default_rng(7)
    lens = np.ones(1203, dtype=np.int64)
    lens[[400, 17, 1100]] = (128, 129, 257)
    d = cr.from_rows([np.sort(rng.choice(300, n, replace=False)) for n in lens], 300)
    m, dp, o = handle(d, pairwise=pairwise, B=1200)
    assert m.batch_users == 1200
    np.testing.assert_array_equal(np.diff(dp.train_ptr)[:4], (257, 129, 128, 1))
    np.testing.assert_array_equal(m.user_order()[:3], (1100, 17, 400))
    check_window(m, o, dp, 13, 0, 0, 1200, pairwise)


@pytest.mark.parametrize("pairwise", MODELS)
def test_more_than_65536_items_uses_32_bit_keys(built, pairwise):
    """70 000 items: no 16-bit key copies, the library radix sort on the 32-bit item ids + segment_kernel"""
    d = synth.generate(50, 70_000, 2_000, seed=4, min_items=20)
    m, dp, o = handle(d, pairwise=pairwise, B=50)
    items = check_window(m, o, dp, 3, 0, 0, 50, pairwise)
    assert items.max() > 65535
