"""-m gpu: cdae_hip_warp_search — the device search of a WARP handle (cdae_warp_kernels.hpp warp_search, the function the training
kernels call) — against tests/warp_ref.py, EXACTLY: items, counts and margins.

The parameters are integer-valued (set through set_param), so every score is exact in fp32 in any summation order and a device decision
that differs from the reference's is a wrong candidate, a wrong order or a wrong comparison, never rounding.  Cases: every K tier edge
(padding lanes at the odd sizes), a user with one positive and one with every item but one, exact ties s(j) == s(i) - 1 (not violators),
first violators at draw 1, 64, 65 (the seam between two rounds of 64 candidates), 499 (the last draw that trains) and 500 (looked at by
nobody: the pair is skipped), num_neg 1 and 12, sub-ranges, a range that spans two chunks of 8 192 users.
"""
import numpy as np
import pytest

import cdae_amd
import mf_conflict_ref as mc
import warp_ref as wr

pytestmark = pytest.mark.gpu

SEED, EPOCH = 7, 3


def int_model(d, K, num_neg, rng, uv=None, iv=None, ib=None, epoch=EPOCH):
    """a WARP handle on d with integer-valued tables (about six non-zero coordinates per row whatever K: the scores stay near the margin)
    and the reference state of the same numbers"""
    U, I = d.num_users, d.num_items
    dens = min(1.0, 6.0 / K)

    def table(rows):
        return (rng.integers(-2, 3, (rows, K)) * (rng.random((rows, K)) < dens)).astype(np.float32)
    uv = table(U) if uv is None else uv
    iv = table(I) if iv is None else iv
    ib = rng.integers(-1, 2, I).astype(np.float32) if ib is None else ib
    m = cdae_amd.WARP(cdae_amd.WARPConfig(num_dim=K, num_neg=num_neg))
    m.reset(d, seed=1)
    np.testing.assert_array_equal(m.user_order(), np.arange(U))
    m.set(cdae_amd.P_WU, uv); m.set(cdae_amd.P_W, iv); m.set(cdae_amd.P_BP, ib)
    st = wr.State(uv, np.ones((U, K)), iv, np.ones((I, K)), ib)
    return m, st, wr.Draws(d.train_ptr, d.train_col, I, num_neg, SEED, epoch)


def ref_all(st, dr, pos_begin=0, pos_end=None):
    pos_end = dr.U if pos_end is None else pos_end
    out = [wr.search(st, dr, pos, p, k) for pos in range(pos_begin, pos_end) for p in range(int(dr.ptr[pos + 1] - dr.ptr[pos]))
           for k in range(dr.num_neg)]
    return (np.array([o[0] for o in out], dtype=np.uint32), np.array([o[1] for o in out], dtype=np.uint32),
            np.array([o[2] for o in out], dtype=np.float32))


def assert_search_equal(m, st, dr, pos_begin=0, pos_end=None, epoch=EPOCH):
    item, cnt, margin = m.search(SEED, epoch, pos_begin, pos_end, with_margin=True)
    r_item, r_cnt, r_margin = ref_all(st, dr, pos_begin, pos_end)
    np.testing.assert_array_equal(cnt, r_cnt)
    np.testing.assert_array_equal(item, r_item)
    np.testing.assert_array_equal(margin, r_margin)
    i2, c2 = m.search(SEED, epoch, pos_begin, pos_end)                 # without the margins: the same decisions
    np.testing.assert_array_equal(i2, item); np.testing.assert_array_equal(c2, cnt)
    return item, cnt, margin


def d40_plus():
    """D40 (a user with ONE positive among its eight) and a ninth user with every item but one"""
    d = mc.d40()
    rows = [d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]] for u in range(d.num_users)]
    return mc.from_rows(rows + [np.delete(np.arange(40), 23)], 40)


@pytest.mark.parametrize("K", [1, 64, 65, 128, 129, 256, 257, 512])
def test_every_k_tier_on_d40(built, K):
    d = d40_plus()
    assert 1 in np.diff(d.train_ptr) and 39 in np.diff(d.train_ptr)
    m, st, dr = int_model(d, K, 5, np.random.default_rng(K))
    item, cnt, margin = assert_search_equal(m, st, dr)
    assert (cnt == 1).any() and ((cnt > 1) & (cnt < wr.MAX_TRY)).any()
    assert ((cnt == wr.MAX_TRY) == (item == wr.NONE)).all()
    assert (margin[cnt < wr.MAX_TRY] > 0).all() and (margin[cnt == wr.MAX_TRY] == 0).all()
    last = slice(int(d.train_ptr[8]) * 5, None)                       # the user with one negative: the first draw or none
    assert set(cnt[last].tolist()) <= {1, wr.MAX_TRY} and set(item[last].tolist()) <= {23, wr.NONE}
    m.close()


def test_exact_ties_are_not_violators(built):
    """every candidate scores s(i) - 1 exactly except one item per user that scores s(i): the tie is passed over, the item found"""
    d12 = mc.d12()                                                     # D12 without item 11: an item nobody rated
    d = mc.from_rows([r[r != 11] for r in (d12.train_col[d12.train_ptr[u]:d12.train_ptr[u + 1]] for u in range(d12.num_users))], 12)
    assert np.diff(d.train_ptr).min() >= 1
    U, I, K = d.num_users, 12, 24
    rng = np.random.default_rng(5)
    rated = np.zeros((U, I), dtype=bool)
    rated[np.repeat(np.arange(U), np.diff(d.train_ptr)), d.train_col] = True
    unrated_by_all = np.nonzero(~rated.any(axis=0))[0]
    assert unrated_by_all.tolist() == [11]
    # coordinate x < I of an item row is 1 for item x alone, so uv[u, x] sets the score of (u, x) by itself; the other coordinates and the
    # biases are random integers that it compensates
    iv = np.zeros((I, K), dtype=np.float32); uv = np.zeros((U, K), dtype=np.float32)
    iv[np.arange(I), np.arange(I)] = 1.0
    iv[:, I:] = rng.integers(-2, 3, (I, K - I)); uv[:, I:] = rng.integers(-2, 3, (U, K - I))
    ib = rng.integers(-2, 3, I).astype(np.float32)
    target = np.where(rated, 5.0, 4.0)                                 # a positive scores 5, a negative 4 = 5 - 1: ties ...
    target[:, 11] = 5.0                                                # ... but for one item, a violator for every user
    uv[:, :I] = target - ib[None, :] - uv[:, I:] @ iv[:, I:].T
    m, st, dr = int_model(d, K, 3, rng, uv=uv, iv=iv, ib=ib)
    item, cnt, margin = assert_search_equal(m, st, dr)
    assert set(item.tolist()) <= {int(unrated_by_all[0]), wr.NONE} and (cnt > 1).any()
    assert (margin[cnt < wr.MAX_TRY] == 1.0).all()
    # and with nothing above the tie every search is exhausted
    ib[11] -= 1.0
    m.set(cdae_amd.P_BP, ib)
    item, cnt = m.search(SEED, EPOCH)
    assert (cnt == wr.MAX_TRY).all() and (item == wr.NONE).all()
    m.close()


def test_first_violators_at_the_seams_of_the_search(built):
    """six users with one positive each on 20 000 items; user a's only violator is the item its search draws at t_a = 0, 63, 64, 498, 499
    (and none): cnt 1, 64, 65, 499, and the last two skipped — the 500th draw is looked at by nobody"""
    I, K, epoch = 20_000, 24, 1                                        # (an epoch whose draws satisfy the premise asserted below)
    depths = (0, 63, 64, wr.LOOK - 1, wr.LOOK, None)
    d = mc.from_rows([[100 + u] for u in range(len(depths))], I)
    rng = np.random.default_rng(9)
    dr = wr.Draws(d.train_ptr, d.train_col, I, 1, SEED, epoch)
    key = [wr.rng_key(SEED, epoch, u, wr.STREAM_NEGATIVE) for u in range(len(depths))]
    cands = [[wr.sample_negative(key[u], wr.draw_index(0, 1, 0, t), [100 + u], I) for t in range(wr.MAX_TRY)] for u in range(len(depths))]
    violators = [cands[u][t] for u, t in enumerate(depths) if t is not None]
    for u, t in enumerate(depths):                                     # the premise: nobody meets a violator before its own
        seen = cands[u][:wr.LOOK if t is None else t]
        assert not set(seen) & set(violators), (u, t)
    uv = np.tile(rng.integers(-2, 3, K).astype(np.float32), (len(depths), 1))
    iv = rng.integers(-2, 3, (I, K)).astype(np.float32)
    target = np.full(I, -3.0)
    target[[100 + u for u in range(len(depths))]] = 2.0                # s(i) = 2: a violator scores above 1
    target[violators] = 2.0
    ib = (target - iv @ uv[0]).astype(np.float32)
    m, st, _ = int_model(d, K, 1, rng, uv=uv, iv=iv, ib=ib, epoch=epoch)
    item, cnt, margin = assert_search_equal(m, st, dr, epoch=epoch)
    assert cnt.tolist() == [1, 64, 65, wr.LOOK, wr.MAX_TRY, wr.MAX_TRY]
    assert item.tolist() == violators[:4] + [wr.NONE, wr.NONE]
    m.close()


@pytest.mark.parametrize("num_neg", [1, 12])
def test_num_neg_and_sub_ranges(built, num_neg):
    d = mc.d40()
    m, st, dr = int_model(d, 40, num_neg, np.random.default_rng(num_neg))
    item, cnt, _ = assert_search_equal(m, st, dr)
    assert item.size == int(d.train_ptr[-1]) * num_neg
    for a, b in ((3, 4), (2, 7), (7, 8), (5, 5)):                      # relative to the range's first positive
        i2, c2, _ = assert_search_equal(m, st, dr, a, b)
        lo, hi = int(d.train_ptr[a]) * num_neg, int(d.train_ptr[b]) * num_neg
        np.testing.assert_array_equal(i2, item[lo:hi]); np.testing.assert_array_equal(c2, cnt[lo:hi])
    m.close()


def test_a_range_that_spans_two_chunks(built):
    U = 8192 + 9                                                       # chunks of 8 192 users (include/cdae_hip.h)
    rng = np.random.default_rng(1)
    d = mc.from_rows([[int(i)] for i in rng.integers(0, 40, U)], 40)
    m, st, dr = int_model(d, 8, 1, rng)
    item, cnt, _ = assert_search_equal(m, st, dr)
    assert (cnt[8192:] < wr.MAX_TRY).any() and (cnt[:8192] < wr.MAX_TRY).any()
    assert_search_equal(m, st, dr, 8190, U)                            # a range that begins two users before the seam
    m.close()


def test_the_search_trains_nothing_and_checks_its_arguments(built):
    d = mc.d40()
    m, st, dr = int_model(d, 16, 2, np.random.default_rng(0))
    before = [m.get(w).copy() for w in (cdae_amd.P_WU, cdae_amd.P_WU_AG, cdae_amd.P_W, cdae_amd.P_W_AG, cdae_amd.P_BP)]
    m.search(SEED, EPOCH)
    for w, b in zip((cdae_amd.P_WU, cdae_amd.P_WU_AG, cdae_amd.P_W, cdae_amd.P_W_AG, cdae_amd.P_BP), before):
        np.testing.assert_array_equal(m.get(w), b)
    n = int(d.train_ptr[-1]) * 2
    buf = np.zeros(n + 1, dtype=np.uint32)
    lib = m.lib
    for bad_count in (n - 1, n + 1, 0):
        assert lib.cdae_hip_warp_search(m.h, SEED, EPOCH, 0, d.num_users, buf.ctypes.data, buf.ctypes.data, None, bad_count) != 0
        assert "pairs" in lib.cdae_hip_last_error().decode()
    assert lib.cdae_hip_warp_search(m.h, SEED, EPOCH, 5, 4, buf.ctypes.data, buf.ctypes.data, None, 0) != 0
    assert lib.cdae_hip_warp_search(m.h, SEED, EPOCH, 0, d.num_users + 1, buf.ctypes.data, buf.ctypes.data, None, n) != 0
    assert lib.cdae_hip_warp_search(m.h, SEED, EPOCH, 0, d.num_users, None, buf.ctypes.data, None, n) != 0
    with pytest.raises(cdae_amd.CDAEError, match="recorded"):
        m.choices()
    # what refuses an IMF / BPR handle refuses this one with the same text; there is no list before the step
    imf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=16))
    imf.reset(d, seed=1)
    for call in (lambda x: x.get_hidden_values([0, 1]), lambda x: x.train_one_user_corruption(0, [], []), lambda x: x.recommend_user(0, [1])):
        texts = []
        for handle in (imf, m):
            with pytest.raises(cdae_amd.CDAEError) as e:
                call(handle)
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    for call in (lambda: m.debug_sample_batch(1, 0, 0, 1), lambda: m.debug_row_pack(1, 0, 0, 1)):
        with pytest.raises(cdae_amd.CDAEError, match="no example list"):
            call()
    # and the three entry points refuse every other kind of handle
    for other in (imf, cdae_amd.WRMF(cdae_amd.WRMFConfig(num_dim=8)), cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=8, lt=cdae_amd.CROSS_ENTROPY))):
        if other is not imf:
            other.reset(d, seed=1)
        for rc in (lib.cdae_hip_warp_search(other.h, 0, 0, 0, 0, None, None, None, 0), lib.cdae_hip_warp_record_choices(other.h, 1),
                   lib.cdae_hip_warp_choices(other.h, None, None, 0)):
            assert rc != 0 and "applies to a WARP handle" in lib.cdae_hip_last_error().decode()
        other.close()
    m.close()
