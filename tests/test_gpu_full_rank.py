"""-m gpu: exact full-catalogue ranks of named items (cdae_hip_full_rank_rows).

out_ranks[p] = the number of items outside the row's rated set that precede target p in cdae_hip_recommend_all's total order
(descending score, equal scores by ascending item id): the place the item takes in the row's recommend_rows list of unbounded
length.  Pinned here:
  1. the exact order on integer models whose scores fp32 holds exactly, all five matrix-core instantiations and the general path,
     target rows that cross the 16-target window, one row that names ALL of its unrated items;
  2. agreement with the lists of recommend_rows on real-valued models: rank == place, score bitwise equal;
  3. the fp64 scores, within the derived fp32 bound;
  4. agreement with eval_topn_rows (integer hits exactly, the means within fp64 summation order);
  5. position independence, the row chunk, a row that spans several workgroups;
  6. edges and every refusal, after which the handle still answers correctly.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth
from cdae_amd.metrics import ranking_metrics
from full_rank_ref import NO_USER, csr, draw_targets, draw_uids, expected_ranks, rows_of
from test_gpu_rank_exact import bias_pattern, cdae_model, int_model, load, make_data, special_rows  # noqa: F401 (bias_pattern: through int_model)

pytestmark = pytest.mark.gpu

EVAL_CHUNK = 32768                   # rows per launch group (cdae_hip.hip)
MODES = ("random", "levels", "low", "last", "zero")


def int_rows(rng, I, R):
    """the mask-aimed rated sets of test_gpu_rank_exact (whole tiles, each lane half, exactly 7 items left), an empty row, then
    ordinary rows of 1-40 items"""
    rows = list(special_rows(rng, I, ("tiles", "half0", "half1", "leaves7")).values()) + [np.empty(0, np.uint32)]
    rows += [np.sort(rng.choice(I, size=int(rng.integers(1, 41)), replace=False)).astype(np.uint32) for _ in range(R - len(rows))]
    return rows


def plain_data(U, I, seed):
    """train rows of 1-5 items: what a handle needs before its rows entry points answer (they never read the train rows)"""
    rng = np.random.default_rng(seed)
    ptr, col = csr([np.sort(rng.choice(I, int(rng.integers(1, 6)), replace=False)).astype(np.uint32) for _ in range(U)])
    return synth.Interactions(U, I, ptr, col, np.zeros(U + 1, np.int64), np.empty(0, np.uint32))


# ---- 1. exact order on integer models ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,I", [(8, 977), (61, 992), (100, 1023), (200, 977), (256, 992), (300, 1023), (512, 977)])
def test_exact_ranks_on_integer_models(built, K, I):
    """K: the five instantiations of full_rank_mfma_kernel (NCH 4 / 8 / 16 / 25 / 32) and the general path (300, 512); 129 rows: a
    partial workgroup; I: a partial last tile, I mod 4 != 0 (977, 1023)."""
    U, R = 129, 129
    asymmetric = K in (61, 300)
    d = make_data(U, I, seed=K)
    model = cdae_model(d, K, asymmetric)
    rng = np.random.default_rng(2000 + K)
    rated = int_rows(rng, I, R)
    ptr, col = csr(rated)
    everything = (3, 11)                                           # `leaves7` and an ordinary row name ALL of their unrated items
    targets = draw_targets(rng, rated, I, all_of=everything)
    tptr, tcol = csr(targets)
    sizes = np.diff(tptr)
    assert {0, 1, 3, 16, 17, 40} <= set(sizes.tolist()) and sizes[3] == 7 and sizes[11] == I - rated[11].size > 900
    assert sum(0 in t and I - 1 in t for t in targets) > 30            # (wherever a row of 16 or more targets leaves them unrated)
    assert all(((t & 4) == 0).any() and ((t & 4) != 0).any() for t in targets[5:] if t.size >= 16)
    uids = draw_uids(rng, U, R)
    for mode in MODES:
        p = int_model(mode, U, I, K, asymmetric, seed=K + I)
        want, want_sc = expected_ranks(p, ptr, col, uids, tptr, tcol)
        load(model, p)
        ranks, sc = model.full_rank_rows(ptr, col, tptr, tcol, uids, with_scores=True)
        np.testing.assert_array_equal(ranks, want, err_msg=mode)
        np.testing.assert_array_equal(sc, want_sc, err_msg=mode)
        np.testing.assert_array_equal(model.full_rank_rows(ptr, col, tptr, tcol, uids), want)        # without scores
        for r in everything:                                       # exactly a permutation of 0 .. n - 1
            np.testing.assert_array_equal(np.sort(ranks[tptr[r]:tptr[r + 1]]), np.arange(sizes[r]))
        if mode == "zero":                                         # all scores equal: the unrated items with a lower id
            lower = np.concatenate([t - np.searchsorted(rt, t) for t, rt in zip(targets, rated)])
            np.testing.assert_array_equal(ranks, lower)
        if mode in ("low", "last"):                                # (the targets do sit inside the plateau of 40 equal best scores)
            assert ((tcol < 40) if mode == "low" else (tcol >= I - 40)).sum() > 100


# ---- real-valued models, shared by cases 2, 3 and 4 ---------------------------------------------------------------------------------
U_T, I_T = 200, 977


@functools.lru_cache(maxsize=None)
def real_model(K):
    """random float parameters, the default sigmoid hidden layer"""
    d = synth.generate(U_T, I_T, U_T * 40, seed=7, min_items=5)
    m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64))
    m.reset(d, seed=3)
    rng = np.random.default_rng(K)
    m.set(cdae_amd.P_W, rng.normal(0, 0.3, (I_T, K))); m.set(cdae_amd.P_B, rng.normal(0, 0.3, K))
    m.set(cdae_amd.P_WU, rng.normal(0, 0.3, (U_T, K))); m.set(cdae_amd.P_BP, rng.normal(0, 0.3, I_T))
    return m, d


@functools.lru_cache(maxsize=None)
def foreign_rows(R=150, seed=5):
    """rows that are no train rows (1-60 items, one of 300: several summation groups), user ids with repeats and NO_USER"""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(I_T, 300, replace=False)).astype(np.uint32)]
    rows += [np.sort(rng.choice(I_T, int(rng.integers(1, 61)), replace=False)).astype(np.uint32) for _ in range(R - 1)]
    return csr(rows) + (draw_uids(rng, U_T, R),)


# ---- 2. agreement with the lists ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,topks", [(64, (16,)), (200, (16,)), (300, (10, 24))])
def test_listed_ids_get_their_place_and_their_score(built, K, topks):
    model, _ = real_model(K)
    ptr, col, uids = foreign_rows()
    R = ptr.size - 1
    for topk in topks:
        ids, sc = model.recommend_rows(ptr, col, uids, topk, with_scores=True)
        assert (ids != 0xFFFFFFFF).all() and np.unique(sc).size > R
        order = np.argsort(ids, axis=1)                            # targets ascend inside a row
        tptr, tcol = np.arange(R + 1, dtype=np.int64) * topk, np.take_along_axis(ids, order, axis=1).ravel()
        ranks, tsc = model.full_rank_rows(ptr, col, tptr, tcol, uids, with_scores=True)
        np.testing.assert_array_equal(ranks.reshape(R, topk), order)                               # rank == place
        assert tsc.reshape(R, topk).tobytes() == np.take_along_axis(sc, order, axis=1).tobytes()   # bitwise


# ---- 3. against fp64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 200, 300])
def test_ranks_lie_in_the_fp64_interval(built, K):
    """train rows with their own users, so that get_hidden_values returns the fp32 z the call ranks from (include/cdae_hip.h:
    a row equal to a train row has the handle's inference z).  eps: the bound helpers.assert_valid_topk(eps="derived") uses,
    2 (Kc + 2) 2^-24 max_j (sum_k |z_k D_jk| + |b'_j|).  Every rank lies in [#{s > t + eps}, #{s >= t - eps} - 1] over the unrated."""
    model, d = real_model(K)
    U = d.num_users
    uids = np.arange(U, dtype=np.uint32)
    rng = np.random.default_rng(K + 1)
    rated = rows_of(d.train_ptr, d.train_col)
    tptr, tcol = csr(draw_targets(rng, rated, I_T))
    ranks, sc = model.full_rank_rows(d.train_ptr, d.train_col, tptr, tcol, uids, with_scores=True)
    z = model.get_hidden_values(uids, mode=0).astype(np.float64)[:, :K]
    D = model.get(cdae_amd.P_W).astype(np.float64).reshape(I_T, -1)[:, :K]
    bp = model.get(cdae_amd.P_BP).astype(np.float64)
    Kc = int(model.lib.cdae_hip_row_stride(model.h))
    eps = 2.0 * (Kc + 2) * 2.0 ** -24 * (np.abs(z) @ np.abs(D).T + np.abs(bp)).max(axis=1)
    S = z @ D.T + bp
    for r in range(U):
        s = S[r].copy()
        s[rated[r].astype(np.int64)] = -np.inf
        for p in range(tptr[r], tptr[r + 1]):
            t = S[r, tcol[p]]
            lo, hi = int((s > t + eps[r]).sum()), int((s >= t - eps[r]).sum()) - 1
            assert lo <= ranks[p] <= hi, (r, tcol[p], lo, int(ranks[p]), hi)
            assert abs(float(sc[p]) - t) <= eps[r]
    assert np.unique(ranks).size > 300


# ---- 4. agreement with eval_topn_rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [200, 300])
def test_the_metrics_agree_with_eval_topn_rows(built, K):
    model, _ = real_model(K)
    ptr, col, uids = foreign_rows()
    R = ptr.size - 1
    rng = np.random.default_rng(K + 2)
    rated = rows_of(ptr, col)
    listed = model.recommend_rows(ptr, col, uids, 10)
    targets = []
    for r in range(R):                                             # about half of the targets from the row's list, so that there are hits
        free = np.setdiff1d(np.arange(I_T, dtype=np.uint32), rated[r])
        n = (0, 1, 4, 9)[r % 4]
        pick = np.r_[rng.permutation(listed[r])[:(n + 1) // 2], rng.permutation(free)[:n]]
        targets.append(np.unique(pick)[:n].astype(np.uint32) if n else np.empty(0, np.uint32))
    tptr, tcol = csr(targets)
    rets, hits = model.eval_topn_rows(ptr, col, tptr, tcol, uids, 10)
    ranks = model.full_rank_rows(ptr, col, tptr, tcol, uids)
    np.testing.assert_array_equal(hits, np.array([(ranks < k).sum() for k in (1, 5, 10)], dtype=np.uint64))
    assert hits[0] > 0 and hits[2] > hits[0]
    m = ranking_metrics(tptr, ranks, I_T - np.diff(ptr), (1, 5, 10))
    names = ["precision@1", "precision@5", "precision@10", "recall@1", "recall@5", "recall@10", "map@5", "map@10"]
    for name, want in zip(names, rets):
        assert abs(m[name] - want) <= R * 2.0 ** -52 * abs(want), (name, m[name], want)
    full = model.eval_ranking_rows(ptr, col, tptr, tcol, uids)
    assert full["recall@10"] == m["recall@10"] and full["recall@100"] >= full["recall@50"] >= full["recall@20"] >= m["recall@10"]
    assert 0.0 < full["mrr"] <= 1.0 and 0.0 < full["auc"] <= 1.0 and full["rows"] == (np.diff(tptr) > 0).sum()


# ---- 5. position independence and chunking ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [200, 300])
def test_a_subset_of_the_rows_in_another_order_gives_the_same_bits(built, K):
    model, _ = real_model(K)
    ptr, col, uids = foreign_rows()
    R = ptr.size - 1
    rng = np.random.default_rng(K + 3)
    rated = rows_of(ptr, col)
    targets = draw_targets(rng, rated, I_T, all_of=(7,))
    tptr, tcol = csr(targets)
    ranks, sc = model.full_rank_rows(ptr, col, tptr, tcol, uids, with_scores=True)
    pick = rng.permutation(R)[:R // 3]
    pick = np.r_[pick, 7] if 7 not in pick else pick
    ptr2, col2 = csr([rated[r] for r in pick])
    tptr2, tcol2 = csr([targets[r] for r in pick])
    ranks2, sc2 = model.full_rank_rows(ptr2, col2, tptr2, tcol2, uids[pick], with_scores=True)
    for n, r in enumerate(pick):
        np.testing.assert_array_equal(ranks2[tptr2[n]:tptr2[n + 1]], ranks[tptr[r]:tptr[r + 1]])
        assert sc2[tptr2[n]:tptr2[n + 1]].tobytes() == sc[tptr[r]:tptr[r + 1]].tobytes()


def test_rows_beyond_one_chunk(built):
    """32 768 + 5 rows of one target each at K = 8, I = 40: two launch groups"""
    U, I, K, R = 129, 40, 8, EVAL_CHUNK + 5
    rng = np.random.default_rng(55)
    d = plain_data(U, I, seed=3)
    model = cdae_model(d, K, False)
    p = int_model("random", U, I, K, False, seed=5)
    load(model, p)
    lens = rng.integers(0, 6, R)
    flat = np.argsort(rng.random((R, I)), axis=1).astype(np.uint32)
    rated = [np.sort(flat[r, :lens[r]]) for r in range(R)]
    ptr, col = csr(rated)
    tptr, tcol = np.arange(R + 1, dtype=np.int64), flat[:, 7].copy()          # one unrated item per row
    uids = draw_uids(rng, U, R)
    want, want_sc = expected_ranks(p, ptr, col, uids, tptr, tcol)
    ranks, sc = model.full_rank_rows(ptr, col, tptr, tcol, uids, with_scores=True)
    np.testing.assert_array_equal(ranks, want)
    np.testing.assert_array_equal(sc, want_sc)
    assert np.unique(ranks[EVAL_CHUNK:]).size > 1


@pytest.mark.parametrize("K", [8, 300])
def test_one_row_with_more_targets_than_a_workgroup_has_windows(built, K):
    """I = 4001, one row that names all of its ~3 960 unrated items: more than 16 x 128 targets, so its windows fill several
    workgroups of the counting launch (K = 8); K = 300: the general path's wavefronts take them in turn.  Around it two ordinary rows."""
    U, I = 5, 4001
    d = plain_data(U, I, seed=K)
    model = cdae_model(d, K, False)
    rng = np.random.default_rng(K)
    rated = [np.sort(rng.choice(I, n, replace=False)).astype(np.uint32) for n in (12, 41, 30)]
    targets = draw_targets(rng, rated, I, all_of=(1,))
    targets[0], targets[2] = targets[0][:0], np.sort(rng.choice(np.setdiff1d(np.arange(I, dtype=np.uint32), rated[2]), 17, replace=False))
    ptr, col = csr(rated)
    tptr, tcol = csr(targets)
    assert tptr[2] - tptr[1] == I - 41 > 16 * 128
    uids = np.array([4, NO_USER, 0], dtype=np.uint32)
    for mode in ("random", "levels"):
        p = int_model(mode, U, I, K, False, seed=K + 1, wmax=1)
        want, want_sc = expected_ranks(p, ptr, col, uids, tptr, tcol)
        load(model, p)
        ranks, sc = model.full_rank_rows(ptr, col, tptr, tcol, uids, with_scores=True)
        np.testing.assert_array_equal(ranks, want, err_msg=mode)
        np.testing.assert_array_equal(sc, want_sc)
        np.testing.assert_array_equal(np.sort(ranks[tptr[1]:tptr[2]]), np.arange(I - 41))


# ---- 6. edges and refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [61, 300])
def test_edges_and_refusals_leave_the_handle_usable(built, K):
    U, I, R = 129, 977, 60
    d = make_data(U, I, seed=K)
    model = cdae_model(d, K, False)
    p = int_model("random", U, I, K, False, seed=K + I)
    load(model, p)
    rng = np.random.default_rng(7)
    rated = int_rows(rng, I, R)
    ptr, col = csr(rated)
    targets = draw_targets(rng, rated, I)
    tptr, tcol = csr(targets)
    uids = draw_uids(rng, U, R)
    assert (uids == NO_USER).any() and (uids != NO_USER).any()
    want, want_sc = expected_ranks(p, ptr, col, uids, tptr, tcol)

    def still_right():
        ranks, sc = model.full_rank_rows(ptr, col, tptr, tcol, uids, with_scores=True)
        np.testing.assert_array_equal(ranks, want)
        np.testing.assert_array_equal(sc, want_sc)
    still_right()
    still_right()                                                  # (a second identical call: the grown buffers are reused)
    # edges that succeed
    assert model.full_rank_rows(np.zeros(1, np.int64), np.empty(0, np.uint32), np.zeros(1, np.int64), np.empty(0, np.uint32)).shape == (0,)
    assert model.lib.cdae_hip_full_rank_rows(model.h, 0, None, None, None, None, None, None, None) == 0
    assert model.full_rank_rows(ptr, col, np.zeros(R + 1, np.int64), np.empty(0, np.uint32), uids).shape == (0,)
    no_targets = np.zeros(R + 1, np.int64)
    assert model.lib.cdae_hip_full_rank_rows(model.h, R, None, ptr.ctypes.data, col.ctypes.data, no_targets.ctypes.data, None, None, None) == 0
    none, none_sc = expected_ranks(p, ptr, col, None, tptr, tcol)
    got, got_sc = model.full_rank_rows(ptr, col, tptr, tcol, None, with_scores=True)          # uids=None: no user node anywhere
    np.testing.assert_array_equal(got, none)
    np.testing.assert_array_equal(got_sc, none_sc)
    # refusals that name the row
    big = next(r for r in range(R) if targets[r].size >= 16 and rated[r].size)
    a = int(tptr[big])
    assert rated[big].size

    def changed(at, value):
        c = tcol.copy(); c[at] = value
        return c
    first_rated = int(rated[big][0]) if not np.isin(rated[big][0], targets[big]) else None
    assert first_rated is not None
    in_rated = np.sort(np.r_[targets[big][1:], np.uint32(first_rated)]).astype(np.uint32)       # one target replaced by a rated item
    bad = [(np.r_[tcol[:a], in_rated, tcol[tptr[big + 1]:]].astype(np.uint32), f"row {big}"),
           (np.r_[tcol[:a], tcol[a + 1], tcol[a], tcol[a + 2:]].astype(np.uint32), f"row {big}"),      # unsorted
           (changed(a + 1, tcol[a]), f"row {big}"),                                                     # duplicate
           (changed(int(tptr[big + 1]) - 1, I), f"row {big}")]                                         # out of range
    for c, word in bad:
        with pytest.raises(cdae_amd.CDAEError, match=word):
            model.full_rank_rows(ptr, col, tptr, c, uids)
        still_right()
    rc = model.lib.cdae_hip_full_rank_rows(model.h, R, uids.ctypes.data, ptr.ctypes.data, col.ctypes.data, tptr.ctypes.data, tcol.ctypes.data,
                                           None, None)
    assert rc != 0 and b"out_ranks" in model.lib.cdae_hip_last_error()
    still_right()
    # an IMF / BPR handle, an item shard, a handle without interactions
    mf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=8, batch_users=1))
    mf.reset(d, seed=1)
    with pytest.raises(cdae_amd.CDAEError, match="IMF / BPR"):
        mf.full_rank_rows(ptr, col, tptr, tcol)
    np.testing.assert_array_equal(mf.recommend_all(10).shape, (U, 10))           # (still usable)
    mm = cdae_amd.MultiCDAE(model.cfg, devices=[0, 0], item_rows=True)
    mm.reset(d, seed=1)
    shard, out = C.c_void_p(), np.empty(tcol.size, np.uint32)
    assert mm.lib.cdae_hip_multi_shard(mm.h, 0, C.byref(shard), None, None) == 0
    rc = mm.lib.cdae_hip_full_rank_rows(shard, R, None, ptr.ctypes.data, col.ctypes.data, tptr.ctypes.data, tcol.ctypes.data, out.ctypes.data, None)
    assert rc != 0 and b"item shard" in mm.lib.cdae_hip_last_error()
    np.testing.assert_array_equal(mm.recommend_all(10).shape, (U, 10))           # (still usable)
    fresh = cdae_amd.CDAE(model.cfg)
    with pytest.raises(cdae_amd.CDAEError, match="set_interactions"):
        fresh.full_rank_rows(ptr, col, tptr, tcol)
    fresh.reset(d, seed=1)
    load(fresh, p)
    np.testing.assert_array_equal(fresh.full_rank_rows(ptr, col, tptr, tcol, uids), want)
    still_right()


def test_an_input_free_model_ranks_by_the_empty_input(built):
    """corruption_ratio == 1: z is encoded from nothing (cdae.hpp:168-172), the row is still excluded"""
    U, I, K, R = 64, 977, 100, 40
    d = make_data(U, I, seed=K)
    model = cdae_model(d, K, False, corruption_ratio=1.0, scaled=False)
    p = int_model("random", U, I, K, False, seed=K)
    load(model, p)
    rng = np.random.default_rng(9)
    rated = int_rows(rng, I, R)
    ptr, col = csr(rated)
    tptr, tcol = csr(draw_targets(rng, rated, I))
    uids = draw_uids(rng, U, R)
    want, want_sc = expected_ranks(dict(p, W=np.zeros_like(p["W"]), V=p["W"]), ptr, col, uids, tptr, tcol)   # nothing summed, D = W
    ranks, sc = model.full_rank_rows(ptr, col, tptr, tcol, uids, with_scores=True)
    np.testing.assert_array_equal(ranks, want)
    np.testing.assert_array_equal(sc, want_sc)
