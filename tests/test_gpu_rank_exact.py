"""Top-k ranking pinned exactly: models whose every score is an integer that fp32 holds exactly in ANY summation order (linear hidden
layer, small-integer parameters, helpers.assert_fp32_exact), so that rated_bits_kernel + recommend_mfma_kernel, the general
recommend_kernel, the host merge of the item-rows layout and the TOPN kernels must return the documented total order of
include/cdae_hip.h — descending score, equal scores by ascending item id, 0xFFFFFFFF beyond the user's unrated items — bit for bit,
for every user and every place.  The expected tables are integer arithmetic in numpy (helpers.exact_scores + rank_total_order,
themselves checked against the fp64 oracles in tests/test_rank_reference.py).  Every comparison is assert_array_equal over all users."""
import numpy as np
import pytest

import cdae_amd
import oracle as orc
from cdae_amd import synth
from helpers import SENTINEL, assert_fp32_exact, exact_scores, rank_total_order

pytestmark = pytest.mark.gpu

TOPKS = (1, 10, 16, 17, 24)          # <= 16: matrix cores when K <= 256; 17, 24 and every K > 256: general path
EXACT_UNRATED = (1, 7, 10, 16, 17, 24)
MODES = ("random", "zero", "levels", "half1", "half0", "last", "low")


# ---- data: rows that aim at the masks, then ordinary ones ----------------------------------------------------------------------
def special_rows(rng, I, which=None):
    """name -> sorted rated items.  tiles: whole 32-item tiles (all of [0, 200) but three items: with 8 item shards of ~125 items the
    first shard keeps fewer than topk candidates), the first and the last item; half0 / half1: every item of one lane half of
    recommend_mfma_kernel (items 8q + 0..3 / 8q + 4..7); leaves<n>: exactly n unrated items, some of them in the last tile; lowest:
    the lowest ids of the `low` plateau and part of the `last` one."""
    ids = np.arange(I)
    rows = {"tiles": np.setdiff1d(np.r_[np.arange(200), I - 1], [5, 77, 150]),
            "half0": ids[(ids & 4) == 0], "half1": ids[(ids & 4) != 0],
            "lowest": np.setdiff1d(np.r_[np.arange(13), np.arange(I - 40, I - 30)], [3])}
    for n in EXACT_UNRATED:
        keep = np.r_[rng.choice(I - 32, n - n // 2, replace=False), I - 1 - rng.choice(32, n // 2, replace=False)]
        rows[f"leaves{n}"] = np.setdiff1d(ids, keep)
    return {k: v.astype(np.uint32) for k, v in rows.items() if which is None or k in which}


def make_data(U, I, seed, rot=0, which=None):
    rng = np.random.default_rng(seed)
    sp = list(special_rows(rng, I, which).values())
    sp = sp[rot % len(sp):] + sp[:rot % len(sp)]
    rows = sp[:U] + [np.sort(rng.choice(I, size=int(rng.integers(1, 41)), replace=False)).astype(np.uint32) for _ in range(U - len(sp))]
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    return synth.Interactions(U, I, ptr, np.concatenate(rows), np.zeros(U + 1, np.int64), np.empty(0, np.uint32))


# ---- integer models ------------------------------------------------------------------------------------------------------------
def bias_pattern(mode, I):
    j = np.arange(I)
    if mode == "levels":     # three levels, each in every tile, in both lane halves and far more than 16 times per lane
        return (5 * j + j // 8 + j // 32) % 3
    if mode == "half1":      # the best level only in lane half 1 (items 8q + 4..7), the rest alternating
        return np.where((j & 4) != 0, 2, j % 2)
    if mode == "half0":
        return np.where((j & 4) == 0, 2, j % 2)
    if mode == "last":       # a plateau of 40 best scores at the very end: the last tile (partial or not) and a piece of the one before
        return np.where(j >= I - 40, 3, 0)
    if mode == "low":        # a plateau of 40 best scores at the lowest ids, which several users have rated
        return np.where(j < 40, 3, 0)
    raise AssertionError(mode)


def int_model(mode, U, I, K, asymmetric, seed, wmax=2):
    """Integer parameters as float64 arrays (keys W, b, Wu, bp and V when asymmetric)."""
    rng = np.random.default_rng(seed)
    dense = (lambda n: rng.integers(-wmax, wmax + 1, (n, K))) if wmax > 1 else (lambda n: rng.choice([-1, 0, 1], (n, K), p=[.1, .8, .1]))
    p = dict(W=dense(I), b=rng.integers(-3, 4, K), Wu=rng.integers(-3, 4, (U, K)), bp=rng.integers(-4, 5, I))
    if asymmetric:
        p["V"] = dense(I)
    if mode == "zero":
        p = {k: np.zeros_like(v) for k, v in p.items()}
    elif mode != "random":
        # every decoder row is the same vector (<= 16 non-zero coordinates): z . D[j] is one non-trivial number per user, computed
        # by the same MFMAs / fmas for every item, and the ranking is b' alone — the plateaus of bias_pattern
        r = np.zeros(K, dtype=np.int64)
        at = rng.choice(K, min(K, 16), replace=False)
        r[at] = rng.integers(1, wmax + 1, at.size) * rng.choice([-1, 1], at.size)
        p["V" if asymmetric else "W"] = np.tile(r, (I, 1))
        p["bp"] = bias_pattern(mode, I)
    return {k: v.astype(np.float64) for k, v in p.items()}


def load(model, p):
    model.set(cdae_amd.P_W, p["W"]); model.set(cdae_amd.P_B, p["b"]); model.set(cdae_amd.P_WU, p["Wu"]); model.set(cdae_amd.P_BP, p["bp"])
    if "V" in p:
        model.set(cdae_amd.P_V, p["V"])


def expected_table(d, p, topk, **kw):
    Z, S, D, bq = exact_scores(d.train_ptr, d.train_col, **p, **kw)
    assert_fp32_exact(Z, D, bq)                      # a condition on the inputs, checked before the GPU is touched
    return rank_total_order(S, d.train_ptr, d.train_col, topk)


def check_tables(model, d, want):
    """whole range and a sub-range that is not aligned to 128 users, every topk, every user, every place"""
    U = d.num_users
    a, b = (3, U - 2) if U > 6 else (U - 1, U)
    for topk in TOPKS:
        np.testing.assert_array_equal(model.recommend_all(topk, a, b), want[a:b, :topk], err_msg=f"sub-range, topk {topk}")
        np.testing.assert_array_equal(model.recommend_all(topk), want[:, :topk], err_msg=f"topk {topk}")


def check_sentinels(d, want):
    """(the expected table itself: a user with n < topk unrated items has exactly n ids, then the sentinel)"""
    left = d.num_items - np.diff(d.train_ptr)
    np.testing.assert_array_equal((want != SENTINEL).sum(axis=1), np.minimum(left, want.shape[1]))


def cdae_model(d, K, asymmetric, **kw):
    m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, linear=True, asymmetric=asymmetric, batch_users=32, **kw))
    m.reset(d, seed=1)
    return m


# K: the five instantiations of recommend_mfma_kernel (NCH 4 / 8 / 16 / 25 / 32), each also with pad columns; 300, 512: general path only.
# Users 1 / 127 / 129 / 301 (partial last workgroup); items with I mod 32 in {0, 1, 31, 17} and I mod 4 != 0 (961, 1023, 977).
SHAPES = [(8, 301, 977), (5, 129, 992), (64, 127, 961), (61, 301, 1023), (100, 129, 1023), (99, 1, 977), (200, 301, 961), (197, 127, 992),
          (256, 1, 1023), (250, 129, 977), (300, 127, 961), (512, 129, 1023)]


@pytest.mark.parametrize("asymmetric", [False, True])
@pytest.mark.parametrize("K,U,I", SHAPES)
def test_every_place_of_every_user(built, K, U, I, asymmetric):
    """Both recommend paths on random integer models (ties by the hundred) and on the designed plateaus, all masks; plus
    recommend_user with a foreign rated set in random order (general path, z encoded from that set)."""
    d = make_data(U, I, seed=K + U, rot=K + int(asymmetric))
    model = cdae_model(d, K, asymmetric)
    rng = np.random.default_rng(K)
    for mode in MODES:
        p = int_model(mode, U, I, K, asymmetric, seed=K + I)
        want = expected_table(d, p, max(TOPKS))
        check_sentinels(d, want)
        load(model, p)
        check_tables(model, d, want)
        if mode in ("random", "levels"):
            for uid in {0, U - 1}:
                foreign = rng.permutation(rng.choice(I, 30, replace=False)).astype(np.uint32)
                one = dict(p, Wu=p["Wu"][uid:uid + 1])
                Z, S, D, bq = exact_scores(np.array([0, 30]), np.sort(foreign), **one)
                assert_fp32_exact(Z, D, bq)
                for topk in (10, 24):
                    np.testing.assert_array_equal(model.recommend_user(uid, foreign, topk),
                                                  rank_total_order(S, None, None, topk, rated=[foreign])[0])


@pytest.mark.parametrize("K,U,asymmetric", [(8, 130, False), (300, 40, True)])
def test_more_than_65536_items(built, K, U, asymmetric):
    """70 050 items: 2190 bit words per user (> RATED_LDS_WORDS: rated_bits_kernel clears and fills the rows in global memory; 2190 is
    no multiple of 4, so every other row starts 8 bytes off a 16-byte boundary and has head and tail words outside the uint4 stores —
    the `tiles` and `lowest` users set bits in both), and the general path keeps its scores in the global workspace (280 KiB > LDS).
    The sub-range call lays other users' rows over the same words, so a word that is not cleared shows."""
    I = 70_050
    assert (I + 31) // 32 > 2048 and ((I + 31) // 32) % 4 == 2 and I * 4 + 64 > 160 * 1024
    d = make_data(U, I, seed=K, which=("tiles", "half1", "lowest", "leaves7", "leaves24"))
    model = cdae_model(d, K, asymmetric)
    for mode in ("random", "levels", "last", "low"):
        p = int_model(mode, U, I, K, asymmetric, seed=K + 1, wmax=1)
        want = expected_table(d, p, max(TOPKS))
        load(model, p)
        check_tables(model, d, want)


def test_sigmoid_beyond_18_is_exactly_0_or_1(built):
    """The default activation: hidden sums that all lie beyond +-18 give z in {0, 1} exactly (activate(), cdae_kernels.hpp), so the
    ranking of a NON-linear model is pinned the same way."""
    U, I, K = 129, 977, 64
    d = make_data(U, I, seed=9)
    rng = np.random.default_rng(9)
    model = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, linear=False, tanh=False, batch_users=32))
    model.reset(d, seed=1)
    for mode in ("random", "levels"):
        p = int_model(mode, U, I, K, False, seed=4)
        p["b"] = (rng.choice([-1, 1], K) * 5000).astype(np.float64)        # |sum W| <= 2 * 977, |Wu| <= 3
        want = expected_table(d, p, max(TOPKS), saturated_sigmoid=True)
        load(model, p)
        z = model.get_hidden_values(np.arange(U, dtype=np.uint32), mode=0)
        assert np.isin(z, (0.0, 1.0)).all() and 0 < z.mean() < 1
        check_tables(model, d, want)


@pytest.mark.parametrize("pairwise", [False, True])
@pytest.mark.parametrize("K,B", [(8, 1), (100, 64), (300, 16)])
def test_imf_and_bpr_handles(built, K, B, pairwise):
    """IMF / BPR: z = uv[u], D = iv, b' = ib; a non-zero integer ub shifts a user's scores alike and must not change the ranking.
    batch_users > 1 stores the user rows in training order: the user_perm branch of cdae_hip_recommend_all."""
    U, I = 301, 977
    d = make_data(U, I, seed=K + B)
    m = cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, pairwise=pairwise, lt=cdae_amd.LOG if pairwise else cdae_amd.SQUARE, batch_users=B))
    m.reset(d, seed=1)
    identity = np.array_equal(m.user_order(), np.arange(U))
    assert identity == (B == 1)                        # (the block schedule really permutes the rows)
    for mode in ("random", "levels", "low"):
        p = int_model(mode, U, I, K, False, seed=K)
        q = dict(uv=p["Wu"], iv=p["W"], ib=p["bp"], ub=np.random.default_rng(K).integers(-9, 10, U).astype(np.float64))
        Z, S, D, bq = exact_scores(d.train_ptr, d.train_col, **q)
        assert_fp32_exact(Z, D, bq)
        want = rank_total_order(S, d.train_ptr, d.train_col, max(TOPKS))
        m.set(cdae_amd.P_WU, q["uv"]); m.set(cdae_amd.P_W, q["iv"]); m.set(cdae_amd.P_BP, q["ib"]); m.set(cdae_amd.P_UB, q["ub"])
        np.testing.assert_array_equal(m.get(cdae_amd.P_WU), q["uv"])       # by user id, whatever the stored order
        check_tables(m, d, want)


@pytest.mark.parametrize("K,shards,item_rows", [(8, 2, True), (100, 3, True), (64, 8, True), (300, 3, True), (64, 3, False)])
def test_sharded_tables_equal_the_single_handle(built, K, shards, item_rows):
    """MultiCDAE over logical shards: the item-rows layout ranks every shard's items (general kernel, scores kept) and merges on the
    host — plateaus straddle the shard cuts, and the `tiles` user has fewer than topk candidates in the first of 8 shards; the user
    layout hands each shard its users.  Both must return the single handle's table, which is the expected one."""
    U, I = 129, 977
    d = make_data(U, I, seed=K + shards)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, linear=True, batch_users=32)
    one = cdae_amd.CDAE(cfg)
    one.reset(d, seed=1)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0] * shards, item_rows=item_rows)
    mm.reset(d, seed=1)
    if item_rows and shards == 8:
        cut = mm.shards()[0][1]
        row0 = d.train_col[d.train_ptr[0]:d.train_ptr[1]]
        assert 0 < cut - (row0 < cut).sum() < 10          # user 0 (`tiles`): fewer than 10 unrated items in shard 0
    for mode in MODES:
        p = int_model(mode, U, I, K, False, seed=K)
        want = expected_table(d, p, max(TOPKS))
        load(one, p)
        for which, key in ((cdae_amd.P_W, "W"), (cdae_amd.P_B, "b"), (cdae_amd.P_WU, "Wu"), (cdae_amd.P_BP, "bp")):
            mm.set(which, p[key])
        for topk in TOPKS:
            single = one.recommend_all(topk)
            np.testing.assert_array_equal(single, want[:, :topk])
            np.testing.assert_array_equal(mm.recommend_all(topk), single, err_msg=f"{mode} topk {topk}")
            np.testing.assert_array_equal(mm.recommend_all(topk, 3, U - 2), single[3:U - 2])


@pytest.mark.parametrize("K,U,I,asymmetric", [(8, 2, 40, False), (300, 3, 40, True)])
def test_fewer_unrated_items_than_topk_through_the_item_rows_merge(built, K, U, I, asymmetric):
    """Users with 3 and 12 unrated items in all, topk up to 20 (17 through the merge), 2 shards of about 20 items: the sentinel comes out of the matrix-core kernel,
    the general kernel (which used to repeat the lowest RATED id there) and the merge, after the user's unrated items in order."""
    rng = np.random.default_rng(K)
    rows = [np.setdiff1d(np.arange(I), keep).astype(np.uint32) for keep in ([7, 21, 39], [0, 1, 2, 3, 19, 20, 22, 30, 31, 32, 33, 38])]
    rows += [np.sort(rng.choice(I, 5, replace=False)).astype(np.uint32) for _ in range(U - 2)]
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    d = synth.Interactions(U, I, ptr, np.concatenate(rows), np.zeros(U + 1, np.int64), np.empty(0, np.uint32))
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, linear=True, asymmetric=asymmetric, batch_users=32)
    one = cdae_amd.CDAE(cfg)
    one.reset(d, seed=1)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0, 0], item_rows=True)
    mm.reset(d, seed=1)
    shard_items = min(b - a for a, b in mm.shards())        # (the merge takes topk candidates of every shard: topk <= its items)
    assert shard_items >= 17
    for mode in ("random", "zero", "levels"):
        p = int_model(mode, U, I, K, asymmetric, seed=K)
        want = expected_table(d, p, 20)
        np.testing.assert_array_equal((want != SENTINEL).sum(axis=1)[:2], [3, 12])
        load(one, p)
        for which, key in ((cdae_amd.P_W, "W"), (cdae_amd.P_B, "b"), (cdae_amd.P_WU, "Wu"), (cdae_amd.P_BP, "bp"), (cdae_amd.P_V, "V")):
            if key in p:
                mm.set(which, p[key])
        for topk in (1, 4, 10, 16, 17, 20):
            np.testing.assert_array_equal(one.recommend_all(topk), want[:, :topk], err_msg=f"{mode} topk {topk}")
            if topk <= shard_items:
                np.testing.assert_array_equal(mm.recommend_all(topk), want[:, :topk], err_msg=f"{mode} topk {topk} (item rows)")


def _test_rows(d, want, seed):
    """Validation rows: users without test items, with one, with several; about half of the items from the user's expected list
    (i.e. inside the tie plateaus), the rest from anywhere outside the train row."""
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(d.num_users):
        n = (0, 1, 3, 8)[u % 4]
        listed = want[u][want[u] != SENTINEL].astype(np.int64)
        free = np.setdiff1d(np.arange(d.num_items), d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]])
        pick = np.r_[rng.permutation(listed)[:(n + 1) // 2], rng.permutation(free)[:n]]
        rows.append(np.unique(pick)[:n].astype(np.uint32) if n else np.empty(0, np.uint32))
    return np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64), np.concatenate(rows)


def _hits(ids, tp, tc):
    h = np.zeros(3, dtype=np.uint64)
    for u in range(ids.shape[0]):
        inside = np.isin(ids[u, :20], tc[tp[u]:tp[u + 1]])
        h += np.array([inside[:1].sum(), inside[:5].sum(), inside[:10].sum()], dtype=np.uint64)
    return h


@pytest.mark.parametrize("kind,K", [("cdae", 64), ("cdae", 300), ("imf", 100)])
def test_topn_metrics_of_the_exact_tables(built, kind, K):
    """set_test_rows + eval_topn: the ids are the expected table, rets8 carries the bits of the oracle's sequential evaluation of that
    table (evaluation.hpp:113-219), hits3 the integer counts; topk 10, 5 and 16 (only min(topk, 20) places are scored on both sides).
    MultiCDAE.eval_topn (host loop over the merged table) gives the same 8 + 3 numbers."""
    U, I = 301, 977
    d = make_data(U, I, seed=K)
    if kind == "cdae":
        model = cdae_model(d, K, False)
        mm = cdae_amd.MultiCDAE(model.cfg, devices=[0] * 3, item_rows=True)
        mm.reset(d, seed=1)
    else:
        model = cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, batch_users=64))
        model.reset(d, seed=1)
        mm = None
    for mode in ("random", "levels"):
        p = int_model(mode, U, I, K, False, seed=K + 2)
        if kind == "cdae":
            want = expected_table(d, p, 16)
            load(model, p)
            for which, key in ((cdae_amd.P_W, "W"), (cdae_amd.P_B, "b"), (cdae_amd.P_WU, "Wu"), (cdae_amd.P_BP, "bp")):
                mm.set(which, p[key])
        else:
            Z, S, D, bq = exact_scores(d.train_ptr, d.train_col, uv=p["Wu"], iv=p["W"], ib=p["bp"])
            assert_fp32_exact(Z, D, bq)
            want = rank_total_order(S, d.train_ptr, d.train_col, 16)
            model.set(cdae_amd.P_WU, p["Wu"]); model.set(cdae_amd.P_W, p["W"]); model.set(cdae_amd.P_BP, p["bp"])
        tp, tc = _test_rows(d, want, seed=K)
        assert (np.diff(tp) == 0).any() and (np.diff(tp) == 1).any()
        model.set_test_rows(tp, tc)
        for topk in (10, 5, 16):
            rets, hits, ids = model.eval_topn(topk, with_ids=True)
            np.testing.assert_array_equal(ids, want[:, :topk])
            ref = orc.eval_topn(want[:, :topk], tp, tc)
            assert rets.tobytes() == ref.tobytes(), (topk, rets, ref)
            np.testing.assert_array_equal(hits, _hits(want[:, :topk], tp, tc))
            assert hits[2] > 0
            rets2, hits2 = model.eval_topn(topk)                       # without the id table
            assert rets2.tobytes() == ref.tobytes() and np.array_equal(hits2, hits)
            if mm is not None:
                rets_m, hits_m = mm.eval_topn(tp, tc, topk)
                assert rets_m.tobytes() == ref.tobytes(), (topk, rets_m, ref)
                np.testing.assert_array_equal(hits_m, hits)
