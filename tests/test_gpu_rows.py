"""-m gpu: batched top-k and TOPN for rated sets the caller supplies (cdae_hip_recommend_rows / cdae_hip_eval_topn_rows).

recommend(uid, topk, rated_item_set) of the reference (cdae.hpp:162-196) encodes the hidden layer FROM the given set and excludes
exactly that set.  The batched entry points do that for a CSR of rows that need not be train rows, with a row -> user indirection
(any user any number of times, NO_USER for a row without a user node), on both recommend paths.  Pinned here:
  * the documented total order, every row and every place, on integer models whose scores fp32 holds exactly (helpers.exact_scores),
    with the returned scores equal to the integer scores and -inf in the sentinel places;
  * bit identity with a TWIN handle whose train rows are the caller's rows and whose private rows are the gathered ones: the
    summation order of the input sum is part of the contract (include/cdae_hip.h);
  * train rows with uids 0..U-1 reproduce recommend_all and eval_topn;
  * the fp64 oracle over the caller's rows; the chunk boundary; item spaces beyond 65 536; every refusal; and the wall-clock
    comparison with the loop of recommend_user calls the batched call replaces.
"""
import functools
import time

import numpy as np
import pytest

import cdae_amd
import oracle as orc
from cdae_amd import synth
from helpers import SENTINEL, assert_fp32_exact, assert_valid_topk, exact_scores, rank_total_order, record_measured
from test_gpu_rank_exact import bias_pattern, cdae_model, int_model, load, make_data, special_rows  # noqa: F401 (bias_pattern: through int_model)

pytestmark = pytest.mark.gpu

NO_USER = cdae_amd.NO_USER
TOPKS = (1, 10, 16, 17, 24)          # <= 16: matrix cores when K <= 256; 17, 24 and every K > 256: general path
EVAL_CHUNK = 32768                   # rows per launch group (cdae_hip.hip)


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
    """M[uids], rows of `fill` where the row has no user node (or everywhere, uids None)"""
    out = np.full((len(uids), M.shape[1]), fill, dtype=M.dtype)
    real = np.asarray(uids) != NO_USER
    out[real] = M[np.asarray(uids)[real].astype(np.int64)]
    return out


def expected_rows(p, ptr, col, uids, topk):
    """(ids, scores) of the documented order for integer parameters p; scores as float32, -inf in the sentinel places"""
    R = ptr.size - 1
    u = np.full(R, NO_USER, dtype=np.uint32) if uids is None else uids
    q = dict(p, Wu=gathered(p["Wu"], u, 0.0))
    Z, S, D, bq = exact_scores(ptr, col, **q)
    assert_fp32_exact(Z, D, bq)                      # a condition on the inputs, checked before the GPU is touched
    ids = rank_total_order(S, ptr, col, topk)
    sc = np.where(ids == SENTINEL, -np.inf, np.take_along_axis(S, np.minimum(ids, S.shape[1] - 1).astype(np.int64), axis=1)).astype(np.float32)
    return ids, sc


def foreign_int_rows(rng, I, R):
    """the mask-aimed sets of test_gpu_rank_exact (whole tiles, each lane half, exactly 1 / 7 / 10 / 16 / 17 / 24 items left: sentinels
    on both paths), an empty row, then ordinary rows of 1-40 items"""
    rows = list(special_rows(rng, I).values()) + [np.empty(0, np.uint32)]
    rows += [np.sort(rng.choice(I, size=int(rng.integers(1, 41)), replace=False)).astype(np.uint32) for _ in range(R - len(rows))]
    return rows


# ---- 1. exact total order on integer models ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("asymmetric", [False, True])
@pytest.mark.parametrize("K", [8, 61, 100, 200, 250, 300])      # the five NCH instantiations, with pad columns; 300: general path
def test_every_place_of_every_row(built, K, asymmetric):
    U, I, R = 129, 977, 301
    d = make_data(U, I, seed=K)
    model = cdae_model(d, K, asymmetric)
    rng = np.random.default_rng(1000 + K)
    ptr, col = csr(foreign_int_rows(rng, I, R))
    assert not np.array_equal(ptr[:U + 1], d.train_ptr)
    uids = draw_uids(rng, U, R)
    assert (uids == NO_USER).any() and np.unique(uids).size < R
    for mode in ("random", "levels", "half1", "last", "low"):
        p = int_model(mode, U, I, K, asymmetric, seed=K + I)
        load(model, p)
        want, want_sc = expected_rows(p, ptr, col, uids, max(TOPKS))
        np.testing.assert_array_equal((want != SENTINEL).sum(axis=1), np.minimum(I - np.diff(ptr), max(TOPKS)))
        for topk in TOPKS:
            ids, sc = model.recommend_rows(ptr, col, uids, topk, with_scores=True)
            np.testing.assert_array_equal(ids, want[:, :topk], err_msg=f"{mode} topk {topk}")
            np.testing.assert_array_equal(sc, want_sc[:, :topk], err_msg=f"{mode} topk {topk} scores")
            np.testing.assert_array_equal(model.recommend_rows(ptr, col, uids, topk), want[:, :topk])        # without scores
        if mode == "random":
            none, none_sc = expected_rows(p, ptr, col, None, 17)
            for topk in (16, 17):
                ids, sc = model.recommend_rows(ptr, col, None, topk, with_scores=True)
                np.testing.assert_array_equal(ids, none[:, :topk])
                np.testing.assert_array_equal(sc, none_sc[:, :topk])


# ---- trained real-valued models, shared by cases 2, 3, 4 and 8 --------------------------------------------------------------------
U_T, I_T = 300, 977


@functools.lru_cache(maxsize=None)
def trained(K, flags=()):
    d = synth.generate(U_T, I_T, U_T * 40, seed=7, min_items=5)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64, **dict(flags))
    m = cdae_amd.CDAE(cfg)
    m.reset(d, seed=3)
    for ep in range(2):
        m.train_one_iteration(3, ep)
    return m, d


@functools.lru_cache(maxsize=None)
def foreign(R=260, seed=5):
    """rows that are no train rows: three longer than 2 x 128 items (several summation groups whatever the unit), one of a single
    item, ordinary ones of 1-60 items (no empty one: the twin handle's train rows may not be empty; cases 1, 5 and 6 have them); permuted user ids, some rows without a user node; target sets outside the rows, some empty"""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(I_T, n, replace=False)).astype(np.uint32) for n in (300, 257, 129, 1)]
    rows += [np.sort(rng.choice(I_T, int(rng.integers(1, 61)), replace=False)).astype(np.uint32) for _ in range(R - len(rows))]
    uids = rng.permutation(U_T)[:R].astype(np.uint32)
    uids[rng.random(R) < 0.15] = NO_USER
    uids[0] = 17                                     # a long row with a user node, one without
    uids[1] = NO_USER
    targets = []
    for r, row in enumerate(rows):
        free = np.setdiff1d(np.arange(I_T, dtype=np.uint32), row)
        targets.append(np.sort(rng.choice(free, (0, 1, 4, 9)[r % 4], replace=False)).astype(np.uint32))
    return csr(rows) + (uids,) + csr(targets)


def twin_of(model, ptr, col, uids):
    """a handle with the same configuration whose TRAIN rows are the caller's rows and whose private rows are the gathered ones"""
    cfg, K = model.cfg, model.cfg.num_dim
    tw = cdae_amd.CDAE(cfg)
    tw.set_interactions(ptr.size - 1, model.num_items, ptr, col)
    tw.init_params(0)
    for which in (cdae_amd.P_W, cdae_amd.P_B, cdae_amd.P_BP) + ((cdae_amd.P_V,) if cfg.asymmetric else ()):
        tw.set(which, model.get(which))
    tw.set(cdae_amd.P_WU, gathered(model.get(cdae_amd.P_WU), uids, 0.0))
    if cfg.linear_function:
        tw.set(cdae_amd.P_UU, gathered(model.get(cdae_amd.P_UU), uids, 1.0))
    assert K == tw.cfg.num_dim
    return tw


# ---- 2. bit identity with a twin handle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags", [(200, ()), (300, ()), (40, (("linear_function", True),)), (40, (("tanh", True),)),
                                     (40, (("corruption_ratio", 1.0), ("scaled", False)))])
def test_a_twin_handle_returns_the_same_bits(built, K, flags):
    model, d = trained(K, flags)
    ptr, col, uids, _, _ = foreign()
    assert np.diff(ptr).max() > 2 * 128
    tw = twin_of(model, ptr, col, uids)
    z = tw.get_hidden_values(np.arange(ptr.size - 1, dtype=np.uint32), mode=0)
    assert np.isfinite(z).all() and np.unique(z[:, 0]).size > (1 if dict(flags).get("corruption_ratio") == 1.0 else 50)
    for topk in (10, 24):
        got = model.recommend_rows(ptr, col, uids, topk)
        np.testing.assert_array_equal(got, tw.recommend_all(topk), err_msg=f"topk {topk}")
        assert not any(np.intersect1d(g, r).size for g, r in zip(got, rows_of(ptr, col)))
    tw.close()


def test_a_twin_handle_returns_the_same_bits_in_groups_of_128(built):
    """the other branch of the summation contract: min(batch_users, num_users) > 1024 on BOTH handles, so the work unit — the group
    of the input sum — is 128 items.  A group of 65-128 items then spans two 64-lane passes of one wavefront; rows of 129, 257 and
    300 items have 2, 3 and 3 groups (one of them a single item), rows of exactly 128 and 127 items have one."""
    U, K, R = 1100, 40, 1100
    d = synth.generate(U, I_T, U * 20, seed=9, min_items=5)
    model = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=2048))
    model.reset(d, seed=3)
    model.train_one_iteration(3, 0)
    assert min(model.cfg.batch_users, U) > 1024 and min(model.cfg.batch_users, R) > 1024
    rng = np.random.default_rng(12)
    lens = [300, 257, 129, 128, 127, 100, 65, 64, 1] + [int(rng.integers(1, 61)) for _ in range(R - 9)]
    ptr, col = csr([np.sort(rng.choice(I_T, n, replace=False)).astype(np.uint32) for n in lens])
    uids = draw_uids(rng, U, R)
    uids[0], uids[1] = 17, NO_USER
    tw = twin_of(model, ptr, col, uids)
    z = tw.get_hidden_values(np.arange(R, dtype=np.uint32), mode=0)
    assert np.isfinite(z).all() and np.unique(z[:, 0]).size > 50
    for topk in (10, 24):
        np.testing.assert_array_equal(model.recommend_rows(ptr, col, uids, topk), tw.recommend_all(topk), err_msg=f"topk {topk}")
    tw.close()


# ---- 3. train rows and arange uids reproduce recommend_all / eval_topn -------------------------------------------------------------
@pytest.mark.parametrize("K", [200, 300])
def test_train_rows_reproduce_recommend_all_and_eval_topn(built, K):
    model, d = trained(K)
    uids = np.arange(U_T, dtype=np.uint32)
    for topk in (10, 24):
        np.testing.assert_array_equal(model.recommend_rows(d.train_ptr, d.train_col, uids, topk), model.recommend_all(topk))
    model.set_test_rows(d.test_ptr, d.test_col)
    for topk in (10, 24):
        rets, hits, ids = model.eval_topn(topk, with_ids=True)
        rets2, hits2, ids2 = model.eval_topn_rows(d.train_ptr, d.train_col, d.test_ptr, d.test_col, uids, topk, with_ids=True)
        assert (rets2 == rets).all() and (hits2 == hits).all(), (rets, rets2, hits, hits2)
        np.testing.assert_array_equal(ids2, ids)
        rets3, hits3 = model.eval_topn_rows(d.train_ptr, d.train_col, d.test_ptr, d.test_col, uids, topk)
        assert (rets3 == rets).all() and (hits3 == hits).all()
    assert rets[5] > 0


# ---- 4. against the fp64 oracle -----------------------------------------------------------------------------------------------------
def _clear_rows(sc, tol=1e-4):
    return np.abs(np.diff(sc, axis=1)).min(axis=1) > tol


@pytest.mark.parametrize("K", [200, 300])
def test_against_the_fp64_oracle_over_the_callers_rows(built, K):
    model, d = trained(K)
    ptr, col, uids, tptr, tcol = foreign()
    R = ptr.size - 1
    ocfg = orc.OracleConfig(num_dim=K, loss_type=cdae_amd.CROSS_ENTROPY, beta=1.0)
    o = orc.Oracle(ocfg, R, I_T, ptr, col)
    for which in (cdae_amd.P_W, cdae_amd.P_B, cdae_amd.P_BP):
        o.set(which, model.get(which).astype(np.float64))
    o.set(cdae_amd.P_WU, gathered(model.get(cdae_amd.P_WU), uids, 0.0).astype(np.float64))
    tw = twin_of(model, ptr, col, uids)
    z = tw.get_hidden_values(np.arange(R, dtype=np.uint32), mode=0)       # the fp32 z a handle encodes from those sets
    tw.close()
    D = model.get(cdae_amd.P_W).astype(np.float64)
    bp = model.get(cdae_amd.P_BP).astype(np.float64)
    Kc = int(model.lib.cdae_hip_row_stride(model.h))
    eps = 2.0 * (Kc + 2) * 2.0 ** -24 * (np.abs(z.astype(np.float64)) @ np.abs(D).T + np.abs(bp)).max(axis=1)      # as assert_valid_topk derives it
    S64 = oracle_scores(o, R)
    for topk in (10, 24):
        ids, sc = model.recommend_rows(ptr, col, uids, topk, with_scores=True)
        ref, ref_sc = o.recommend(topk + 1, with_scores=True)             # (one more place: the gap below the list counts too)
        clear = _clear_rows(ref_sc)
        assert clear.mean() > 0.8
        np.testing.assert_array_equal(ids[clear], ref[clear, :topk])
        assert_valid_topk(model, d, ids, topk, K, eps="derived", users=np.arange(R), rated=rows_of(ptr, col), Z=z)
        want_sc = np.take_along_axis(S64, ids.astype(np.int64), axis=1)
        assert (np.abs(sc.astype(np.float64) - want_sc) <= eps[:, None]).all(), np.abs(sc - want_sc).max()
        assert (np.diff(sc, axis=1) <= 0).all()
        rets, hits, ids2 = model.eval_topn_rows(ptr, col, tptr, tcol, uids, topk, with_ids=True)
        np.testing.assert_array_equal(ids2, ids)
        want = orc.eval_topn(ids, tptr, tcol)
        assert np.array_equal(rets.view(np.uint64), want.view(np.uint64)), (rets, want)
        rets2, hits2 = model.eval_topn_rows(ptr, col, tptr, tcol, uids, topk)
        assert np.array_equal(rets2.view(np.uint64), want.view(np.uint64)) and np.array_equal(hits, hits2)
        inside = [np.isin(ids[r, :20], tcol[tptr[r]:tptr[r + 1]]) for r in range(R)]
        np.testing.assert_array_equal(hits, np.array([sum(m[:n].sum() for m in inside) for n in (1, 5, 10)], dtype=np.uint64))


def oracle_scores(o, R):
    """the oracle's fp64 scores of all items for its rows: z from its own encode, D and b' its parameters"""
    K = o.K
    z = o.encode(0, 0, 0, np.arange(R, dtype=np.uint32)).reshape(R, K)
    return z @ o.get(cdae_amd.P_W).reshape(-1, K).T + o.get(cdae_amd.P_BP)


# ---- 5. chunk boundary ------------------------------------------------------------------------------------------------------------
def test_rows_beyond_one_chunk(built):
    U, I, K, R = 129, 96, 8, EVAL_CHUNK + 129
    rng = np.random.default_rng(55)
    train = [np.sort(rng.choice(I, int(rng.integers(1, 6)), replace=False)).astype(np.uint32) for _ in range(U)]
    tp, tc = csr(train)
    d = synth.Interactions(U, I, tp, tc, np.zeros(U + 1, np.int64), np.empty(0, np.uint32))
    model = cdae_model(d, K, False)
    p = int_model("random", U, I, K, False, seed=5)
    load(model, p)
    lens = rng.integers(0, 6, R)
    flat = np.argsort(rng.random((R, I)), axis=1)[:, :5].astype(np.uint32)
    rows = [np.sort(flat[r, :lens[r]]) for r in range(R)]
    ptr, col = csr(rows)
    uids = draw_uids(rng, U, R)
    want, want_sc = expected_rows(p, ptr, col, uids, 17)
    ids, sc = model.recommend_rows(ptr, col, uids, 16, with_scores=True)          # matrix cores: two launch groups
    np.testing.assert_array_equal(ids, want[:, :16])
    np.testing.assert_array_equal(sc, want_sc[:, :16])
    ids, sc = model.recommend_rows(ptr, col, uids, 17, with_scores=True)          # general path
    np.testing.assert_array_equal(ids, want)
    np.testing.assert_array_equal(sc, want_sc)


# ---- 6. more than 65 536 items ------------------------------------------------------------------------------------------------------
def test_rows_over_more_than_65536_items(built):
    """global-memory bit rows (rated_bits_kernel) and the global score workspace (recommend_kernel), as in test_more_than_65536_items"""
    U, I, K, R = 40, 70_050, 8, 40
    assert (I + 31) // 32 > 2048 and I * 4 + 64 > 160 * 1024
    d = make_data(U, I, seed=K, which=("tiles", "lowest"))
    model = cdae_model(d, K, False)
    rng = np.random.default_rng(6)
    rows = list(special_rows(rng, I, ("tiles", "half1", "lowest", "leaves7", "leaves24")).values()) + [np.empty(0, np.uint32)]
    rows += [np.sort(rng.choice(I, size=int(rng.integers(1, 41)), replace=False)).astype(np.uint32) for _ in range(R - len(rows))]
    ptr, col = csr(rows)
    uids = draw_uids(rng, U, R)
    for mode in ("random", "last"):
        p = int_model(mode, U, I, K, False, seed=K + 1, wmax=1)
        load(model, p)
        want, want_sc = expected_rows(p, ptr, col, uids, 17)
        for topk in (10, 17):
            ids, sc = model.recommend_rows(ptr, col, uids, topk, with_scores=True)
            np.testing.assert_array_equal(ids, want[:, :topk], err_msg=f"{mode} topk {topk}")
            np.testing.assert_array_equal(sc, want_sc[:, :topk])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(built):
    U, I, K, R = 129, 977, 61, 301
    d = make_data(U, I, seed=K)
    model = cdae_model(d, K, False)
    p = int_model("random", U, I, K, False, seed=K + I)
    load(model, p)
    rng = np.random.default_rng(7)
    ptr, col = csr(foreign_int_rows(rng, I, R))
    uids = draw_uids(rng, U, R)
    want, _ = expected_rows(p, ptr, col, uids, 17)
    big = int(np.argmax(np.diff(ptr) >= 2))                                      # a row with at least two items
    a = int(ptr[big])

    def swapped():
        c = col.copy(); c[a], c[a + 1] = c[a + 1], c[a]
        return dict(col=c)

    def duplicate():
        c = col.copy(); c[a + 1] = c[a]
        return dict(col=c)

    def item_out_of_range():
        c = col.copy(); c[ptr[big + 1] - 1] = I
        return dict(col=c)

    def uid_out_of_range():
        u = uids.copy(); u[5] = U
        return dict(uids=u)
    bad = [(swapped(), f"row {big}"), (duplicate(), f"row {big}"), (item_out_of_range(), f"row {big}"), (uid_out_of_range(), "row 5"),
           (dict(topk=0), "topk"), (dict(topk=I + 1), "topk")]
    for kw, word in bad:
        args = dict(row_ptr=ptr, col=col, uids=uids, topk=10)
        args.update(kw)
        with pytest.raises(cdae_amd.CDAEError, match=word):
            model.recommend_rows(**args)
        with pytest.raises(cdae_amd.CDAEError, match=word):
            model.eval_topn_rows(args["row_ptr"], args["col"], ptr, col, args["uids"], args["topk"])
        for topk in (10, 17):
            np.testing.assert_array_equal(model.recommend_rows(ptr, col, uids, topk), want[:, :topk])
    # target sets: validated alike; no row with targets is an error
    with pytest.raises(cdae_amd.CDAEError, match="target"):
        model.eval_topn_rows(ptr, col, ptr, swapped()["col"], uids, 10)
    with pytest.raises(cdae_amd.CDAEError, match="target"):
        model.eval_topn_rows(ptr, col, np.zeros(R + 1, np.int64), np.empty(0, np.uint32), uids, 10)
    np.testing.assert_array_equal(model.recommend_rows(ptr, col, uids, 10), want[:, :10])
    # no rows: success, nothing touched
    assert model.recommend_rows(np.zeros(1, np.int64), np.empty(0, np.uint32), None, 10).shape == (0, 10)
    assert model.lib.cdae_hip_recommend_rows(model.h, 0, None, None, None, 10, None, None) == 0
    # an IMF / BPR handle; a handle without interactions
    mf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=8, batch_users=1))
    mf.reset(d, seed=1)
    with pytest.raises(cdae_amd.CDAEError, match="IMF / BPR"):
        mf.recommend_rows(ptr, col, None, 10)
    with pytest.raises(cdae_amd.CDAEError, match="IMF / BPR"):
        mf.eval_topn_rows(ptr, col, ptr, col, None, 10)
    np.testing.assert_array_equal(mf.recommend_all(10).shape, (U, 10))           # (still usable)
    fresh = cdae_amd.CDAE(model.cfg)
    with pytest.raises(cdae_amd.CDAEError, match="set_interactions"):
        fresh.recommend_rows(ptr, col, None, 10)
    fresh.reset(d, seed=1)
    load(fresh, p)
    np.testing.assert_array_equal(fresh.recommend_rows(ptr, col, uids, 10), want[:, :10])
    np.testing.assert_array_equal(model.recommend_rows(ptr, col, uids, 17), want)


# ---- 8. timing against the loop it replaces -----------------------------------------------------------------------------------------
def test_one_batched_call_is_faster_than_the_loop_of_recommend_user(built):
    """2 048 foreign rows on the trained K = 200 model: one recommend_rows call against 2 048 recommend_user calls (the only way to
    do this before: a host sort, an allocation, two synchronisations and three single-workgroup launches per user).  Wall clock
    after one warm-up of each; asserted only as "faster" (both times are printed and go to helpers.record_measured as rows_vs_user_loop)."""
    model, d = trained(200)
    R, topk = 2048, 10
    rng = np.random.default_rng(8)
    rows = [np.sort(rng.choice(I_T, int(rng.integers(1, 61)), replace=False)).astype(np.uint32) for _ in range(R)]
    ptr, col = csr(rows)
    uids = rng.integers(0, U_T, R).astype(np.uint32)

    def batched():
        return model.recommend_rows(ptr, col, uids, topk)

    def loop():
        return np.stack([model.recommend_user(int(uids[r]), rows[r], topk) for r in range(R)])
    batched(); loop()
    t0 = time.perf_counter(); got = batched(); t1 = time.perf_counter(); one = loop(); t2 = time.perf_counter()
    record_measured("rows_vs_user_loop", rows=R, batched_s=t1 - t0, loop_s=t2 - t1)
    print(f"recommend_rows {1e3 * (t1 - t0):.3f} ms, {R} x recommend_user {1e3 * (t2 - t1):.3f} ms")
    assert t1 - t0 < t2 - t1
    _, sc = model.recommend_rows(ptr, col, uids, topk + 1, with_scores=True)      # (one more place: the gap below the list counts too)
    clear = _clear_rows(sc)
    assert clear.mean() > 0.8
    np.testing.assert_array_equal(got[clear], one[clear])
