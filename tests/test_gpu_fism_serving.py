"""-m gpu: a FISM handle served exactly — no training.  P, Q and bi are written through set_param as integers such that every hidden row
z = n^-alpha * (sum of the rated rows of P) is integer-valued and every score z . Q[j] + bi[j] is exact in fp32 in any summation order
(helpers.assert_fp32_exact, the condition tests/test_gpu_rank_exact.py relies on): alpha = 0 with rated sets of any size, alpha = 1 with
sets of 2, 4, 8, 16 items and P in multiples of 16.  Every list, score, rank and TOPN figure must then equal the numpy rules of the
existing reference helpers (helpers.rank_total_order, filtered_ref, score_rows_ref, full_rank_ref, similar_ref, oracle.eval_topn) bit for
bit.  bu is set to non-zero values and must not show in any served score.  One test holds the refusals of a FISM handle, one the train
rows without items that a FISM handle accepts.
"""
import numpy as np
import pytest

import cdae_amd
import oracle as orc
import filtered_ref
import full_rank_ref
import score_rows_ref
import similar_ref
from cdae_amd import synth
from helpers import SENTINEL, assert_fp32_exact, exact_scores, rank_total_order

pytestmark = pytest.mark.gpu

I = 301
KS = (1, 64, 65, 256, 257, 512)
ENC_GROUP = 8                    # FISM_ENC_GROUP (cdae_fism_kernels.hpp): rows of 16 and more items take several groups


def sizes_for(alpha, n, rng):
    return rng.choice([2, 4, 8, 16], n) if alpha else rng.integers(1, 46, n)


def make_data(alpha, U, seed):
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(I, int(s), replace=False)).astype(np.uint32) for s in sizes_for(alpha, U, rng)]
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    return synth.Interactions(U, I, ptr, np.concatenate(rows), np.zeros(U + 1, np.int64), np.empty(0, np.uint32))


def caller_rows(alpha, d, seed):
    """rated sets that are not train rows: an empty one, a long one (several encode groups), sets of every legal size, one train row"""
    rng = np.random.default_rng(seed)
    sizes = [0, 16, 2, 4, 8, 16, 0, 2] if alpha else [0, 45, 1, 2, ENC_GROUP - 1, ENC_GROUP, ENC_GROUP + 1, 3 * ENC_GROUP + 5, 0, 120]
    rows = [np.sort(rng.choice(I, s, replace=False)).astype(np.uint32) for s in sizes]
    rows.append(d.train_col[d.train_ptr[1]:d.train_ptr[2]].astype(np.uint32))
    train = {tuple(d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]) for u in range(d.num_users)}
    assert sum(tuple(r) not in train for r in rows) >= len(rows) - 1 and max(r.size for r in rows) > ENC_GROUP
    return rows


def int_tables(K, U, seed):
    rng = np.random.default_rng(seed)
    return dict(P=16.0 * rng.integers(-2, 3, (I, K)), Q=rng.integers(-2, 3, (I, K)).astype(np.float64), bi=rng.integers(-4, 5, I).astype(np.float64),
                bu=rng.integers(1, 9, U).astype(np.float64))


def model(K, alpha, d, t):
    m = cdae_amd.FISM(cdae_amd.FISMConfig(num_dim=K, alpha=alpha))
    m.reset(d, seed=1)
    m.set(cdae_amd.P_W, t["P"]); m.set(cdae_amd.P_V, t["Q"]); m.set(cdae_amd.P_BP, t["bi"]); m.set(cdae_amd.P_UB, t["bu"])
    return m


def expected_scores(t, alpha, rows):
    """-> S int64 [rows, I]: the exact scores; asserts that z is integer-valued and that fp32 holds every partial sum"""
    z = np.stack([(t["P"][r.astype(np.int64)].sum(axis=0) / (float(r.size) ** alpha if r.size else 1.0)) for r in rows])
    Z, S, D, bq = exact_scores(None, None, uv=z, iv=t["Q"], ib=t["bi"])
    assert_fp32_exact(Z, D, bq)
    mag = np.stack([np.abs(t["P"][r.astype(np.int64)]).sum(axis=0) for r in rows])
    assert mag.max() < 2 ** 24                           # the sum itself is exact in any order too
    return S


def rows_of(d):
    return [d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]] for u in range(d.num_users)]


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("K", KS)
def test_every_served_entry_point_is_exact(K, alpha):
    U = 37
    d = make_data(alpha, U, seed=K)
    t = int_tables(K, U, seed=K + 1)
    m = model(K, alpha, d, t)
    rng = np.random.default_rng(K + 2)
    # the train rows: recommend_all (both sweeps: topk 10 on the matrix cores where K <= 256, 17 on the general path), eval_topn
    S = expected_scores(t, alpha, rows_of(d))
    want = rank_total_order(S, d.train_ptr, d.train_col, 17)
    for topk in (10, 17):
        np.testing.assert_array_equal(m.recommend_all(topk), want[:, :topk], err_msg=f"recommend_all topk {topk}")
    np.testing.assert_array_equal(m.recommend_all(10, 3, U - 2), want[3:U - 2, :10])
    targets = [np.unique(np.r_[want[u][:3][want[u][:3] != SENTINEL], rng.integers(0, I, 2)]).astype(np.uint32) if u % 3 else np.empty(0, np.uint32)
               for u in range(U)]
    targets = [np.setdiff1d(tg, r).astype(np.uint32) for tg, r in zip(targets, rows_of(d))]
    tp, tc = filtered_ref.csr(targets)
    m.set_test_rows(tp, tc)
    rets, hits, ids = m.eval_topn(10, with_ids=True)
    np.testing.assert_array_equal(ids, want[:, :10])
    assert rets.tobytes() == orc.eval_topn(want[:, :10], tp, tc).tobytes() and hits[2] > 0
    # caller-supplied rated sets
    rows = caller_rows(alpha, d, seed=K + 3)
    R = len(rows)
    ptr, col = filtered_ref.csr(rows)
    Sr = expected_scores(t, alpha, rows)
    np.testing.assert_array_equal(Sr[0], t["bi"].astype(np.int64))          # the empty set: z = 0, the scores are bi
    uids = rng.integers(0, U, R).astype(np.uint32)
    uids[::3] = cdae_amd.NO_USER
    for topk in (10, 17):
        wi, ws = filtered_ref.filtered_topk(Sr, rows, None, None, True, topk)
        for u in (None, uids):                           # uids are validated and not otherwise read
            gi, gs = m.recommend_rows(ptr, col, uids=u, topk=topk, with_scores=True)
            np.testing.assert_array_equal(gi, wi)
            np.testing.assert_array_equal(gs, ws)
    wi10 = filtered_ref.filtered_topk(Sr, rows, None, None, True, 10)[0]
    rt = [np.setdiff1d(np.unique(np.r_[wi10[r][:2][wi10[r][:2] != SENTINEL], rng.integers(0, I, 3)]), rows[r]).astype(np.uint32) if r % 2 else
          np.empty(0, np.uint32) for r in range(R)]
    rtp, rtc = filtered_ref.csr(rt)
    rets, hits, ids = m.eval_topn_rows(ptr, col, rtp, rtc, topk=10, with_ids=True)
    np.testing.assert_array_equal(ids, wi10)
    full = np.full((R, 10), SENTINEL, dtype=np.uint32)
    full[:] = wi10
    assert rets.tobytes() == orc.eval_topn(full, rtp, rtc).tobytes()
    # score_rows: candidates from anywhere, the row's own rated items included (scored from the full x)
    cands = [np.unique(np.r_[rng.integers(0, I, 20), rows[r][:3]]).astype(np.uint32) for r in range(R)]
    assert any(np.isin(c, r).any() for c, r in zip(cands, rows))
    cp, cc = filtered_ref.csr(cands)
    sc, rk = m.score_rows(ptr, col, cp, cc, with_ranks=True)
    want_sc = Sr[score_rows_ref.row_of_position(cp), cc.astype(np.int64)]
    np.testing.assert_array_equal(sc, want_sc.astype(np.float32))
    np.testing.assert_array_equal(rk, score_rows_ref.ranks_of(want_sc, cp, cc))
    # full_rank_rows
    tg = full_rank_ref.draw_targets(rng, rows, I, all_of=(1,))
    ftp, ftc = full_rank_ref.csr(tg)
    order = rank_total_order(Sr, None, None, I, rated=rows)
    fr, fs = m.full_rank_rows(ptr, col, ftp, ftc, with_scores=True)
    np.testing.assert_array_equal(fr, full_rank_ref.positions(order, ftp, ftc, I))
    np.testing.assert_array_equal(fs, Sr[np.repeat(np.arange(R), np.diff(ftp)), ftc.astype(np.int64)].astype(np.float32))
    # recommend_rows_filtered: an excl CSR, an allow list, rated items as candidates
    excl = [np.sort(rng.choice(I, 15, replace=False)).astype(np.uint32) for _ in range(R)]
    allow = np.sort(rng.choice(I, 120, replace=False)).astype(np.uint32)
    for kw_ref, kw in (((excl, None, True), dict(exclude=filtered_ref.csr(excl))), ((None, allow, True), dict(allow=allow)),
                       ((excl, allow, False), dict(exclude=filtered_ref.csr(excl), allow=allow, exclude_rated=False)),
                       ((None, None, False), dict(exclude_rated=False))):
        wi, ws = filtered_ref.filtered_topk(Sr, rows, kw_ref[0], kw_ref[1], kw_ref[2], 12)
        gi, gs = m.recommend_rows_filtered(ptr, col, topk=12, with_scores=True, **kw)
        np.testing.assert_array_equal(gi, wi, err_msg=str(kw.keys()))
        np.testing.assert_array_equal(gs, ws, err_msg=str(kw.keys()))


@pytest.mark.parametrize("K", (64, 257))
def test_train_rows_without_items_are_served_their_biases(K):
    """a FISM handle takes train rows without items (the first, the last, two in a row): z = 0, so recommend_all ranks bi alone for them
    and every other user's list is what it was"""
    U, alpha = 11, 0.0
    full = make_data(alpha, U, seed=K)
    rows = [r if u not in (0, 4, 5, U - 1) else r[:0] for u, r in enumerate(rows_of(full))]
    ptr, col = filtered_ref.csr(rows)
    d = synth.Interactions(U, I, ptr.astype(np.int64), col.astype(np.uint32), np.zeros(U + 1, np.int64), np.empty(0, np.uint32))
    t = int_tables(K, U, seed=K + 1)
    m = model(K, alpha, d, t)
    S = expected_scores(t, alpha, rows)
    np.testing.assert_array_equal(S[0], t["bi"].astype(np.int64))
    want = rank_total_order(S, d.train_ptr, d.train_col, 17)
    for topk in (10, 17):
        np.testing.assert_array_equal(m.recommend_all(topk), want[:, :topk], err_msg=f"recommend_all topk {topk}")


def pow2_table(K, seed, value):
    """rows of four entries +-value (one when K < 4): every norm is a power of two, every normalised entry +-0.5 (or +-1)"""
    rng = np.random.default_rng(seed)
    T = np.zeros((I, K))
    nz = min(K, 4)
    for i in range(I):
        T[i, rng.choice(K, nz, replace=False)] = value * rng.choice([-1.0, 1.0], nz)
    return T


@pytest.mark.parametrize("K", KS)
def test_similar_items_over_both_tables(K):
    d = make_data(0.0, 9, seed=K)
    t = int_tables(K, 9, seed=K + 1)
    m = model(K, 0.0, d, t)
    rng = np.random.default_rng(K)
    queries = np.r_[0, I - 1, rng.integers(0, I, 20)].astype(np.uint32)
    for table, T in (("input", t["P"]), ("output", t["Q"])):
        similar_ref.assert_exact_products(T, 1.0)
        wi, ws = similar_ref.similar_topk(T, queries, "dot", True, None, None, 10)
        gi, gs = m.similar_items(queries, topk=10, metric="dot", table=table, with_scores=True)
        np.testing.assert_array_equal(gi, wi, err_msg=table)
        np.testing.assert_array_equal(gs, ws, err_msg=table)
    c = dict(P=pow2_table(K, K + 5, 8.0), Q=pow2_table(K, K + 6, 1.0))
    m.set(cdae_amd.P_W, c["P"]); m.set(cdae_amd.P_V, c["Q"])
    for table, T in (("input", c["P"]), ("output", c["Q"])):
        similar_ref.assert_exact_products(similar_ref.normalise(T), 0.5)
        wi, ws = similar_ref.similar_topk(T, queries, "cosine", True, None, None, 10)
        gi, gs = m.similar_items(queries, topk=10, metric="cosine", table=table, with_scores=True)
        np.testing.assert_array_equal(gi, wi, err_msg=table)
        np.testing.assert_array_equal(gs, ws, err_msg=table)
    assert not np.array_equal(similar_ref.similar_topk(c["P"], queries, "cosine")[0], similar_ref.similar_topk(c["Q"], queries, "cosine")[0])


def test_refusals_of_a_fism_handle():
    d = make_data(0.0, 9, seed=3)
    m = model(24, 0.0, d, int_tables(24, 9, seed=4))
    lib, h = m.lib, m.h
    ptr, col = filtered_ref.csr(rows_of(d)[:2])

    def refused(call, *words):
        with pytest.raises(cdae_amd.CDAEError) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)

    before = {w: m.get(w) for w in (cdae_amd.P_W, cdae_amd.P_V, cdae_amd.P_BP, cdae_amd.P_UB)}
    refused(lambda: m.debug_sample_batch(1, 0, 0, 1), "FISM", "no example list")
    refused(lambda: m.debug_row_pack(1, 0, 0, 1), "FISM", "no example list")
    refused(lambda: m.get_hidden_values([0, 1]), "FISM", "no user node")
    refused(lambda: m.train_one_user_corruption(0, [int(d.train_col[0])], [int(np.setdiff1d(np.arange(I), rows_of(d)[0])[0])]), "FISM", "no example list")
    refused(lambda: m.fold_in_rows(ptr, col), "FISM", "nothing to fit")
    refused(lambda: m.recommend_user(0, rows_of(d)[0], 5), "FISM", "cdae_hip_recommend_rows")
    refused(m.delta_begin, "FISM", "delta")
    refused(lambda: m.exchange_configure(1), "FISM", "exchange")
    refused(lambda: cdae_amd.WRMF.half_step(m, 0), "WRMF handle")
    refused(lambda: cdae_amd.WARP.record_choices(m, True), "WARP handle")
    assert lib.cdae_hip_set_guest_nodes(h, 1, None, None, None, None) != 0
    for w, a in before.items():                           # refused before any launch: nothing moved
        np.testing.assert_array_equal(m.get(w), a)
    assert m.data_loss(1, 0) == 0.0 and m.penalty_loss() == 0.0
    m.prefetch_users(1, 0, 0, 3)                          # nothing to prepare: accepted, does nothing
    assert m.plan() == dict(resident_rows=256, window_instances=2048)
    fresh = cdae_amd.FISM(cdae_amd.FISMConfig(num_dim=24))
    assert fresh.plan()["resident_rows"] == 0             # before set_interactions
    refused(lambda: cdae_amd.FISM.plan(cdae_amd.MF(cdae_amd.MFConfig(num_dim=8))), "FISM handle")
