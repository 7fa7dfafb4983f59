"""-m gpu: FISMauc training (cdae_hip_create_fism_pair, cdae_fism_pair_kernels.hpp) against tests/fism_pair_ref.py, the fp64 restatement of
the pair loop, over two epochs: the five tables (P, Q, their accumulators, bi) within 2e-4 of the reference in fism_ref's measure.  The
trajectory takes no decision, so the device and the reference run free; that the trajectories are well conditioned is
tests/test_fism_pair_reference.py's assertion, as is that the fixtures tell a stale Q[i], a stale repeated Q[j] and P[i] left in v apart.

Cases (fism_pair_ref.CASES): both edges of every NI tier with AdaGrad; plain SGD at one K per tier; LOG; no bias terms; alpha 0 / 0.5 / 1;
num_neg 1, 12 (a negative repeats inside a positive), 64, 65; rows of 1 and 2 items, rows of 11 of 12 items, users without items; the
residency seams at K 64 / 256 / 512; more pairs than one launch window.  Bit equality: both residency settings on every seam and gaps
case, two runs, one range against two adjacent ranges and against single users.  stats; user_id_offset; serving on small-integer tables
at one K per tier, exactly; recommend_all after training; the refusals of a FISM handle and CDAE_P_UB.
"""
import numpy as np
import pytest

import cdae_amd
import filtered_ref
import fism_pair_ref as pr
import full_rank_ref
import oracle as orc
import score_rows_ref
import similar_ref
import test_gpu_fism_serving as sv
from helpers import SENTINEL, rank_total_order

pytestmark = pytest.mark.gpu

TABLES = (("P", cdae_amd.P_W), ("Pa", cdae_amd.P_W_AG), ("Q", cdae_amd.P_V), ("Qa", cdae_amd.P_V_AG), ("bi", cdae_amd.P_BP))
ALL6 = TABLES + (("bia", cdae_amd.P_BP_AG),)
SEAMS = ("seam64", "seam256", "seam512")
GAPS = ("gaps-K24", "gaps-K200")


def config(K, num_neg, hyper):
    return cdae_amd.FISMPConfig(num_dim=K, num_neg=num_neg, lt=hyper.get("loss", cdae_amd.SQUARE), using_adagrad=hyper.get("adagrad", True),
                                using_bias_term=hyper.get("bias", True), learn_rate=hyper.get("learn_rate", 0.1),
                                lambda_=hyper.get("lambda_", 0.01), alpha=hyper.get("alpha", 1.0))


def make(case):
    name, ds, K, num_neg, hyper, sseed = case
    d = pr.fixture_data(ds)
    m = cdae_amd.FISMP(config(K, num_neg, hyper))
    m.reset(d, seed=pr.PSEED)
    return d, m


def tables(m, which=TABLES):
    return {n: m.get(w) for n, w in which}


def train(m, case, ranges=None, resident=True):
    """the case's epochs from the state the handle is in -> (tables, stats of the last call)"""
    m.set_resident(resident)
    st = None
    for ep in range(pr.EPOCHS):
        if ranges is None:
            st = m.train_one_iteration(case[5], ep)
        else:
            for a, b in ranges:
                st = m.train_users(case[5], ep, a, b)
    return tables(m, ALL6), st


def assert_same_bits(a, b, what):
    for n in a:
        np.testing.assert_array_equal(a[n].view(np.uint32), b[n].view(np.uint32), err_msg=f"{what}: {n}")


def test_init_params_is_the_references_start_and_there_is_no_user_bias():
    c = pr.case("d40-K65")
    d, m = make(c)
    st = pr.new_state(c)
    for n, w in TABLES:
        np.testing.assert_array_equal(m.get(w), getattr(st, n).astype(np.float32), err_msg=n)
    np.testing.assert_array_equal(m.get(cdae_amd.P_BP_AG), np.full(d.num_items, 1e-4, np.float32))
    for which in (cdae_amd.P_UB, cdae_amd.P_UB_AG, cdae_amd.P_WU, cdae_amd.P_WU_AG, cdae_amd.P_UU, cdae_amd.P_B):
        with pytest.raises(cdae_amd.CDAEError, match="not allocated"):
            m.get(which)
    with pytest.raises(cdae_amd.CDAEError, match="not allocated"):
        m.set(cdae_amd.P_UB, np.zeros(d.num_users, np.float32))


@pytest.mark.parametrize("name", [c[0] for c in pr.CASES])
def test_two_epochs_match_the_reference(name):
    c = pr.case(name)
    d, m = make(c)
    if name.startswith("seam"):
        lens = np.diff(d.train_ptr)
        C, W = m.plan()["resident_rows"], pr.WAVES
        assert C == pr.resident_rows(c[2]) and sorted(lens.tolist()) == sorted((1, 2, W - 1, W, W + 1, C - 1, C, C + 1, 2 * C + 1))
    got, stats = train(m, c)
    nnz = int(d.train_ptr[-1])
    assert (stats.users, stats.examples) == (d.num_users, nnz * c[3])
    ref = pr.reference(name)
    errs = {n: pr.measure(got[n], getattr(ref, n)) for n, _ in TABLES}
    print(f"{name}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert max(errs.values()) <= pr.BOUND, errs
    if not c[4].get("bias", True):
        assert not got["bi"].any()


@pytest.mark.parametrize("name", SEAMS + GAPS)
def test_both_residency_settings_give_the_same_bits(name):
    c = pr.case(name)
    d, m = make(c)
    assert m.plan()["resident_rows"] > 0
    a, _ = train(m, c, resident=True)
    m.init_params(pr.PSEED)
    m.set_resident(False)
    assert m.plan()["resident_rows"] == 0
    b, _ = train(m, c, resident=False)
    assert_same_bits(a, b, name)
    m.init_params(pr.PSEED)                                   # ... and a second run leaves the same bits again
    a2, _ = train(m, c, resident=True)
    assert_same_bits(a, a2, name + " repeated")


def test_one_range_two_adjacent_ranges_and_single_users_give_the_same_bits():
    c = pr.case("d40-K65")
    d, m = make(c)
    a, st = train(m, c)
    assert st.batches == 1                                    # D40's 705 pairs: one launch window
    m.init_params(pr.PSEED)
    b, _ = train(m, c, ranges=((0, 3), (3, d.num_users)))
    assert_same_bits(a, b, "two ranges")
    m.init_params(pr.PSEED)
    b, st = train(m, c, ranges=[(u, u + 1) for u in range(d.num_users)])
    assert (st.batches, st.users) == (1, 1)
    assert_same_bits(a, b, "user by user")


def test_a_window_boundary_inside_the_range_gives_the_same_bits():
    c = pr.case("win")
    d, m = make(c)
    pairs = int(d.train_ptr[-1]) * c[3]
    assert pairs > m.plan()["window_instances"] == pr.WINDOW_INSTANCES
    a, st = train(m, c)
    assert (st.batches, st.users, st.examples) == (2, d.num_users, pairs)
    m.init_params(pr.PSEED)
    b, st = train(m, c, ranges=[(u, u + 1) for u in range(d.num_users)])
    assert (st.batches, st.users) == (1, 1)
    assert_same_bits(a, b, "user by user")
    m.init_params(pr.PSEED)
    b, _ = train(m, c, ranges=((0, 5), (5, d.num_users)))
    assert_same_bits(a, b, "two ranges")


def test_a_sub_range_trains_its_users_only():
    c = pr.case("d40-K65")
    d, m = make(c)
    st = m.train_users(c[5], 0, 2, 5)
    ref = pr.new_state(c)
    n = pr.train(ref, d.train_ptr, d.train_col, c[5], 0, users=(2, 5))
    got = tables(m)
    assert n == int(d.train_ptr[5] - d.train_ptr[2]) * 5 == st.examples and st.users == 3
    assert max(pr.measure(got[k], getattr(ref, k)) for k, _ in TABLES) <= pr.BOUND


@pytest.mark.parametrize("name", GAPS)
def test_users_without_train_items_move_no_bit_and_are_counted(name):
    c = pr.case(name)
    d, m = make(c)
    lens = np.diff(d.train_ptr)
    empty, U = lens == 0, d.num_users
    start = tables(m, ALL6)
    pair = next(u for u in range(U - 1) if empty[u] and empty[u + 1])
    st = m.train_users(c[5], 0, pair, pair + 2)               # a range of empty users alone: a launch that holds no pair
    assert (st.users, st.examples, st.batches) == (2, 0, 1)
    assert_same_bits(start, tables(m, ALL6), "two empty users")
    a, st = train(m, c)
    assert (st.users, st.examples) == (U, int(d.train_ptr[-1]) * c[3])
    m.init_params(pr.PSEED)
    b, _ = train(m, c, ranges=[(u, u + 1) for u in range(U)])
    assert_same_bits(a, b, "user by user")


def test_the_user_id_offset_keys_the_negatives():
    """X: D40 with user_id_offset 3.  Y: three empty users, then D40's rows, offset 0.  User u of X draws what user u + 3 of Y draws, so
    from the same P and Q both end with the same bits; without the offset D40 draws other negatives."""
    c = pr.case("d40-K65")
    d = pr.fixture_data(c[1])
    U, I = d.num_users, d.num_items

    def handle(ptr, users, offset):
        m = cdae_amd.FISMP(config(c[2], c[3], c[4]))
        m.set_interactions(users, I, ptr, d.train_col, user_id_offset=offset)
        m.init_params(pr.PSEED)
        return m

    x = handle(d.train_ptr, U, 3)
    y = handle(np.r_[0, 0, 0, d.train_ptr], U + 3, 0)
    z = handle(d.train_ptr, U, 0)
    for w in (cdae_amd.P_W, cdae_amd.P_V):
        y.set(w, x.get(w))
        z.set(w, x.get(w))
    gx, gy, gz = (train(m, c)[0] for m in (x, y, z))
    assert_same_bits(gx, gy, "offset 3 against three users in front")
    assert (gx["Q"].view(np.uint32) != gz["Q"].view(np.uint32)).any()          # the offset is read


def test_enqueue_users_and_collect_stats_are_train_users():
    c = pr.case("d40-K65")
    d, m = make(c)
    ranges = ((0, 3), (3, d.num_users))
    want = np.zeros(3, dtype=np.int64)
    for ep in range(pr.EPOCHS):
        for a, b in ranges:
            st = m.train_users(c[5], ep, a, b)
            want += (st.users, st.examples, st.batches)
    a = tables(m, ALL6)
    assert tuple(want) == (pr.EPOCHS * d.num_users, pr.EPOCHS * int(d.train_ptr[-1]) * c[3], pr.EPOCHS * 2)
    m.init_params(pr.PSEED)
    for ep in range(pr.EPOCHS):
        for u0, u1 in ranges:
            m.enqueue_users(c[5], ep, u0, u1)
    st = m.collect_stats()
    assert (st.users, st.examples, st.batches) == tuple(want)
    assert_same_bits(a, tables(m, ALL6), "enqueue_users")


def test_a_pair_handle_and_a_fism_handle_differ_only_in_the_loop():
    """from the same start the two handles train to different tables, and the FISM handle still steps bu"""
    c = pr.case("d40-K65")
    d, m = make(c)
    f = cdae_amd.FISM(cdae_amd.FISMConfig(**vars(config(c[2], c[3], c[4]))))
    f.reset(d, seed=pr.PSEED)
    for n, w in TABLES:
        np.testing.assert_array_equal(f.get(w), m.get(w), err_msg=n)
    sp, sf = m.train_one_iteration(c[5], 0), f.train_one_iteration(c[5], 0)
    assert sf.examples - sp.examples == int(d.train_ptr[-1])
    assert (f.get(cdae_amd.P_V) != m.get(cdae_amd.P_V)).any() and f.get(cdae_amd.P_UB).all()


# ---- serving: a FISM handle's, exactly, on small-integer tables (tests/test_gpu_fism_serving.py chooses them) ---------------------------
def served_model(K, alpha, d, t):
    m = cdae_amd.FISMP(cdae_amd.FISMPConfig(num_dim=K, alpha=alpha))
    m.reset(d, seed=1)
    m.set(cdae_amd.P_W, t["P"]); m.set(cdae_amd.P_V, t["Q"]); m.set(cdae_amd.P_BP, t["bi"])
    return m


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("K", (64, 128, 256, 512))
def test_every_served_entry_point_is_exact(K, alpha):
    U, I = 23, sv.I
    d = sv.make_data(alpha, U, seed=K)
    t = sv.int_tables(K, U, seed=K + 1)
    m = served_model(K, alpha, d, t)
    rng = np.random.default_rng(K + 2)
    rows = sv.caller_rows(alpha, d, seed=K + 3)
    R = len(rows)
    ptr, col = filtered_ref.csr(rows)
    Sr = sv.expected_scores(t, alpha, rows)
    # recommend_rows
    wi, ws = filtered_ref.filtered_topk(Sr, rows, None, None, True, 10)
    gi, gs = m.recommend_rows(ptr, col, topk=10, with_scores=True)
    np.testing.assert_array_equal(gi, wi)
    np.testing.assert_array_equal(gs, ws)
    # eval_topn_rows
    rt = [np.setdiff1d(np.unique(np.r_[wi[r][:2][wi[r][:2] != SENTINEL], rng.integers(0, I, 3)]), rows[r]).astype(np.uint32) if r % 2 else
          np.empty(0, np.uint32) for r in range(R)]
    rtp, rtc = filtered_ref.csr(rt)
    rets, hits, ids = m.eval_topn_rows(ptr, col, rtp, rtc, topk=10, with_ids=True)
    np.testing.assert_array_equal(ids, wi)
    full = np.full((R, 10), SENTINEL, dtype=np.uint32)
    full[:] = wi
    assert rets.tobytes() == orc.eval_topn(full, rtp, rtc).tobytes()
    # score_rows
    cands = [np.unique(np.r_[rng.integers(0, I, 20), rows[r][:3]]).astype(np.uint32) for r in range(R)]
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
    # recommend_rows_filtered
    excl = [np.sort(rng.choice(I, 15, replace=False)).astype(np.uint32) for _ in range(R)]
    allow = np.sort(rng.choice(I, 120, replace=False)).astype(np.uint32)
    wi, ws = filtered_ref.filtered_topk(Sr, rows, excl, allow, False, 12)
    gi, gs = m.recommend_rows_filtered(ptr, col, topk=12, with_scores=True, exclude=filtered_ref.csr(excl), allow=allow, exclude_rated=False)
    np.testing.assert_array_equal(gi, wi)
    np.testing.assert_array_equal(gs, ws)
    # similar_items over P and Q
    queries = np.r_[0, I - 1, rng.integers(0, I, 20)].astype(np.uint32)
    for table, T in (("input", t["P"]), ("output", t["Q"])):
        similar_ref.assert_exact_products(T, 1.0)
        wi, ws = similar_ref.similar_topk(T, queries, "dot", True, None, None, 10)
        gi, gs = m.similar_items(queries, topk=10, metric="dot", table=table, with_scores=True)
        np.testing.assert_array_equal(gi, wi, err_msg=table)
        np.testing.assert_array_equal(gs, ws, err_msg=table)
    # the train rows
    S = sv.expected_scores(t, alpha, sv.rows_of(d))
    np.testing.assert_array_equal(m.recommend_all(10), rank_total_order(S, d.train_ptr, d.train_col, 10))


def test_recommend_all_after_training_ranks_the_trained_tables():
    c = pr.case("d40-K65")
    d, m = make(c)
    got, _ = train(m, c)
    rec = m.recommend_all(5)
    ref = pr.State(got["P"], got["Q"], d.num_users, alpha=c[4]["alpha"])
    ref.bi = got["bi"].astype(np.float64)
    clear = 0
    for u in range(d.num_users):
        row = d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]
        s = ref.Q @ pr.hidden(ref, row) + ref.bi
        s[row] = -np.inf
        order = np.argsort(-s, kind="stable")
        assert not np.isin(rec[u], row).any() and np.unique(rec[u]).size == 5
        if np.abs(np.diff(s[order[:6]])).min() > 1e-4 * np.abs(s[np.isfinite(s)]).max():   # where the scores are clearly apart the lists agree
            np.testing.assert_array_equal(rec[u], order[:5])
            clear += 1
    assert clear >= d.num_users // 2


def test_refusals_of_a_pair_handle():
    d = sv.make_data(0.0, 9, seed=3)
    m = served_model(24, 0.0, d, sv.int_tables(24, 9, seed=4))
    lib, h = m.lib, m.h
    I = sv.I
    ptr, col = filtered_ref.csr(sv.rows_of(d)[:2])

    def refused(call, *words):
        with pytest.raises(cdae_amd.CDAEError) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)

    before = {w: m.get(w) for w in (cdae_amd.P_W, cdae_amd.P_V, cdae_amd.P_BP)}
    refused(lambda: m.get(cdae_amd.P_UB), "not allocated")
    refused(lambda: m.get(cdae_amd.P_UB_AG), "not allocated")
    refused(lambda: m.set(cdae_amd.P_UB, np.zeros(9, np.float32)), "not allocated")
    refused(lambda: m.debug_sample_batch(1, 0, 0, 1), "FISM", "no example list")
    refused(lambda: m.debug_row_pack(1, 0, 0, 1), "FISM", "no example list")
    refused(lambda: m.get_hidden_values([0, 1]), "FISM", "no user node")
    refused(lambda: m.train_one_user_corruption(0, [int(d.train_col[0])], [int(np.setdiff1d(np.arange(I), sv.rows_of(d)[0])[0])]), "FISM", "no example list")
    refused(lambda: m.fold_in_rows(ptr, col), "FISM", "nothing to fit")
    refused(lambda: m.recommend_user(0, sv.rows_of(d)[0], 5), "FISM", "cdae_hip_recommend_rows")
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
    assert cdae_amd.FISMP(cdae_amd.FISMPConfig(num_dim=24)).plan()["resident_rows"] == 0             # before set_interactions
    refused(lambda: cdae_amd.FISMP(cdae_amd.FISMPConfig(lt=cdae_amd.CROSS_ENTROPY)), "CROSS_ENTROPY", "LOG's")
