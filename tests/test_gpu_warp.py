"""-m gpu: WARP training (cdae_hip_create_warp, cdae_warp_kernels.hpp) against tests/warp_ref.py, the fp64 restatement of the loop
and of the block schedule, over two epochs.

A WARP trajectory branches on comparisons of scores, and an fp32 and an fp64 score may fall on different sides of a margin; one flipped
decision changes everything after it.  So the handle records its choices (record_choices) and after every epoch the reference FOLLOWS
them, verifying each one: every candidate before the chosen one has margin <= +tol, the chosen one > -tol, a skipped pair nothing above
+tol among its 499 candidates (tol = 1e-3; tests/test_warp_reference.py shows that next to no comparison falls into that band and that
the searches are of every depth).  Decisions that differ from the reference's own free decision are counted and capped at 1e-3 of the
comparisons — they are expected to be 0; the cap only keeps the band from hiding a broken search.  The parameters must then agree within
tests/test_gpu_mf.py's bound: 2e-4 of the parameter's range (the same arithmetic — fp32 storage, 1-ulp rcp / sqrt — against fp64).

Cases (warp_ref.CASES): the loop on D40 at both edges of every K tier with the defaults (from K = 128 on the accumulators start at 3, 5, 10
and not at 1e-4, so that |score| stays below 16: warp_ref.CASES has the reasoning); at K = 200 with plain SGD, LOG loss, num_neg 1
and 12; the loop on "tiny" (300 users: two launch windows); blocks of 8 on D40; blocks of 33 on "tiny" at K = 24, 200 and 300 (a partial
last block, the activity-grouped order of user_order()).

The pinning pass added: item biases that start uniform in +-0.5 (and random user biases) on the loop at K = 65 and 200 and on blocks of 8
and 33 — every other case starts all biases at 0, where a wrong bias pointer or a bias left out of yui moves no bit; D40 with two dense
users (one and two items left: rank weights l[0], l[1], l[2]); block handles whose last block holds ONE user (nine users in blocks of 8,
"tiny" in blocks of 299): that block runs the in-place kernel.  Biases and their accumulators keep their bits in every case.  Exactly,
bit for bit and in the recorded choices: P_UB zero against random; one call against two ranges, single users, ranges around the
256-user launch window, enqueue_users + collect_stats (and the stats of each); a block handle's ranges cut between blocks; a handle
with user_id_offset 3 against one with three users in front.  tests/test_warp_reference.py shows on the CPU that the 2e-4 bound would
notice each of nine ways to write the loop wrong.

The saturation pass added the losses that had never run in warp_user_kernel — SQUARE and CROSS_ENTROPY on the loop and on blocks of 8
(D40, K = 24, the defaults) — and five cases whose item biases start uniform in +-100 (d40-loop-bias100-*: SQUARE, LOGISTIC, LOG, HINGE,
CROSS_ENTROPY at learn rate 0.03).  Biases take no step, so those scores stay near +-100 and yui - score, what mf_loss_grad sees, goes
down to -200: three quarters of the trained pairs lie below -18 and a sixth below -88.5, where __expf has overflowed, and SQUARE steps
on gradients of 400 (tests/test_warp_reference.py asserts and prints the shares).  The method, tol, the cap and the 2e-4 bound are the
same.  LOGISTIC has no other case: g = -1 / d near d = 0 cannot be pinned from small biases (warp_ref.CASES).
"""
import numpy as np
import pytest

import cdae_amd
import warp_ref as wr
from helpers import record_measured

pytestmark = pytest.mark.gpu

TABLES = (("uv", cdae_amd.P_WU), ("uva", cdae_amd.P_WU_AG), ("iv", cdae_amd.P_W), ("iva", cdae_amd.P_W_AG))
USER_INDEXED = {cdae_amd.P_WU, cdae_amd.P_WU_AG}


def config(K, num_neg, B, hyper):
    return cdae_amd.WARPConfig(num_dim=K, num_neg=num_neg, batch_users=B, lt=hyper.get("loss", cdae_amd.HINGE),
                               using_adagrad=hyper.get("adagrad", True), learn_rate=hyper.get("learn_rate", 0.1), lambda_=hyper.get("lambda_", 0.1))


def by_position(m, which, order):
    a = m.get(which).astype(np.float64)
    return a[order] if which in USER_INDEXED else a


def in_training_order(d, order):
    lens = np.diff(d.train_ptr)[order]
    ptr = np.r_[0, np.cumsum(lens)].astype(np.int64)
    col = np.concatenate([d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]] for u in order]).astype(np.uint32)
    return ptr, col


def user_bias_start(case, d):
    """the P_UB a case starts from: random where the case's item biases are (ub is part of no score and of no step)"""
    return wr.bias_start(case[5].get("ib0"), d.num_users, salt=1)


def make(case, ub=None):
    name, ds, B, K, num_neg, hyper, pseed, sseed = case
    d = wr.fixture_data(ds)
    m = cdae_amd.WARP(config(K, num_neg, B, hyper))
    m.reset(d, seed=pseed)
    if hyper.get("acc0"):                                                  # a fixture that starts its accumulators elsewhere (warp_ref.CASES)
        m.set(cdae_amd.P_WU_AG, np.full((d.num_users, K), hyper["acc0"], dtype=np.float32))
        m.set(cdae_amd.P_W_AG, np.full((d.num_items, K), hyper["acc0"], dtype=np.float32))
    assert not m.get(cdae_amd.P_BP).any() and not m.get(cdae_amd.P_UB).any()        # init_params' biases
    ib0, ub0 = wr.bias_start(hyper.get("ib0"), d.num_items), user_bias_start(case, d) if ub is None else ub
    if hyper.get("ib0"):                                                   # ... and its item biases
        assert np.abs(ib0).max() > 0.4 and np.abs(ub0).max() > 0.4
        m.set(cdae_amd.P_BP, ib0)
    if ub0.any():
        m.set(cdae_amd.P_UB, ub0)
    order = m.user_order().astype(np.int64)
    assert sorted(order.tolist()) == list(range(d.num_users))
    np.testing.assert_array_equal(order, wr.user_order(np.diff(d.train_ptr), B))     # B = 1: the identity, the reference's order
    ptr, col = in_training_order(d, order)
    st = wr.State(*(by_position(m, w, order) for _, w in TABLES), m.get(cdae_amd.P_BP), **hyper)
    ini = wr.init_state(d.num_users, d.num_items, K, pseed, **hyper)      # IMF's init: the same streams, keyed by position
    for n, _ in TABLES:
        np.testing.assert_allclose(getattr(st, n), getattr(ini, n), rtol=1e-6, atol=1e-9)
    np.testing.assert_array_equal(st.ib, ini.ib)                           # the case's start, bit for bit
    np.testing.assert_array_equal(m.get(cdae_amd.P_UB), ub0)
    return d, m, st, order, ptr, col


def max_err(m, st, order):
    return wr.max_err({n: by_position(m, w, order) for n, w in TABLES}, st)


BIASES = (("ib", cdae_amd.P_BP), ("iba", cdae_amd.P_BP_AG), ("ub", cdae_amd.P_UB), ("uba", cdae_amd.P_UB_AG))


def bias_tables(m):
    """the bias tables and their accumulators, those the handle allocates"""
    out = {}
    for n, w in BIASES:
        try:
            out[n] = m.get(w).view(np.uint32).copy()
        except cdae_amd.CDAEError as e:
            assert "not allocated" in str(e), e
    assert "ib" in out and "ub" in out
    return out


_RUNS = {}


def run_case(case):
    """the case's two epochs, once per session: the device trains, the reference follows its recorded choices"""
    name, ds, B, K, num_neg, hyper, pseed, sseed = case
    if name not in _RUNS:
        d, m, st, order, ptr, col = make(case)
        assert m.batch_users == B
        m.record_choices(True)
        r = dict(comparisons=0, disagreements=0, bad=[], exhausted=0, beyond=0)
        biases = bias_tables(m)
        nnz, blocks = int(d.train_ptr[-1]), d.num_users if B == 1 else -(-d.num_users // B)     # (the loop counts one batch per user)
        for ep in range(wr.EPOCHS):
            stats = m.train_one_iteration(sseed, ep)
            assert (stats.users, stats.examples, stats.batches) == (d.num_users, 2 * num_neg * nnz, blocks)
            assert (m.choices()[1] >= 1).all()                             # every block ran, a tail block of one user too
            o = wr.train(st, wr.Draws(ptr, col, d.num_items, num_neg, sseed, ep), B, choices=m.choices(), tol=wr.TOL)
            assert o["one_user_blocks"] == (B > 1 and d.num_users % B == 1)
            r["bad"] += [(ep,) + b for b in o["bad"]]
            r["comparisons"] += o["comparisons"]; r["disagreements"] += o["disagreements"]
            r["exhausted"] += o["exhausted"]; r["beyond"] += o["cnt65_499"]
            r["err"], r["which"] = max_err(m, st, order)
            print(f"{name} epoch {ep}: {o['comparisons']} comparisons, {o['disagreements']} disagreements, {len(o['bad'])} unverified, "
                  f"{o['exhausted']} exhausted, {o['cnt65_499']} beyond the first round, max |score| {o['max_abs_score']:.3g}, "
                  f"err {r['err']:.3g} ({r['which']})")
        after = bias_tables(m)
        r["biases"] = [n for n in biases if not np.array_equal(biases[n], after[n])]     # the tables two epochs have changed a bit of
        r["bias_start"] = bool(biases["ib"].any()), bool(biases["ub"].any())
        record_measured(f"warp_{name}", err=r["err"], comparisons=r["comparisons"], disagreements=r["disagreements"], unverified=len(r["bad"]))
        m.close()
        _RUNS[name] = r
    return _RUNS[name]


@pytest.mark.parametrize("case", wr.CASES, ids=[c[0] for c in wr.CASES])
def test_every_decision_of_the_trajectory_verifies(built, case):
    r = run_case(case)
    assert not r["bad"], (len(r["bad"]), r["bad"][:5])
    assert r["disagreements"] <= wr.NEAR_SHARE * r["comparisons"], (r["disagreements"], r["comparisons"])
    assert r["exhausted"] >= 1 and r["beyond"] >= 1       # the searches the device made are of the depths the CPU file promises
    # biases are part of no step: P_BP, P_UB and their accumulators keep their bits, from a zero and from a non-zero start
    assert not r["biases"]
    assert r["bias_start"] == (bool(case[5].get("ib0")),) * 2


@pytest.mark.parametrize("case", wr.CASES, ids=[c[0] for c in wr.CASES])
def test_parameters_of_the_trajectory_agree(built, case):
    """2e-4 of the parameter's range after two epochs, the bound tests/test_gpu_mf.py holds IMF / BPR to."""
    r = run_case(case)
    assert r["err"] < 2e-4, (r["err"], r["which"])


def trained(case, record, epochs=wr.EPOCHS):
    d, m, *_ = make(case)
    if record is not None:
        m.record_choices(record)
    for ep in range(epochs):
        m.train_one_iteration(case[7], ep)
    out = [m.get(w).copy() for _, w in TABLES]
    m.close()
    return out


@pytest.mark.parametrize("case", [c for c in wr.CASES if c[0] in ("d40-loop-K65", "d40-block8")], ids=lambda c: c[0])
def test_recording_changes_no_bit_and_a_run_repeats_bit_for_bit(built, case):
    plain, again, recorded, switched_off = trained(case, None), trained(case, None), trained(case, True), trained(case, False)
    for a, b, c, e in zip(plain, again, recorded, switched_off):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(a, e)


def test_the_record_covers_the_users_a_call_trained(built):
    case = next(c for c in wr.CASES if c[0] == "d40-loop-K64")
    d, m, *_ = make(case)
    m.record_choices(True)
    item, cnt = m.choices()
    assert (item == wr.NONE).all() and (cnt == 0).all()                   # nothing trained yet
    m.train_users(case[7], 0, 2, 5)
    item, cnt = m.choices()
    lo, hi = int(d.train_ptr[2]) * 5, int(d.train_ptr[5]) * 5
    assert (cnt[lo:hi] >= 1).all() and (cnt[:lo] == 0).all() and (cnt[hi:] == 0).all()
    assert ((cnt[lo:hi] == wr.MAX_TRY) == (item[lo:hi] == wr.NONE)).all()
    m.close()


def case_named(name):
    return next(c for c in wr.CASES if c[0] == name)


def bits(m):
    return {n: m.get(w).view(np.uint32).copy() for n, w in TABLES}


def assert_same_run(a, b, what):
    """the same bits in uv, uva, iv, iva and the same recorded choices"""
    for n, _ in TABLES:
        np.testing.assert_array_equal(a[0][n], b[0][n], err_msg=f"{what}: {n}")
    np.testing.assert_array_equal(a[1][1], b[1][1], err_msg=f"{what}: cnt")
    np.testing.assert_array_equal(a[1][0], b[1][0], err_msg=f"{what}: item")


def run_ranges(case, ranges=None, enqueue=False, ub=None):
    """the case's epochs from its start, each over `ranges` of positions (None: train_one_iteration), through train_users or through
    enqueue_users + one collect_stats -> (bits of the four tables, recorded choices, (users, examples, batches) summed over the calls)"""
    d, m, *_ = make(case, ub=ub)
    m.record_choices(True)
    total = np.zeros(3, dtype=np.int64)
    for ep in range(wr.EPOCHS):
        for a, b in ranges or ((None, None),):
            if enqueue:
                m.enqueue_users(case[7], ep, a, b)
                continue
            st = m.train_one_iteration(case[7], ep) if a is None else m.train_users(case[7], ep, a, b)
            total += (st.users, st.examples, st.batches)
            lens = np.diff(d.train_ptr)[m.user_order().astype(np.int64)]
            if a is not None and case[2] == 1:                             # the loop: one batch per user, two list places per pair
                assert (st.users, st.examples, st.batches) == (b - a, 2 * case[4] * int(lens[a:b].sum()), b - a)
    if enqueue:
        st = m.collect_stats()
        total += (st.users, st.examples, st.batches)
        st = m.collect_stats()                                             # ... and the counters start again
        assert (st.users, st.examples, st.batches) == (0, 0, 0)
    out = bits(m), m.choices(), tuple(int(x) for x in total)
    m.close()
    return out


@pytest.mark.parametrize("name", ["d40-loop-K65", "d40-block8"])
def test_the_user_biases_are_part_of_nothing(built, name):
    """ub cancels on both sides of the search's test and is part of no step: zero or random, the same bits and the same choices"""
    case = case_named(name)
    U = wr.fixture_data(case[1]).num_users
    zero = run_ranges(case, ub=np.zeros(U, dtype=np.float32))
    rand = run_ranges(case, ub=np.random.default_rng(8).uniform(-2, 2, U).astype(np.float32))
    assert_same_run(zero, rand, "P_UB random")


def test_ranges_of_the_loop_leave_the_bits_of_one_call(built):
    """The in-place loop is ONE wavefront that reads back the rows it has stored; users trained one launch at a time get that order from
    the launch boundary.  Both must be the same loop, bit for bit."""
    case = case_named("d40-loop-K65")
    d = wr.fixture_data(case[1])
    U, pairs = d.num_users, int(d.train_ptr[-1]) * case[4]
    whole = run_ranges(case)
    assert whole[2] == (wr.EPOCHS * U, wr.EPOCHS * 2 * pairs, wr.EPOCHS * U)
    two = run_ranges(case, ((0, 3), (3, U)))
    assert_same_run(whole, two, "(0, 3), (3, U)")
    single = run_ranges(case, [(u, u + 1) for u in range(U)])
    assert_same_run(whole, single, "user by user")
    assert two[2] == whole[2] and single[2] == whole[2]
    queued = run_ranges(case, ((0, 3), (3, U)), enqueue=True)              # enqueue_users + collect_stats are the two train_users calls
    assert_same_run(two, queued, "enqueue_users")
    assert queued[2] == two[2]


def test_ranges_around_the_launch_window_seam_leave_the_same_bits(built):
    """"tiny" has 300 users and a launch of the loop walks 256: ranges that end at the seam and one user before it"""
    case = case_named("tiny-loop")
    d = wr.fixture_data(case[1])
    assert d.num_users == 300
    whole = run_ranges(case)
    for ranges in (((0, 256), (256, 300)), ((0, 255), (255, 300))):
        assert_same_run(whole, run_ranges(case, ranges), str(ranges))


def test_ranges_of_a_block_handle_cut_between_blocks_leave_the_same_bits(built):
    case = case_named("tiny-block33-K24")
    whole = run_ranges(case)
    assert whole[2][2] == wr.EPOCHS * 10                                    # nine blocks of 33 and a tail of three
    cut = run_ranges(case, ((0, 33), (33, 165), (165, 297), (297, 300)))
    assert_same_run(whole, cut, "ranges cut at multiples of 33")
    assert cut[2] == whole[2]


def test_a_sub_range_trains_its_users_only(built):
    """train_users(2, 5) against the reference over the same positions, following the record; the other users keep their bits"""
    case = case_named("d40-loop-K64")
    d, m, st, order, ptr, col = make(case)
    start = bits(m)
    m.record_choices(True)
    m.train_users(case[7], 0, 2, 5)
    o = wr.train(st, wr.Draws(ptr, col, d.num_items, case[4], case[7], 0), 1, choices=m.choices(), tol=wr.TOL, positions=(2, 5))
    assert not o["bad"] and o["disagreements"] <= wr.NEAR_SHARE * o["comparisons"]
    assert o["trained"] >= 1 and o["trained"] + o["exhausted"] == int(d.train_ptr[5] - d.train_ptr[2]) * case[4]
    err, which = max_err(m, st, order)
    print(f"sub-range (2, 5): err {err:.3g} ({which})")
    assert err < 2e-4, (err, which)
    after = bits(m)
    for n in ("uv", "uva"):
        np.testing.assert_array_equal(after[n][:2], start[n][:2]); np.testing.assert_array_equal(after[n][5:], start[n][5:])
        assert (after[n][2:5] != start[n][2:5]).any(axis=1).all()
    m.close()


def test_the_user_id_offset_keys_the_negatives(built):
    """X: D40 with user_id_offset 3.  Y: three one-item users, then D40's rows, offset 0.  Z: D40, offset 0.  User u of X draws what
    user u + 3 of Y draws: the same searches, and from the same tables the same bits; Z draws other negatives.  Then X's trajectory
    against the reference with Draws(uid_offset=3)."""
    case = case_named("d40-loop-K65")
    name, ds, B, K, num_neg, hyper, pseed, sseed = case
    d = wr.fixture_data(ds)
    U, I = d.num_users, d.num_items
    front = np.array([0, 5, 39], dtype=np.uint32)

    def handle(ptr, col, users, offset):
        m = cdae_amd.WARP(config(K, num_neg, 1, hyper))
        m.set_interactions(users, I, ptr, col, user_id_offset=offset)
        m.init_params(pseed)
        np.testing.assert_array_equal(m.user_order(), np.arange(users))    # B = 1: position = user
        return m

    x = handle(d.train_ptr, d.train_col, U, 3)
    y = handle(np.r_[0, 1, 2, 3 + d.train_ptr], np.r_[front, d.train_col], U + 3, 0)
    z = handle(d.train_ptr, d.train_col, U, 0)
    uv, iv = x.get(cdae_amd.P_WU), x.get(cdae_amd.P_W)
    uvy = y.get(cdae_amd.P_WU)
    uvy[3:] = uv
    y.set(cdae_amd.P_WU, uvy); z.set(cdae_amd.P_WU, uv)
    y.set(cdae_amd.P_W, iv); z.set(cdae_amd.P_W, iv)
    x.record_choices(True)
    st = wr.State(*(x.get(w).astype(np.float64) for _, w in TABLES), x.get(cdae_amd.P_BP), **hyper)
    r = dict(comparisons=0, disagreements=0, bad=[])
    for ep in range(wr.EPOCHS):
        sx, sy, sz = x.search(sseed, ep), y.search(sseed, ep, 3, U + 3), z.search(sseed, ep)
        np.testing.assert_array_equal(sx[0], sy[0]); np.testing.assert_array_equal(sx[1], sy[1])
        if ep == 0:                                                        # (the same tables still: only the keys differ)
            assert (sx[0] != sz[0]).any()
        x.train_one_iteration(sseed, ep); y.train_users(sseed, ep, 3, U + 3); z.train_one_iteration(sseed, ep)
        gx, gy, gz = bits(x), bits(y), bits(z)
        for n in ("iv", "iva"):
            np.testing.assert_array_equal(gy[n], gx[n], err_msg=n)
        for n in ("uv", "uva"):
            np.testing.assert_array_equal(gy[n][3:], gx[n], err_msg=n)
        assert (gz["iv"] != gx["iv"]).any() and (gz["uv"] != gx["uv"]).any()           # the offset is read
        o = wr.train(st, wr.Draws(d.train_ptr, d.train_col, I, num_neg, sseed, ep, uid_offset=3), 1, choices=x.choices(), tol=wr.TOL)
        r["bad"] += o["bad"]; r["comparisons"] += o["comparisons"]; r["disagreements"] += o["disagreements"]
    err, which = wr.max_err({n: x.get(w).astype(np.float64) for n, w in TABLES}, st)
    print(f"offset 3: {r['comparisons']} comparisons, {r['disagreements']} disagreements, {len(r['bad'])} unverified, err {err:.3g} ({which})")
    record_measured("warp_uid_offset", err=err, comparisons=r["comparisons"], disagreements=r["disagreements"], unverified=len(r["bad"]))
    assert not r["bad"] and r["disagreements"] <= wr.NEAR_SHARE * r["comparisons"]
    assert err < 2e-4, (err, which)
    for m in (x, y, z):
        m.close()


def test_a_warp_handle_is_served_like_an_imf_handle(built):
    """the same tables in a WARP handle and in an IMF handle: the same lists from recommend_all, the same neighbours from similar_items"""
    d = wr.fixture_data("tiny")
    rng = np.random.default_rng(4)
    K = 24
    w = cdae_amd.WARP(cdae_amd.WARPConfig(num_dim=K)); w.reset(d, seed=3)
    f = cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, batch_users=1)); f.reset(d, seed=3)
    tables = {cdae_amd.P_WU: rng.standard_normal((d.num_users, K)), cdae_amd.P_W: rng.standard_normal((d.num_items, K)),
              cdae_amd.P_UB: rng.standard_normal(d.num_users), cdae_amd.P_BP: rng.standard_normal(d.num_items)}
    for which, t in tables.items():
        w.set(which, t.astype(np.float32)); f.set(which, t.astype(np.float32))
        np.testing.assert_array_equal(w.get(which), t.astype(np.float32))
    for topk in (10, 20):
        np.testing.assert_array_equal(w.recommend_all(topk), f.recommend_all(topk))
    np.testing.assert_array_equal(w.recommend_all(10, 40, 90), f.recommend_all(10)[40:90])
    np.testing.assert_array_equal(w.similar_items(np.arange(30), topk=5), f.similar_items(np.arange(30), topk=5))
    w.set_test_rows(d.test_ptr, d.test_col); f.set_test_rows(d.test_ptr, d.test_col)
    np.testing.assert_array_equal(w.eval_topn(10)[0], f.eval_topn(10)[0])
    assert w.current_loss(1, 0) == 0.0
    w.close(); f.close()
