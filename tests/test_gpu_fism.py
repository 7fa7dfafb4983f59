"""-m gpu: FISM training (cdae_hip_create_fism, cdae_fism_kernels.hpp) against tests/fism_ref.py, the fp64 restatement of the loop, over
two epochs: all six tables (P, Q, their accumulators, bi, bu) within 2e-4 of the reference in the measure of tests/test_gpu_mf.py
(max |difference| / (1e-3 + max |value|)).  A FISM trajectory takes no decision, so the device and the reference run free; that the
trajectories are well conditioned (the float32 reference within 5e-5 of the float64 one) is tests/test_fism_reference.py's assertion.

Cases (fism_ref.CASES): the loop on D40 at both edges of every NI tier; at K = 200 plain SGD, CE, LOG, num_neg 1 and 12, no bias terms,
alpha 0 / 0.5 / 1; rows of 1 and 2 items; duplicate negatives inside one user (D12, num_neg 12); more than one launch window ("win");
the residency seam at K = 64 / 256 / 512 (rows of 1, 2, W - 1, W, W + 1, C - 1, C, C + 1, 2C + 1 items with C from cdae_hip_fism_plan).
Bit equality: both residency settings on every seam case, two runs, one range against two adjacent ranges and against single users.
Further cases: users without train items ("gaps", at K = 24 and 200: they take no step); rows of 11 of 12 items, whose draws reach the
walk behind 32 rejected candidates ("dense"); num_neg 64, 65 and 130, the second round of the 64 negatives a wavefront draws at once;
plain SGD and no bias terms at the other NI tiers.  Exactly: a handle with user_id_offset 3 against one with three empty users in front;
enqueue_users + collect_stats against train_users.
"""
import numpy as np
import pytest

import cdae_amd
import fism_ref as fr

pytestmark = pytest.mark.gpu

TABLES = (("P", cdae_amd.P_W), ("Pa", cdae_amd.P_W_AG), ("Q", cdae_amd.P_V), ("Qa", cdae_amd.P_V_AG), ("bi", cdae_amd.P_BP), ("bu", cdae_amd.P_UB))
ALL8 = TABLES + (("bia", cdae_amd.P_BP_AG), ("bua", cdae_amd.P_UB_AG))
SEAMS = ("seam64", "seam256", "seam512")


def config(K, num_neg, hyper):
    return cdae_amd.FISMConfig(num_dim=K, num_neg=num_neg, lt=hyper.get("loss", cdae_amd.SQUARE), using_adagrad=hyper.get("adagrad", True),
                               using_bias_term=hyper.get("bias", True), learn_rate=hyper.get("learn_rate", 0.1),
                               lambda_=hyper.get("lambda_", 0.01), alpha=hyper.get("alpha", 1.0))


def make(case):
    name, ds, K, num_neg, hyper, sseed = case
    d = fr.fixture_data(ds)
    m = cdae_amd.FISM(config(K, num_neg, hyper))
    m.reset(d, seed=fr.PSEED)
    return d, m


def tables(m, which=TABLES):
    return {n: m.get(w) for n, w in which}


def train(m, case, ranges=None, resident=True):
    """the case's epochs from the state the handle is in -> (tables, stats of the last call)"""
    m.set_resident(resident)
    st = None
    for ep in range(fr.EPOCHS):
        if ranges is None:
            st = m.train_one_iteration(case[5], ep)
        else:
            for a, b in ranges:
                st = m.train_users(case[5], ep, a, b)
    return tables(m), st


def test_init_params_is_the_references_start():
    c = fr.case("d40-K65")
    d, m = make(c)
    st = fr.new_state(c)
    for n, w in TABLES:
        np.testing.assert_array_equal(m.get(w), getattr(st, n).astype(np.float32), err_msg=n)
    np.testing.assert_array_equal(m.get(cdae_amd.P_BP_AG), np.full(d.num_items, 1e-4, np.float32))
    np.testing.assert_array_equal(m.get(cdae_amd.P_UB_AG), np.full(d.num_users, 1e-4, np.float32))
    for which in (cdae_amd.P_WU, cdae_amd.P_WU_AG, cdae_amd.P_UU, cdae_amd.P_B):
        with pytest.raises(cdae_amd.CDAEError, match="not allocated"):
            m.get(which)


@pytest.mark.parametrize("name", [c[0] for c in fr.CASES])
def test_two_epochs_match_the_reference(name):
    c = fr.case(name)
    d, m = make(c)
    if name.startswith("seam"):
        lens = np.diff(d.train_ptr)
        C, W = m.plan()["resident_rows"], fr.WAVES
        assert C == fr.resident_rows(c[2]) and sorted(lens.tolist()) == sorted((1, 2, W - 1, W, W + 1, C - 1, C, C + 1, 2 * C + 1))
    got, stats = train(m, c)
    nnz = int(d.train_ptr[-1])
    assert (stats.users, stats.examples) == (d.num_users, nnz * (1 + c[3]))
    ref = fr.reference(name)
    errs = {n: fr.measure(got[n], getattr(ref, n)) for n, _ in TABLES}
    print(f"{name}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert max(errs.values()) <= fr.BOUND, errs
    if not c[4].get("bias", True):
        assert not got["bi"].any() and not got["bu"].any()


def assert_same_bits(a, b, what):
    for n in a:
        np.testing.assert_array_equal(a[n].view(np.uint32), b[n].view(np.uint32), err_msg=f"{what}: {n}")


@pytest.mark.parametrize("name", SEAMS)
def test_both_residency_settings_give_the_same_bits(name):
    c = fr.case(name)
    d, m = make(c)
    assert m.plan()["resident_rows"] > 0
    a, _ = train(m, c, resident=True)
    m.init_params(fr.PSEED)
    m.set_resident(False)
    assert m.plan()["resident_rows"] == 0
    b, _ = train(m, c, resident=False)
    assert_same_bits(a, b, name)
    m.init_params(fr.PSEED)                                   # ... and a second run leaves the same bits again
    a2, _ = train(m, c, resident=True)
    assert_same_bits(a, a2, name + " repeated")


def test_one_range_and_two_adjacent_ranges_give_the_same_bits():
    c = fr.case("d40-K65")
    d, m = make(c)
    a, st = train(m, c)
    assert st.batches == 1                                    # D40's 846 instances: one launch window
    m.init_params(fr.PSEED)
    b, _ = train(m, c, ranges=((0, 3), (3, d.num_users)))
    assert_same_bits(a, b, "two ranges")


def test_a_window_boundary_inside_the_range_gives_the_same_bits():
    c = fr.case("win")
    d, m = make(c)
    inst = int(d.train_ptr[-1]) * (1 + c[3])
    assert inst > m.plan()["window_instances"] == fr.WINDOW_INSTANCES
    a, st = train(m, c)
    assert (st.batches, st.users, st.examples) == (2, d.num_users, inst)
    m.init_params(fr.PSEED)
    b, st = train(m, c, ranges=[(u, u + 1) for u in range(d.num_users)])
    assert (st.batches, st.users) == (1, 1)
    assert_same_bits(a, b, "user by user")


def test_a_sub_range_trains_its_users_only():
    c = fr.case("d40-K65")
    d, m = make(c)
    m.train_users(c[5], 0, 2, 5)
    ref = fr.new_state(c)
    n = fr.train(ref, d.train_ptr, d.train_col, c[5], 0, users=(2, 5))
    got = tables(m)
    assert n == int(d.train_ptr[5] - d.train_ptr[2]) * 6
    assert max(fr.measure(got[k], getattr(ref, k)) for k, _ in TABLES) <= fr.BOUND
    assert not got["bu"][:2].any() and not got["bu"][5:].any() and got["bu"][2:5].all()


@pytest.mark.parametrize("name", ("gaps-K24", "gaps-K200"))
def test_users_without_train_items_take_no_step(name):
    """include/cdae_hip.h: such a user is counted in stats.users, adds nothing to stats.examples, and bu[u] and its accumulator keep
    their bits"""
    c = fr.case(name)
    d, m = make(c)
    lens = np.diff(d.train_ptr)
    empty, U = lens == 0, d.num_users
    assert tuple(lens) == fr.GAPS_LENGTHS
    start = tables(m, ALL8)
    pair = next(u for u in range(U - 1) if empty[u] and empty[u + 1])
    st = m.train_users(c[5], 0, pair, pair + 2)               # a range of empty users alone: a launch that holds no instance
    assert (st.users, st.examples) == (2, 0)
    assert_same_bits(start, tables(m, ALL8), "two empty users")
    _, st = train(m, c)
    assert (st.users, st.examples) == (U, int(d.train_ptr[-1]) * (1 + c[3]))
    a = tables(m, ALL8)
    for n in ("bu", "bua"):
        np.testing.assert_array_equal(a[n][empty].view(np.uint32), start[n][empty].view(np.uint32), err_msg=n)
        assert (a[n][~empty] != start[n][~empty]).all(), n
    m.init_params(fr.PSEED)
    train(m, c, ranges=[(u, u + 1) for u in range(U)])
    assert_same_bits(a, tables(m, ALL8), "user by user")
    m.init_params(fr.PSEED)
    train(m, c, resident=False)
    assert_same_bits(a, tables(m, ALL8), "every row streaming")


def test_the_user_id_offset_keys_the_negatives():
    """X: D40 with user_id_offset 3.  Y: three empty users, then D40's rows, offset 0.  User u of X draws what user u + 3 of Y draws, so
    from the same P and Q both end with the same bits; without the offset D40 draws other negatives."""
    c = fr.case("d40-K65")
    d = fr.fixture_data(c[1])
    U, I = d.num_users, d.num_items

    def handle(ptr, users, offset):
        m = cdae_amd.FISM(config(c[2], c[3], c[4]))
        m.set_interactions(users, I, ptr, d.train_col, user_id_offset=offset)
        m.init_params(fr.PSEED)
        return m

    x = handle(d.train_ptr, U, 3)
    y = handle(np.r_[0, 0, 0, d.train_ptr], U + 3, 0)
    z = handle(d.train_ptr, U, 0)
    for w in (cdae_amd.P_W, cdae_amd.P_V):
        y.set(w, x.get(w))
        z.set(w, x.get(w))
    bu0 = tables(y, ALL8)
    shared = [t for t in ALL8 if t[0] not in ("bu", "bua")]
    for m in (x, y, z):
        train(m, c)
    gx, gy, gz = (tables(m, ALL8) for m in (x, y, z))
    assert_same_bits({n: gx[n] for n, _ in shared}, {n: gy[n] for n, _ in shared}, "offset 3 against three users in front")
    for n in ("bu", "bua"):
        np.testing.assert_array_equal(gy[n][3:].view(np.uint32), gx[n].view(np.uint32), err_msg=n)
        np.testing.assert_array_equal(gy[n][:3].view(np.uint32), bu0[n][:3].view(np.uint32), err_msg=n)
    assert (gx["Q"].view(np.uint32) != gz["Q"].view(np.uint32)).any()          # the offset is read


def test_enqueue_users_and_collect_stats_are_train_users():
    c = fr.case("d40-K65")
    d, m = make(c)
    ranges = ((0, 3), (3, d.num_users))
    want = np.zeros(3, dtype=np.int64)
    for ep in range(fr.EPOCHS):
        for a, b in ranges:
            st = m.train_users(c[5], ep, a, b)
            want += (st.users, st.examples, st.batches)
    a = tables(m, ALL8)
    assert tuple(want) == (fr.EPOCHS * d.num_users, fr.EPOCHS * int(d.train_ptr[-1]) * (1 + c[3]), fr.EPOCHS * 2)
    m.init_params(fr.PSEED)
    for ep in range(fr.EPOCHS):
        for u0, u1 in ranges:
            m.enqueue_users(c[5], ep, u0, u1)
    st = m.collect_stats()
    assert (st.users, st.examples, st.batches) == tuple(want)
    assert_same_bits(a, tables(m, ALL8), "enqueue_users")
    st = m.collect_stats()                                      # ... and the counters start again
    assert (st.users, st.examples, st.batches) == (0, 0, 0)
