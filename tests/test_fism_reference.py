"""CPU: tests/fism_ref.py, the fp64 restatement of FISM that tests/test_gpu_fism.py holds the device to — the premise of its bound (every
case's float32 run ends within DRIFT_MAX of the float64 one, so that 2e-4 on the device measures the kernel and not the trajectory), the
gradients it steps on against finite differences of the loss, and that the restated algorithm learns.  Also what the fixtures are
for: the empty rows of "gaps", the draws of "dense" that reach the walk behind 32 rejected candidates, the second round of negatives at
num_neg 65 and 130 — and that a trajectory with either draw done wrong ends far outside the device bound on every table."""
import numpy as np
import pytest

import fism_ref as fr


@pytest.mark.parametrize("name", [c[0] for c in fr.CASES])
def test_the_float32_reference_stays_within_the_drift_premise(name):
    r = fr.run_free(fr.case(name))
    print(f"{name}: drift {r['drift']:.2e} (recorded {fr.DRIFTS[name]:.2e}), max |pred| {r['max_abs_pred']:.3g}")
    assert r["drift"] <= fr.DRIFT_MAX, r
    assert r["drift"] == pytest.approx(fr.DRIFTS[name], rel=0.05)          # the figure in the file is this run's
    assert r["max_abs_pred"] < 16.0


def test_the_cases_cover_what_the_gpu_test_names():
    by = {c[0]: c for c in fr.CASES}
    assert {by[f"d40-K{K}"][2] for K in (1, 64, 65, 128, 129, 256, 257, 512)} == {1, 64, 65, 128, 129, 256, 257, 512}      # both edges of every NI tier
    assert by["d40-sgd"][4]["adagrad"] is False and by["d40-ce"][4]["loss"] == 5 and by["d40-log"][4]["loss"] == 2
    assert (by["d40-neg1"][3], by["d40-neg12"][3], by["d12-neg12"][3]) == (1, 12, 12) and by["d40-nobias"][4]["bias"] is False
    assert [by[n][4]["alpha"] for n in ("d40-alpha0", "d40-alpha05", "d40-alpha1")] == [0.0, 0.5, 1.0]
    for c in fr.CASES:
        assert c[4].get("learn_rate", 0.1) in (0.1, 0.03, 0.01) and c[4]["alpha"] == (1.0 if c[0].startswith("seam") or c[0] == "d40-alpha1" else
                                                                                     0.0 if c[0] == "d40-alpha0" else 0.5)
    assert sorted(np.diff(fr.fixture_data("ones").train_ptr).tolist())[0] == 1 and max(np.diff(fr.fixture_data("ones").train_ptr)) == 2
    win = fr.fixture_data("win")
    assert int(win.train_ptr[-1]) * 6 > fr.WINDOW_INSTANCES
    for K in (64, 256, 512):
        C, W = fr.resident_rows(K), fr.WAVES
        d = fr.fixture_data(f"seam{K}")
        assert sorted(np.diff(d.train_ptr).tolist()) == sorted((1, 2, W - 1, W, W + 1, C - 1, C, C + 1, 2 * C + 1)) and d.num_items == 2 * C + 200
    # duplicate negatives inside one user: D12's longest row leaves 3 items for 12 draws per positive
    d12 = fr.fixture_data("d12")
    neg = fr.negatives(d12.train_ptr, d12.train_col, 12, 12, 1, 0, 3)
    assert all(np.unique(row).size < row.size for row in neg)
    # users without train items: the first, the last, two in a row, one between trained users; at NI = 1 and at NI = 4
    lens = np.diff(fr.fixture_data("gaps").train_ptr).tolist()
    assert tuple(lens) == fr.GAPS_LENGTHS and lens[0] == 0 and lens[-1] == 0
    assert any(a == 0 and b == 0 for a, b in zip(lens, lens[1:])) and any(a > 0 and b == 0 and c > 0 for a, b, c in zip(lens, lens[1:], lens[2:]))
    assert (by["gaps-K24"][1:4], by["gaps-K200"][1:4]) == (("gaps", 24, 5), ("gaps", 200, 5))
    # rows that leave one item to draw from
    assert sorted(np.diff(fr.fixture_data("dense").train_ptr).tolist()) == [0, 1, 4, 10, 11, 11] and fr.fixture_data("dense").num_items == 12
    assert by["dense"][1:4] == ("dense", 24, 5)
    # the second round of the 64 negatives a wavefront draws at once: a full round, one more, two rounds and two more; at NI = 1 and NI = 4
    assert [by[n][1:4] for n in REFILL + ("d12-neg64",)] == [("d12", 24, 65), ("d12", 24, 130), ("d40", 200, 65), ("d12", 24, 64)]
    # plain SGD and no bias terms at the other three NI tiers (K = 200 has them above)
    for K in (64, 128, 512):
        assert by[f"d40-sgd-K{K}"][1:4] == ("d40", K, 5) and by[f"d40-sgd-K{K}"][4]["adagrad"] is False
    for K in (64, 512):
        assert by[f"d40-nobias-K{K}"][1:4] == ("d40", K, 5) and by[f"d40-nobias-K{K}"][4]["bias"] is False


REFILL = ("d12-neg65", "d12-neg130", "d40-neg65")          # num_neg above the 64 negatives one round holds
ROUND = 64


@pytest.mark.parametrize("name", REFILL)
def test_a_kernel_that_replays_its_first_round_draws_other_items(name):
    """at the case's seed, in both epochs, every user has a positive p and a k >= 64 whose negative is not the one of k % 64"""
    _, ds, K, nn, hyper, sseed = fr.case(name)
    d = fr.fixture_data(ds)
    for ep in range(fr.EPOCHS):
        for u in range(d.num_users):
            neg = fr.negatives(d.train_ptr, d.train_col, d.num_items, nn, sseed, ep, u)
            assert neg.shape == (d.train_ptr[u + 1] - d.train_ptr[u], nn)
            assert (neg[:, ROUND:] != neg[:, np.arange(ROUND, nn) % ROUND]).any(), (ep, u)


def without_the_walk(ptr, col, num_items, num_neg, seed, epoch, u):
    """fr.negatives, wrong: a draw whose 32 candidates are all rated keeps the last of them -> (negatives, such draws)"""
    cand = fr.candidates(ptr, col, num_items, num_neg, seed, epoch, u)
    rated = np.isin(cand, col[ptr[u]:ptr[u + 1]])
    first = np.where(rated.all(axis=2), cand.shape[2] - 1, np.argmin(rated, axis=2))
    return np.take_along_axis(cand, first[:, :, None], axis=2)[:, :, 0], int(rated.all(axis=2).sum())


def test_dense_rows_send_draws_to_the_walk():
    """in each epoch of "dense" at least one draw finds all 32 candidates rated; every other draw is the first unrated candidate, and a
    walked one is an unrated item that is not the last candidate"""
    _, ds, K, nn, hyper, sseed = fr.case("dense")
    d = fr.fixture_data(ds)
    for ep in range(fr.EPOCHS):
        walked = 0
        for u in range(d.num_users):
            row = d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]
            neg = fr.negatives(d.train_ptr, d.train_col, d.num_items, nn, sseed, ep, u)
            wrong, w = without_the_walk(d.train_ptr, d.train_col, d.num_items, nn, sseed, ep, u)
            assert int((neg != wrong).sum()) == w and not np.isin(neg, row).any()
            walked += w
        print(f"dense, epoch {ep}: {walked} draws take the walk")
        assert walked >= 1


@pytest.mark.parametrize("name", REFILL + ("dense",))
def test_the_fixtures_tell_a_wrong_draw_from_the_right_one(name, monkeypatch):
    """The fp64 reference with wrong negatives — the first round replayed (neg[:, k] = neg[:, k % 64]), or for "dense" the last rejected
    candidate kept instead of the walk — ends at least 10 x BOUND from the reference on every one of the six tables: a kernel with either
    fault cannot pass test_gpu_fism.py's bound on any table."""
    c = fr.case(name)
    d = fr.fixture_data(c[1])
    right = fr.reference(name)
    true_negatives = fr.negatives

    def wrong(ptr, col, num_items, num_neg, seed, epoch, u):
        if name == "dense":
            return without_the_walk(ptr, col, num_items, num_neg, seed, epoch, u)[0]
        neg = true_negatives(ptr, col, num_items, num_neg, seed, epoch, u)
        return neg[:, np.arange(num_neg) % ROUND]

    monkeypatch.setattr(fr, "negatives", wrong)
    st = fr.new_state(c)
    for ep in range(fr.EPOCHS):
        fr.train(st, d.train_ptr, d.train_col, c[5], ep)
    dist = {n: fr.measure(getattr(st, n), getattr(right, n)) for n in fr.State.TABLES}
    print(f"{name}: " + ", ".join(f"{n} {e:.2e}" for n, e in dist.items()))
    assert min(dist.values()) >= 10 * fr.BOUND, dist


def loss_value(loss, pred, label):
    if loss == 0:
        return (label - pred) ** 2
    assert loss == 5
    return (1.0 - label) * pred + np.log1p(np.exp(-pred))


@pytest.mark.parametrize("loss", [0, 5])
@pytest.mark.parametrize("rated", [True, False])
def test_the_gradients_are_the_derivatives_of_the_loss(loss, rated):
    """P, Q and both biases: the gradient train() steps on against central differences of loss + lambda / 2 |.|^2 (fism.hpp's L2 terms)"""
    rng = np.random.default_rng(3)
    I, U, K = 12, 2, 5
    st = fr.State(rng.normal(0, 0.5, (I, K)), rng.normal(0, 0.5, (I, K)), U, loss=loss, alpha=0.5, lambda_=0.07)
    st.bi[:] = rng.normal(0, 0.3, I); st.bu[:] = rng.normal(0, 0.3, U)
    rows = np.array([1, 4, 5, 9, 10])
    item = 5 if rated else 7
    g = fr.grads(st, 1, rows, item, rated)

    def numeric(arr, index):
        h = 1e-6
        old = arr[index]
        arr[index] = old + h; up = fr.instance_loss(st, 1, rows, item, rated, loss_value)
        arr[index] = old - h; dn = fr.instance_loss(st, 1, rows, item, rated, loss_value)
        arr[index] = old
        return (up - dn) / (2 * h)

    for r, j in enumerate(g["idx"]):
        for k in range(K):
            assert numeric(st.P, (j, k)) == pytest.approx(g["P"][r, k], rel=1e-6, abs=1e-8)
    if rated:                                              # the rated item's own row is part of no step (j != i)
        assert item not in g["idx"] and numeric(st.P, (item, 0)) == 0.0
    for k in range(K):
        assert numeric(st.Q, (item, k)) == pytest.approx(g["Q"][k], rel=1e-6, abs=1e-8)
    assert numeric(st.bu, 1) == pytest.approx(g["bu"], rel=1e-6, abs=1e-8)
    assert numeric(st.bi, item) == pytest.approx(g["bi"], rel=1e-6, abs=1e-8)


def recall_at_10(scores, d):
    hits = total = 0.0
    users = 0
    for u in range(d.num_users):
        test = d.test_col[d.test_ptr[u]:d.test_ptr[u + 1]]
        if test.size == 0:
            continue
        s = scores(u).copy()
        s[d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]] = -np.inf
        top = np.argsort(-s, kind="stable")[:10]
        total += np.isin(top, test).sum() / test.size
        users += 1
    return total / users


def test_the_reference_learns_to_rank_held_out_items():
    """After EPOCHS (two) epochs on "tiny" the fp64 reference ranks held-out items better than popularity does (Recall@10).
    Two epochs over 300 users are few: from the 1e-3 initial factors AdaGrad's steps shrink as 1 / sqrt(steps taken), and at FISM's
    default learn rate the item factors have not yet overtaken what the item biases alone (popularity) give.  So this test takes a three
    times larger rate, 0.3, with the paper's mid alpha 0.5 and K = 16.  Measured (popularity 0.2377), Recall@10 after epoch 1, 2[, 3, 4]:
      K 16, rate 0.3,  alpha 0.5         0.2207  0.2441     <- this test
      K 16, rate 0.1,  alpha 0.5         0.2057  0.2271  0.2350  0.2419   (overtakes popularity in its fourth epoch)
      K 32, rate 0.1,  alpha 0.5         0.2227  0.2389
      K 16, rate 0.03, alpha 0.5         -       0.2346
      K 10, rate 0.1,  alpha 1 (defaults) 0.2224  0.2150  0.2186  0.2157
      K 16, rate 0.1,  alpha 0.5, num_neg 12 / CE / CE and num_neg 12:  0.2184 / 0.2143 / 0.2130 after epoch 2"""
    d = fr.fixture_data("tiny")
    st = fr.init_state(d.num_items, d.num_users, 16, fr.PSEED, alpha=0.5, learn_rate=0.3)
    for ep in range(fr.EPOCHS):
        fr.train(st, d.train_ptr, d.train_col, 1, ep)
    pop = np.bincount(d.train_col, minlength=d.num_items).astype(np.float64)
    r_pop = recall_at_10(lambda u: pop, d)
    r_fism = recall_at_10(lambda u: st.Q @ fr.hidden(st, d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]) + st.bi, d)
    print(f"Recall@10: FISM {r_fism:.4f}, popularity {r_pop:.4f}")
    assert r_fism > r_pop


# ---- the grid fixture (fism_ref.grid_*): the premises of tests/test_gpu_model_saturation.py -------------------------------------------
def assert_grid_premises(first, classes, want_classes):
    """the first predictions ARE the grid; 22 and 8 of its 53 points lie beyond +-18 and +-88.5 (test_mf_from_grid_scores' shares); the
    run has met every class of saturated instance"""
    np.testing.assert_array_equal(first, fr.grid().astype(first.dtype))
    assert fr.share_beyond(first, 18) > 0.4 and fr.share_beyond(first, 88.5) > 0.14
    assert all(classes.get(c, 0) >= 1 for c in want_classes), classes


FISM_CLASSES = ((True, 1), (True, -1), (False, 1), (False, -1))          # (positive label?, the sign of a prediction beyond +-18)


def test_the_grid_rows_leave_wavefronts_without_a_row():
    d = fr.grid_data()
    lens = np.diff(d.train_ptr)
    assert (d.num_users, d.num_items) == (53, 100) and (lens == 5).all() and 5 < fr.WAVES
    assert (d.train_col[d.train_ptr[:-1]] == np.arange(53)).all()             # user u's first item is item u
    assert fr.scale_table(5, 0.5)[4] == 0.5
    assert set(fr.GRID_CASES) == {"sq-ada", "log-ada", "ce-ada", "log-sgd", "ce-sgd", "log-ada-K300", "log-ada-nobias"}
    assert fr.resident_rows(300) == fr.WAVES * 8 and fr.GRID_CASES["log-ada-K300"][0] == 300


@pytest.mark.parametrize("name", list(fr.GRID_CASES))
def test_the_grid_fixture_predicts_the_grid_and_stays_within_the_drift_premise(name):
    """Every user's first instance predicts its grid point bit for bit, in float64 and in float32; over the two epochs the fp64 reference
    meets a positive and a negative label on either side of +-18; and the same loop in float32 ends within GRID_BOUND / 4 of it, element
    by element — so GRID_BOUND on the device measures the kernel."""
    K, hyper = fr.GRID_CASES[name]
    for dtype64 in (True, False):
        assert_grid_premises(fr.grid_first(fr.grid_state(K, hyper, dtype64)), fr.grid_reference(name).classes, FISM_CLASSES)
    ref = fr.grid_reference(name)
    st32 = fr.grid_run(fr.train, K, hyper, dtype64=False)
    drift = {n: fr.grid_measure(getattr(st32, n), getattr(ref, n)) for n in fr.State.TABLES}
    print(f"grid {name}: max |pred| {ref.max_abs_pred:.4g}, classes {ref.classes}, drift " + ", ".join(f"{n} {e:.2e}" for n, e in drift.items()))
    assert max(drift.values()) <= fr.GRID_DRIFT_MAX, drift
    assert ref.max_abs_pred >= 1000.0


def grid_fault_applies(fault, hyper):
    loss = hyper["loss"]
    return {"neg_label_0": loss == 2, "exp_sign": loss in (2, 5), "clamp18": loss == 0, "no_bias": hyper.get("bias", True),
            "no_s_in_row_step": True}[fault]


GRID_FAULT_CASES = [(f, n) for f in fr.FAULTS for n, (K, h) in fr.GRID_CASES.items() if K == 16 and grid_fault_applies(f, h)]


@pytest.mark.parametrize("fault,name", GRID_FAULT_CASES)
def test_the_grid_fixture_tells_a_faulty_saturated_instance_from_the_right_one(fault, name):
    """The fp64 reference with ONE fault (fism_ref.FAULTS) ends at least 10 x GRID_BOUND from its true self on some compared table, in
    the measure of the GPU test: on every case the fault can differ on (LOG's negative label on LOG; the exponent's sign on LOG and
    CROSS_ENTROPY; the clamp on SQUARE; the biases where there are bias terms)."""
    K, hyper = fr.GRID_CASES[name]
    right = fr.grid_reference(name)
    wrong = fr.grid_run(fr.train, K, hyper, fault=fault)
    dist = {n: fr.grid_measure(getattr(wrong, n), getattr(right, n)) for n in fr.State.TABLES}
    print(f"grid {name}, {fault}: " + ", ".join(f"{n} {e:.2e}" for n, e in dist.items()))
    assert max(dist.values()) >= 10 * fr.GRID_BOUND, dist


def test_every_fault_is_held_against_some_grid_case():
    assert {f for f, _ in GRID_FAULT_CASES} == set(fr.FAULTS)
