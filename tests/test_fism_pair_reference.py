"""CPU: tests/fism_pair_ref.py, the fp64 restatement of FISMauc that tests/test_gpu_fism_pair.py holds the device to — the premise of its
bound (every case's float32 run ends within DRIFT_MAX of the float64 one), the gradients of a pair against finite differences of its
loss, that the restated algorithm learns, and that the fixtures tell the three likely kernel faults from the right loop: each fault leaves
the fp64 reference at least 10 x BOUND away on every table it touches."""
import numpy as np
import pytest

import fism_pair_ref as pr
import fism_ref as fr
from test_fism_reference import recall_at_10


@pytest.mark.parametrize("name", [c[0] for c in pr.CASES])
def test_the_float32_reference_stays_within_the_drift_premise(name):
    r = pr.run_free(pr.case(name))
    print(f"{name}: drift {r['drift']:.2e} (recorded {pr.DRIFTS[name]:.2e}), max |d| {r['max_abs_pred']:.3g}")
    assert r["drift"] <= pr.DRIFT_MAX, r
    assert r["drift"] == pytest.approx(pr.DRIFTS[name], rel=0.05)          # the figure in the file is this run's
    assert r["max_abs_pred"] < 32.0


def test_the_cases_cover_what_the_gpu_test_names():
    by = {c[0]: c for c in pr.CASES}
    for K in (1, 64, 65, 128, 129, 256, 257, 512):                          # both edges of every NI tier, AdaGrad
        assert by[f"d40-K{K}"][1:4] == ("d40", K, 5) and by[f"d40-K{K}"][4].get("adagrad", True)
    for K in (64, 128, 200, 512):                                            # plain SGD at one K per tier
        assert by[f"d40-sgd-K{K}"][2] == K and by[f"d40-sgd-K{K}"][4]["adagrad"] is False
    assert by["d40-log"][4]["loss"] == 2 and by["d40-nobias"][4]["bias"] is False
    assert [by[n][4]["alpha"] for n in ("d40-alpha0", "d40-alpha05", "d40-alpha1")] == [0.0, 0.5, 1.0]
    assert [by[n][3] for n in ("d40-neg1", "d12-neg12", "d12-neg64", "d12-neg65")] == [1, 12, 64, 65]
    for c in pr.CASES:
        assert c[4].get("learn_rate", 0.1) in (0.1, 0.03, 0.01) and c[4].get("loss", 0) in (0, 2) and c[5] in (1, 2, 3)
    assert by["ones"][1] == "ones" and by["dense"][1] == "dense" and (by["gaps-K24"][1:3], by["gaps-K200"][1:3]) == (("gaps", 24), ("gaps", 200))
    win = pr.fixture_data("win")
    assert int(win.train_ptr[-1]) * by["win"][3] > pr.WINDOW_INSTANCES        # more pairs than one launch window holds
    for K in (64, 256, 512):
        assert by[f"seam{K}"][1:3] == (f"seam{K}", K)
    # a negative repeats inside one positive: D12's longest row leaves 3 items for 12 draws
    d12 = pr.fixture_data("d12")
    for ep in range(pr.EPOCHS):
        neg = pr.negatives(d12.train_ptr, d12.train_col, 12, 12, by["d12-neg12"][5], ep, 3)
        assert all(np.unique(row).size < row.size for row in neg)


FAULT_CASES = ("d12-neg12", "d40-K64", "d40-K1")


@pytest.mark.parametrize("fault", pr.FAULTS)
@pytest.mark.parametrize("name", FAULT_CASES)
def test_the_fixtures_tell_a_faulty_loop_from_the_right_one(name, fault):
    """(a) Q[i] and bi[i] held at their start-of-positive values across a positive's pairs (the reference file's stale prediction; a
    register copy that is not stepped), (b) Q[j] of a negative that repeats inside a positive read from before its first step (D12 with
    12 negatives has such repeats in every positive of its longest row; D40's draws repeat too), (c) P[i] left inside v: a kernel with
    any of them cannot pass test_gpu_fism_pair.py's bound on any table."""
    c = pr.case(name)
    right = pr.reference(name)
    st = pr.run(c, fault=fault)
    touched = [n for n in pr.TABLES if c[4].get("adagrad", True) or n not in ("Pa", "Qa")]
    dist = {n: pr.measure(getattr(st, n), getattr(right, n)) for n in touched}
    print(f"{name}, {fault}: " + ", ".join(f"{n} {e:.2e}" for n, e in dist.items()))
    assert len(dist) == 5 and min(dist.values()) >= 10 * pr.BOUND, dist


def loss_value(loss, d):
    if loss == 0:
        return (1.0 - d) ** 2
    assert loss == 2
    return np.log1p(np.exp(-d))


@pytest.mark.parametrize("loss", [0, 2])
@pytest.mark.parametrize("bias", [True, False])
def test_the_pair_gradients_are_the_derivatives_of_the_loss(loss, bias):
    """P, both rows of Q and both biases: the gradient train() steps on against central differences of loss(d, 1) + lambda / 2 |.|^2"""
    rng = np.random.default_rng(3)
    I, U, K = 12, 2, 5
    st = pr.State(rng.normal(0, 0.5, (I, K)), rng.normal(0, 0.5, (I, K)), U, loss=loss, alpha=0.5, lambda_=0.07, bias=bias)
    st.bi[:] = rng.normal(0, 0.3, I)
    rows = np.array([1, 4, 5, 9, 10])
    i, j = 5, 7
    g = pr.grads(st, rows, i, j)

    def numeric(arr, index):
        h = 1e-6
        old = arr[index]
        arr[index] = old + h; up = pr.instance_loss(st, rows, i, j, loss_value)
        arr[index] = old - h; dn = pr.instance_loss(st, rows, i, j, loss_value)
        arr[index] = old
        return (up - dn) / (2 * h)

    assert i not in g["idx"] and g["idx"].size == rows.size - 1
    for r, row in enumerate(g["idx"]):
        for k in range(K):
            assert numeric(st.P, (row, k)) == pytest.approx(g["P"][r, k], rel=1e-6, abs=1e-8)
    assert numeric(st.P, (i, 0)) == 0.0                       # the positive's own row is part of no step
    for k in range(K):
        assert numeric(st.Q, (i, k)) == pytest.approx(g["Qi"][k], rel=1e-6, abs=1e-8)
        assert numeric(st.Q, (j, k)) == pytest.approx(g["Qj"][k], rel=1e-6, abs=1e-8)
    if bias:
        assert numeric(st.bi, i) == pytest.approx(g["bi"], rel=1e-6, abs=1e-8)
        assert numeric(st.bi, j) == pytest.approx(g["bj"], rel=1e-6, abs=1e-8)
    else:
        assert numeric(st.bi, i) == 0.0 and numeric(st.bi, j) == 0.0


def test_the_reference_learns_to_rank_held_out_items():
    """After two epochs on "tiny" at K 16, alpha 0.5, rate 0.1, SQUARE, stream seed 1 the fp64 reference ranks held-out items above
    popularity (Recall@10; measured 0.252 against 0.238 after epoch 2).  LOG at that rate needs three epochs."""
    d = pr.fixture_data("tiny")
    st = pr.init_state(d.num_items, d.num_users, 16, pr.PSEED, alpha=0.5, learn_rate=0.1)
    for ep in range(pr.EPOCHS):
        pr.train(st, d.train_ptr, d.train_col, 1, ep)
    pop = np.bincount(d.train_col, minlength=d.num_items).astype(np.float64)
    r_pop = recall_at_10(lambda u: pop, d)
    r_pair = recall_at_10(lambda u: st.Q @ pr.hidden(st, d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]) + st.bi, d)
    print(f"Recall@10: FISMauc {r_pair:.4f}, popularity {r_pop:.4f}")
    assert r_pair > r_pop


# ---- the grid fixture (fism_ref.grid_*): the premises of tests/test_gpu_model_saturation.py for the pair loop --------------------------
PAIR_CLASSES = ((True, 1), (True, -1))           # a difference beyond +18 and beyond -18 (a pair's label is always 1)


def test_the_grid_cases_are_the_ones_the_gpu_test_names():
    assert set(fr.GRID_PAIR_CASES) == {"sq-ada", "log-ada", "log-sgd", "log-ada-K300", "log-ada-nobias"}
    assert all(h["loss"] in (0, 2) for _, h in fr.GRID_PAIR_CASES.values())


@pytest.mark.parametrize("name", list(fr.GRID_PAIR_CASES))
def test_the_grid_fixture_scores_the_grid_and_stays_within_the_drift_premise(name):
    """The positive of every user's first pair scores its grid point bit for bit (s v . Q[u] + bi[u], in float64 and in float32: the pair's
    difference takes the negative's score off it); over the two epochs the fp64 reference meets differences beyond +18 and beyond -18; and
    the same loop in float32 ends within GRID_BOUND / 4 of it, element by element."""
    from test_fism_reference import assert_grid_premises
    K, hyper = fr.GRID_PAIR_CASES[name]
    ref = pr.grid_reference(name)
    for dtype64 in (True, False):
        assert_grid_premises(fr.grid_first(fr.grid_state(K, hyper, dtype64)), ref.classes, PAIR_CLASSES)
    st32 = fr.grid_run(pr.train, K, hyper, dtype64=False)
    drift = {n: fr.grid_measure(getattr(st32, n), getattr(ref, n)) for n in pr.TABLES}
    print(f"grid pair {name}: max |d| {ref.max_abs_pred:.4g}, classes {ref.classes}, drift " + ", ".join(f"{n} {e:.2e}" for n, e in drift.items()))
    assert max(drift.values()) <= fr.GRID_DRIFT_MAX, drift
    assert ref.max_abs_pred >= 1000.0


@pytest.mark.parametrize("fault", pr.FAULTS)
@pytest.mark.parametrize("name", [n for n, (K, _) in fr.GRID_PAIR_CASES.items() if K == 16])
def test_the_grid_fixture_tells_a_faulty_pair_loop_from_the_right_one(name, fault):
    """each of fism_pair_ref.FAULTS moves some compared table of the grid fixture by at least 10 x GRID_BOUND, element by element"""
    K, hyper = fr.GRID_PAIR_CASES[name]
    right = pr.grid_reference(name)
    wrong = fr.grid_run(pr.train, K, hyper, fault=fault)
    dist = {n: fr.grid_measure(getattr(wrong, n), getattr(right, n)) for n in pr.TABLES}
    print(f"grid pair {name}, {fault}: " + ", ".join(f"{n} {e:.2e}" for n, e in dist.items()))
    assert max(dist.values()) >= 10 * fr.GRID_BOUND, dist
