"""CPU: the fold-in yardstick (tests/fold_in_ref.py) against the unchanged fp64 oracle.

After ONE literal Oracle.step_user from the same parameters the oracle's z, hg and Wu row (and Uu row under linear_function) must equal
the yardstick's step to 1e-12 relative — for every row whose negatives hold no duplicate: in the literal loop a duplicate's second
occurrence sees the row its first occurrence has just stepped, while the fold-in reads frozen rows throughout.

Condition, not measurement: with 20 000 items and rows of 1-12 items a row draws at most 60 negatives, so
P(duplicate) <= 60 * 59 / 2 / 19 988 ~ 9 % for the longest row; at least 3/4 of the rows must qualify, and the assertion says so.
"""
import numpy as np
import pytest

import oracle as orc
from oracle import binding as ob

import fold_in_ref as ref

I, K, R = 20_000, 16, 48
SEED, EPOCH = 5, 2

CONFIGS = {
    "sigmoid": dict(),
    "tanh": dict(tanh=True),
    "linear": dict(linear=True),
    "linear_function": dict(linear_function=True),
    "asymmetric": dict(asymmetric=True),
    "square_sgd": dict(loss_type=ob.LOSS_SQUARE, using_adagrad=False, learn_rate=0.02),
    "two_corruptions": dict(num_corruptions=2),
}


def rows_and_params(cfg, seed):
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(I, int(rng.integers(1, 13)), replace=False)).astype(np.uint32) for _ in range(R)]
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    col = np.concatenate(rows)
    p = {ob.P_W: rng.normal(0, 0.4, (I, K)), ob.P_W_AG: rng.uniform(0.1, 2, (I, K)), ob.P_B: rng.normal(0, 0.3, K),
         ob.P_B_AG: rng.uniform(0.1, 2, K), ob.P_BP: rng.normal(0, 0.3, I), ob.P_BP_AG: rng.uniform(0.1, 2, I),
         ob.P_WU: rng.normal(0, 0.4, (R, K)), ob.P_WU_AG: rng.uniform(0.1, 2, (R, K))}
    if cfg.asymmetric:
        p.update({ob.P_V: rng.normal(0, 0.4, (I, K)), ob.P_V_AG: rng.uniform(0.1, 2, (I, K))})
    if cfg.linear_function:
        p.update({ob.P_UU: rng.normal(1, 0.3, (R, K)), ob.P_UU_AG: rng.uniform(0.1, 2, (R, K))})
    return ptr, col, p


def close(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_literal_step_equals_the_yardstick(built, name):
    cfg = orc.OracleConfig(num_dim=K, **{"loss_type": ob.LOSS_CE, "beta": 1.0, **CONFIGS[name]})
    ptr, col, p = rows_and_params(cfg, seed=len(name))
    o = orc.Oracle(cfg, R, I, ptr, col)
    P = dict(W=p[ob.P_W], b=p[ob.P_B], bp=p[ob.P_BP], V=p.get(ob.P_V))
    ones, small = np.ones((R, K)), np.full((R, K), ref.AG_INIT)
    qualified = checked = 0
    for r in range(R):
        items = col[ptr[r]:ptr[r + 1]]
        for c in range(cfg.num_corruptions):
            neg = o.draw_negatives(SEED, EPOCH, r, c)
            assert neg.size == items.size * cfg.num_neg and not np.isin(neg, items).any()
            checked += 1
            if np.unique(neg).size != neg.size:
                continue
            qualified += 1
            kept = o.draw_inputs(SEED, EPOCH, r, c)
            for which, arr in p.items():                              # the same parameters before every literal step
                o.set(which, arr)
            z, _, _, hg = o.step_user(r, kept, neg)
            node = (p[ob.P_WU][r], p[ob.P_WU_AG][r], p.get(ob.P_UU, ones)[r], p.get(ob.P_UU_AG, small)[r])
            (wu, wa, uu, ua), z_ref, hg_ref = ref.step(cfg, P, items, kept, neg, node)
            assert close(z, z_ref) and close(hg, hg_ref), (name, r, c)
            assert close(o.get(ob.P_WU).reshape(R, K)[r], wu) and close(o.get(ob.P_WU_AG).reshape(R, K)[r], wa), (name, r, c)
            assert not np.array_equal(wu, node[0])                    # (a step was taken)
            if cfg.linear_function:
                assert close(o.get(ob.P_UU).reshape(R, K)[r], uu) and close(o.get(ob.P_UU_AG).reshape(R, K)[r], ua), (name, r, c)
                assert not np.array_equal(uu, node[2])
    assert qualified * 4 >= 3 * checked, (qualified, checked)


def test_the_epoch_loop_chains_the_steps(built):
    """fold_in_row is the steps of (epoch, corruption) in order, each from the node the previous one left; an empty row and
    n_epochs = 0 return the start node"""
    cfg = orc.OracleConfig(num_dim=K, loss_type=ob.LOSS_CE, beta=1.0, num_corruptions=2, linear_function=True)
    ptr, col, p = rows_and_params(cfg, seed=3)
    ptr = np.r_[ptr, ptr[-1]]                                         # one more row, empty
    o = orc.Oracle(cfg, R + 1, I, ptr, col)
    P = dict(W=p[ob.P_W], b=p[ob.P_B], bp=p[ob.P_BP], V=None)
    node = ref.no_node(K)
    want = node
    items = col[ptr[4]:ptr[5]]
    for e in (7, 8):
        for c in (0, 1):
            want, _, _ = ref.step(cfg, P, items, o.draw_inputs(SEED, e, 4, c), o.draw_negatives(SEED, e, 4, c), want)
    got = ref.fold_in_row(o, P, 4, node, SEED, 7, 2)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert all(np.array_equal(a, b) for a, b in zip(ref.fold_in_row(o, P, 4, node, SEED, 7, 0), node))
    assert all(np.array_equal(a, b) for a, b in zip(ref.fold_in_row(o, P, R, node, SEED, 7, 3), node))


# ---- the exactness proof of every fixture tests/test_gpu_fold_in_exact.py runs ---------------------------------------------------------
# A CONDITION, not a measurement: for every (case, row, step) with the real draws, fold_in_ref.exact_step asserts that each
# per-operation result is an fp32 value and that no sum's absolute terms exceed 2^24 units of their common grid; the literal yardstick
# `step` and the float32 step in two other orders (items reversed; the long role's four-way chunk split) must then return the same
# bits.  A case that fails is re-parameterised in fold_in_ref._exact_cases, never exempted.  PROVED is what the GPU file must run.
PROVED = tuple(ref.EXACT_CASES) + ("seam",)
MOST_BITS = {}                        # case -> the most bits any sum of any checked row needs (printed; DESIGN.md §8h quotes a run)


def proved_case(name):
    return ref.seam_case() if name == "seam" else ref.EXACT_CASES[name]


@pytest.mark.parametrize("name", PROVED)
def test_every_exact_fixture_is_exact_in_fp32_in_any_order(built, name):
    case = proved_case(name)
    (cfg, P, _), (ptr, col, uids), start, want, bits = ref.exact_reference(case, prove=True)
    checked = range(ptr.size - 1) if case["check"] is None else case["check"]
    assert set(bits) == set(checked) and cfg.num_corruptions * case["n_epochs"] == 2          # two steps everywhere
    assert cfg.linear and cfg.loss_type == ob.LOSS_SQUARE and not cfg.using_adagrad and cfg.lambda_ != 0
    for v in (cfg.learn_rate, cfg.lambda_, ref.scale_of(cfg)):
        assert np.log2(v) == int(np.log2(v))
    for T in (P["W"], P["V"]):
        if T is not None:
            assert set(np.unique(T)) <= {-1.0, 0.0, 1.0} and (np.count_nonzero(T, axis=1) <= 2).all() and T.any()
    for a in want:                                                    # fp32 values, and the fit moved what the configuration fits
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    rows = np.array(list(checked))
    moved = (want[0][rows] != start[0][rows]).any(axis=1)
    assert moved.any() == cfg.user_factor and (moved.mean() > 0.5 or not cfg.user_factor)      # (a one-item row may sit at y = t)
    assert (want[2][rows] != start[2][rows]).any() == cfg.linear_function
    assert np.array_equal(want[1], start[1]) and np.array_equal(want[3], start[3])            # plain SGD: the accumulators stay
    MOST_BITS[name] = max(bits.values())
    lens = np.diff(ptr)
    worst = max(bits, key=bits.get)
    print(f"\nexact {name}: at most {bits[worst]:.1f} of 24 bits (row {worst}, {lens[worst]} items)")


def test_the_exact_fixtures_cover_what_the_issue_names():
    """every K tier edge, every role seam on both sides, both roles, every start node, duplicates, both corruption edges"""
    C = ref.EXACT_CASES
    assert {c["K"] for n, c in C.items() if n.startswith("sweep")} == {1, 2, 63, 64, 65, 128, 129, 256, 257, 300, 512}
    for neg, (a, b) in {0: (256, 257), 1: (128, 129), 5: (42, 43), 12: (19, 20)}.items():
        assert not ref_is_long(a, neg) and ref_is_long(b, neg)
        hit = [c for c in C.values() if c["fam"].get("num_neg", 5) == neg and {a, b} <= set(c["lens"]) and c["fam"].get("num_items", 977) == 977]
        assert {c["K"] for c in hit} >= {128, 300}, neg
    assert {c["uids"] for c in C.values()} == {"mixed", "guest", "none"}
    lf = [c for c in C.values() if c["fam"].get("linear_function")]
    for uf in (True, False):
        assert {c["K"] for c in lf if c["fam"].get("user_factor", True) == uf and any(ref_is_long(n, 5) for n in c["lens"])} >= {128, 256, 300}
    assert any(c["fam"].get("corruption_ratio") == 0.0 for c in C.values())
    assert any(c["fam"].get("corruption_ratio") == 1.0 and c["fam"].get("scaled") is False for c in C.values())
    dup = [c for n, c in C.items() if n.startswith("dup")]
    assert all(max(c["lens"]) == c["fam"]["num_items"] - 1 for c in dup) and {bool(c["fam"].get("asymmetric")) for c in dup} == {False, True}
    assert any(ref_is_long(max(c["lens"]), c["fam"].get("num_neg", 5)) for c in dup)
    assert any(not ref_is_long(max(c["lens"]), c["fam"].get("num_neg", 5)) for c in dup)
    seam = ref.seam_case()
    lens = np.array(seam["lens"])
    long_rows = [r for r in range(lens.size) if ref_is_long(int(lens[r]), 5)]
    assert long_rows == sorted(ref.SEAM_LONG) and set(long_rows) <= set(seam["check"])
    assert {r - ref.SEAM_CHUNK for r in long_rows if r >= ref.SEAM_CHUNK} == {0, 17, ref.SEAM_R - ref.SEAM_CHUNK - 1}
    assert any(r < ref.SEAM_CHUNK for r in long_rows)                 # the second chunk's slots do not begin the device list


def ref_is_long(n, num_neg):
    """fold_row_is_long (cdae_foldin_kernels.hpp)"""
    return n * (1 + num_neg) > 256
