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
