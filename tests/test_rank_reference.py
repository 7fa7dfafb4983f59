"""The exact-ranking reference of tests/helpers.py (exact_scores, assert_fp32_exact, rank_total_order) checked on the CPU against the
independent fp64 oracles, so that tests/test_gpu_rank_exact.py does not rest on an unverified restatement.

The oracle replays the reference's heap (std::push_heap / sort_heap), whose order INSIDE equal scores is whatever the heap leaves:
on tie-free models its ids must equal the documented total order for every user; on tied models only its score rows can be
compared (ids may differ inside ties, nowhere else)."""
import numpy as np
import pytest

import oracle as orc
from oracle import binding as ob
from helpers import SENTINEL, assert_fp32_exact, exact_scores, rank_total_order

SHAPES = [  # U, I, K, topk, asymmetric
    (50, 977, 8, 10, False),
    (40, 4000, 100, 16, True),
    (24, 20011, 300, 24, False),
    (10, 70001, 64, 17, True),
]


def _rows(rng, U, I, lo=1, hi=40):
    rows = [np.sort(rng.choice(I, size=int(rng.integers(lo, hi)), replace=False)).astype(np.uint32) for _ in range(U)]
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    return ptr, np.concatenate(rows)


def _int_params(rng, U, I, K, asymmetric):
    p = dict(W=rng.integers(-2, 3, (I, K)), b=rng.integers(-3, 4, K), Wu=rng.integers(-3, 4, (U, K)), bp=rng.integers(-4, 5, I))
    if asymmetric:
        p["V"] = rng.integers(-2, 3, (I, K))
    return {k: v.astype(np.float64) for k, v in p.items()}


def _cdae_oracle(U, I, K, asymmetric, ptr, col, p, bp):
    o = orc.Oracle(orc.OracleConfig(num_dim=K, linear=True, asymmetric=asymmetric), U, I, ptr, col)
    o.init_params(1)
    o.set(ob.P_W, p["W"]); o.set(ob.P_B, p["b"]); o.set(ob.P_WU, p["Wu"]); o.set(ob.P_BP, bp)
    if asymmetric:
        o.set(ob.P_V, p["V"])
    return o


@pytest.mark.parametrize("U,I,K,topk,asymmetric", SHAPES)
def test_cdae_oracle_agrees_with_the_total_order(built, U, I, K, topk, asymmetric):
    rng = np.random.default_rng(I + K)
    ptr, col = _rows(rng, U, I)
    p = _int_params(rng, U, I, K, asymmetric)
    Z, S, D, bq = exact_scores(ptr, col, **p)
    assert_fp32_exact(Z, D, bq)
    # tied: integer scores, hundreds of equal ones per user — the score rows agree for every user and place
    ids_o, sc_o = _cdae_oracle(U, I, K, asymmetric, ptr, col, p, p["bp"]).recommend(topk, with_scores=True)
    want = rank_total_order(S, ptr, col, topk)
    np.testing.assert_array_equal(sc_o, np.take_along_axis(S, want.astype(np.int64), axis=1).astype(np.float64))
    np.testing.assert_array_equal(sc_o, np.take_along_axis(S, ids_o.astype(np.int64), axis=1).astype(np.float64))
    assert (np.diff(S, axis=1) == 0).any()                      # (the model is indeed tied)
    # tie-free: b' += item * 2^-20 (fp64 only): the ids agree for ALL users
    tilt = np.arange(I) * 2.0 ** -20
    ids_o = _cdae_oracle(U, I, K, asymmetric, ptr, col, p, p["bp"] + tilt).recommend(topk)
    np.testing.assert_array_equal(ids_o, rank_total_order(S + tilt, ptr, col, topk))


@pytest.mark.parametrize("U,I,K,topk,pairwise", [(50, 977, 8, 10, False), (30, 4000, 100, 16, True), (8, 70001, 64, 24, False)])
def test_mf_oracle_agrees_with_the_total_order(built, U, I, K, topk, pairwise):
    rng = np.random.default_rng(I + K + 1)
    ptr, col = _rows(rng, U, I)
    uv, iv = rng.integers(-3, 4, (U, K)).astype(np.float64), rng.integers(-2, 3, (I, K)).astype(np.float64)
    ub, ib = rng.integers(-50, 51, U).astype(np.float64), rng.integers(-4, 5, I).astype(np.float64)
    Z, S, D, bq = exact_scores(ptr, col, uv=uv, iv=iv, ib=ib, ub=ub)
    assert_fp32_exact(Z, D, bq)

    def oracle(ib_):
        o = orc.MfOracle(orc.MfConfig(num_dim=K, pairwise=pairwise), U, I, ptr, col)
        o.init_params(1)
        o.set(ob.MF_UV, uv); o.set(ob.MF_IV, iv); o.set(ob.MF_UB, ub); o.set(ob.MF_IB, ib_)
        return o
    want = rank_total_order(S, ptr, col, topk)
    ids_o, sc_o = oracle(ib).recommend(topk, with_scores=True)
    np.testing.assert_array_equal(sc_o - ub[:, None], np.take_along_axis(S, want.astype(np.int64), axis=1).astype(np.float64))
    np.testing.assert_array_equal(ids_o, want)                   # this oracle states the total order itself (partial_sort by score, id)
    tilt = np.arange(I) * 2.0 ** -20
    np.testing.assert_array_equal(oracle(ib + tilt).recommend(topk), rank_total_order(S + tilt, ptr, col, topk))


def test_rank_total_order_by_hand():
    # 6 items, scores per user; user 0 rated {1}, user 1 rated {0, 2, 3, 5}, user 2 rated nothing
    S = np.array([[5, 9, 5, 7, 5, 1], [3, 3, 3, 3, 3, 3], [0, 0, 0, 0, 0, 0]], dtype=np.int64)
    ptr, col = np.array([0, 1, 5, 5], dtype=np.int64), np.array([1, 0, 2, 3, 5], dtype=np.uint32)
    got = rank_total_order(S, ptr, col, 4)
    np.testing.assert_array_equal(got, np.array([[3, 0, 2, 4], [1, 4, SENTINEL, SENTINEL], [0, 1, 2, 3]], dtype=np.uint32))
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(rank_total_order(S[:1], None, None, 2, rated=[np.array([3, 0])]), [[1, 2]])
    # the candidate cut above 4 * topk items changes nothing
    rng = np.random.default_rng(3)
    S = rng.integers(-2, 3, (7, 300))
    ptr, col = _rows(rng, 7, 300, 1, 250)
    slow = np.full((7, 5), SENTINEL, dtype=np.uint32)
    for u in range(7):
        cand = sorted(set(range(300)) - set(col[ptr[u]:ptr[u + 1]].tolist()), key=lambda j: (-S[u, j], j))[:5]
        slow[u, :len(cand)] = cand
    np.testing.assert_array_equal(rank_total_order(S, ptr, col, 5), slow)


def test_exact_scores_by_hand_and_its_guards():
    ptr, col = np.array([0, 2, 3], dtype=np.int64), np.array([0, 2, 1], dtype=np.uint32)
    W = np.array([[1, -2], [0, 3], [2, 2]], dtype=np.float64)
    V = np.array([[1, 0], [0, 1], [-1, -1]], dtype=np.float64)
    b, Wu, bp = np.array([1., -1.]), np.array([[0., 1.], [2., 0.]]), np.array([5., 0., -5.])
    Z, S, D, bq = exact_scores(ptr, col, W=W, b=b, Wu=Wu, bp=bp)
    np.testing.assert_array_equal(Z, [[4, 0], [3, 2]])
    np.testing.assert_array_equal(S, [[9, 0, 3], [4, 6, 5]])
    Z, S, D, bq = exact_scores(ptr, col, W=W, b=b, Wu=Wu, bp=bp, V=V)
    np.testing.assert_array_equal(S, [[9, 0, -9], [8, 2, -10]])
    assert_fp32_exact(Z, D, bq)
    # dyadic parameters: the same model scaled by 1/4 (b' by 1/16) has the same integer image
    Z2, S2, _, _ = exact_scores(ptr, col, W=W / 4, b=b / 4, Wu=Wu / 4, bp=bp / 16, V=V / 4, unit=0.25)
    np.testing.assert_array_equal(S2, S)
    with pytest.raises(AssertionError):
        exact_scores(ptr, col, W=W / 8, b=b, Wu=Wu, bp=bp, unit=0.25)       # not a multiple of the unit
    with pytest.raises(AssertionError):
        assert_fp32_exact(Z * 2 ** 23, D, bq)                               # a partial sum would need more than 24 bits
    # the default activation beyond +-18 is exactly 0 / 1
    Z3, S3, _, _ = exact_scores(ptr, col, W=W, b=np.array([40., -40.]), Wu=Wu, bp=bp, saturated_sigmoid=True)
    np.testing.assert_array_equal(Z3, [[1, 0], [1, 0]])
    np.testing.assert_array_equal(S3, [[6, 0, -3], [6, 0, -3]])
    with pytest.raises(AssertionError):
        exact_scores(ptr, col, W=W, b=b, Wu=Wu, bp=bp, saturated_sigmoid=True)
    # IMF / BPR
    Z4, S4, _, _ = exact_scores(ptr, col, uv=Wu, iv=W, ib=bp, ub=np.array([7., -7.]))
    np.testing.assert_array_equal(S4, [[3, 3, -3], [7, 0, -1]])
