"""CPU: the numpy yardstick of tests/test_gpu_score_rows.py (tests/score_rows_ref.py) against the fp64 oracle, so that the expected
values of the GPU tests are not the code under test: scores64 picks, pair by pair, what the oracle's own encode and parameters give
for all items (the dense product oracle_scores of test_gpu_rows.py forms) and what the oracle's recommend reports for the unrated
ones; ranks_of is pinned on a hand-written row with ties."""
import numpy as np
import pytest

import oracle as orc
from oracle.binding import P_B, P_BP, P_V, P_W, P_WU
from score_rows_ref import magnitudes64, ranks_of, row_of_position, scores64

U, I, K = 40, 200, 8


def csr(rows):
    return np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64), (np.concatenate(rows) if rows else np.empty(0)).astype(np.uint32)


@pytest.fixture(scope="module")
def sets():
    rng = np.random.default_rng(3)
    rated = [np.sort(rng.choice(I, int(rng.integers(1, 30)), replace=False)).astype(np.uint32) for _ in range(U)]
    cands = [np.sort(rng.choice(I, int(n), replace=False)).astype(np.uint32) for n in rng.integers(0, 70, U)]
    cands[0] = np.arange(I, dtype=np.uint32)                       # every item, the rated ones among them
    cands[1] = rated[1].copy()                                     # only rated items
    cands[2] = np.empty(0, np.uint32)
    return csr(rated), csr(cands)


@pytest.mark.parametrize("flags", [dict(), dict(tanh=True), dict(asymmetric=True), dict(linear=True)], ids=["sigmoid", "tanh", "asymmetric", "linear"])
def test_scores64_is_the_oracles_score_of_every_pair(built, sets, flags):
    (ptr, col), (cptr, ccol) = sets
    o = orc.Oracle(orc.OracleConfig(num_dim=K, loss_type=5, beta=1.0, **flags), U, I, ptr, col)
    o.init_params(11)
    rng = np.random.default_rng(4)
    o.set(P_BP, rng.normal(0, 0.3, I))
    o.set(P_B, rng.normal(0, 0.3, K))
    wu = rng.normal(0, 0.3, (U, K))
    wu[5] = 0.0                                                    # a row without a user node: a Wu row of zeros that is still added
    o.set(P_WU, wu)
    which = P_V if flags.get("asymmetric") else P_W
    if flags.get("asymmetric"):
        o.set(P_V, rng.normal(0, 0.3, (I, K)))
    z = o.encode(0, 0, 0, np.arange(U, dtype=np.uint32)).reshape(U, K)
    D, bp = o.get(which).reshape(I, K), o.get(P_BP)
    assert np.unique(z[:, 0]).size > 30 and (flags.get("linear") or np.abs(z).max() <= 1.0)
    got = scores64(z, D, bp, cptr, ccol)
    assert got.shape == (cptr[-1],) and got.dtype == np.float64
    S = z @ D.T + bp                                               # all items, as oracle_scores forms them
    r = row_of_position(cptr)
    np.testing.assert_allclose(got, S[r, ccol.astype(np.int64)], rtol=0, atol=1e-13)
    # the oracle's own decode: its recommend reports the score of every unrated item
    for row in (0, 3, 5, 17):
        left = I - int(ptr[row + 1] - ptr[row])
        ids, sc = o.recommend(left, row, row + 1, with_scores=True)
        own = dict(zip(ids[0].tolist(), sc[0].tolist()))
        a, b = cptr[row], cptr[row + 1]
        hit = 0
        for p in range(a, b):
            if int(ccol[p]) in own:
                assert abs(got[p] - own[int(ccol[p])]) <= 1e-12, (row, p)
                hit += 1
        assert hit == np.setdiff1d(ccol[a:b], col[ptr[row]:ptr[row + 1]]).size
    mag = magnitudes64(z, D, bp, cptr, ccol)
    assert (mag >= np.abs(got) - 1e-12).all()
    np.testing.assert_allclose(mag, (np.abs(z) @ np.abs(D).T + np.abs(bp))[r, ccol.astype(np.int64)], rtol=0, atol=1e-13)


def test_ranks_of_on_a_row_with_ties():
    #            ids:  2    5    7    9   11   40  |  1    3   |   | 8
    scores = np.array([1.0, 3.0, 1.0, 3.0, -2.0, 1.0, 0.5, 0.5, 7.0], dtype=np.float32)
    cptr = np.array([0, 6, 8, 8, 9], dtype=np.int64)
    ccol = np.array([2, 5, 7, 9, 11, 40, 1, 3, 8], dtype=np.uint32)
    # row 0: 3.0 (id 5), 3.0 (id 9), then the three 1.0 by id (2, 7, 40), then -2.0; row 1: equal scores by id; row 2 empty; row 3 alone
    want = np.array([2, 0, 3, 1, 5, 4, 0, 1, 0], dtype=np.uint32)
    got = ranks_of(scores, cptr, ccol)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, want)
    # the definition itself: how many candidates of the row precede p
    for a, b in zip(cptr[:-1], cptr[1:]):
        for p in range(a, b):
            before = sum(1 for q in range(a, b) if scores[q] > scores[p] or (scores[q] == scores[p] and ccol[q] < ccol[p]))
            assert got[p] == before
