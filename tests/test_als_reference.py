"""CPU: the numpy definition of the WRMF half-step (tests/als_ref.py) is checked against itself before the GPU is held to it.

fp32 restatement: every operation in float32 stays within 2.5e-5 of the float64 restatement on both fixtures, both sides, every K
tier, at 1 and 3 CG steps (measured: worst 8.3e-7 at one step, 1.3e-5 at three) — which leaves the GPU's different summation order a
factor 8 under the 2e-4 it is asserted at.  Convergence: 2K steps reproduce np.linalg.solve on the formed systems.  Objective: every
half-step of six epochs lowers the weighted objective (smallest relative drop measured: 1.3e-4)."""
import numpy as np
import pytest

import als_ref as ar

FIXTURES = {"F23": ar.F23, "F300": ar.F300}


def sides(R, X, Y):
    """side -> (R of that side, the table solved, the table frozen)"""
    return {"users": (R, X, Y), "items": (R.T, Y, X)}


def test_the_fixtures_have_their_edge_rows():
    for name, (U, I) in (("F23", (37, 23)), ("F300", (40, 300))):
        R = FIXTURES[name]()
        assert R.shape == (U, I) and R[0].sum() == 0 and R[1].sum() == I and R[:, 5].sum() == 1 and R[1, 5] == 1
    assert -(-37 // 32) == 2 and -(-23 // 32) == 1 and 300 // 32 == 9 and 300 % 32       # blocks of 32 rows: partial ones, nine and a partial one


@pytest.mark.parametrize("steps", (1, 3))
@pytest.mark.parametrize("K", ar.KS)
@pytest.mark.parametrize("fx", sorted(FIXTURES))
def test_fp32_restatement_against_fp64(fx, K, steps):
    R = FIXTURES[fx]()
    X, Y = ar.tables(R, K)
    for side, (Rs, A, B) in sides(R, X, Y).items():
        lo = ar.half_step(Rs, A, B, ar.ALPHA, ar.LAMBDA, steps, np.float32)
        hi = ar.half_step(Rs, A, B, ar.ALPHA, ar.LAMBDA, steps, np.float64)
        assert lo.dtype == np.float32 and hi.dtype == np.float64
        e = ar.err(lo, hi)
        print(f"{fx} {side} K={K} steps={steps}: {e:.3e}")
        assert e < ar.BOUND_FP32, (side, e)
        empty = Rs.sum(axis=1) == 0
        assert empty.any() == (side == "users") and np.array_equal(lo[empty], A[empty])


@pytest.mark.parametrize("K", (4, 8))
def test_cg_converges_to_the_solved_system(K):
    for fx in sorted(FIXTURES):
        R = FIXTURES[fx]()
        X, Y = ar.tables(R, K)
        for side, (Rs, A, B) in sides(R, X, Y).items():
            want = ar.exact_half_step(Rs, A, B, ar.ALPHA, ar.LAMBDA)
            for dtype in (np.float32, np.float64):
                e = ar.err(ar.half_step(Rs, A, B, ar.ALPHA, ar.LAMBDA, 2 * K, dtype), want)
                print(f"{fx} {side} K={K} {dtype.__name__}: {e:.3e}")
                assert e < ar.BOUND_FP32, (fx, side, dtype, e)


@pytest.mark.parametrize("K", (10, 64))
def test_every_half_step_lowers_the_objective(K):
    R = ar.F300()
    X, Y = ar.tables(R, K, scale=0.001)
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    obj = [ar.objective(R, X, Y, ar.ALPHA, ar.LAMBDA)]
    for _ in range(6):
        X = ar.half_step(R, X, Y, ar.ALPHA, ar.LAMBDA, 3)
        obj.append(ar.objective(R, X, Y, ar.ALPHA, ar.LAMBDA))
        Y = ar.half_step(R.T, Y, X, ar.ALPHA, ar.LAMBDA, 3)
        obj.append(ar.objective(R, X, Y, ar.ALPHA, ar.LAMBDA))
    drops = -np.diff(obj) / np.array(obj[:-1])
    print(f"K={K}: smallest relative drop {drops.min():.3e}")
    assert len(drops) == 12 and (drops > 0).all(), obj


# ---- the exact-arithmetic fixtures of tests/test_gpu_als_exact.py ---------------------------------------------------------------
def test_integer_gram_fixture_is_exact_and_reaches_every_slice_layout():
    cases = [(r, ar.GRAM_K) for r in ar.GRAM_ROWS] + [(r, K) for K in ar.GRAM_OTHER_KS for r in ar.GRAM_OTHER_ROWS] + [ar.GRAM_ITEM_SIDE]
    for rows, K in cases:
        assert ar.INT_MAX ** 2 * rows < 2 ** 24               # every product and partial sum is an integer fp32 holds: any order is exact
    # (slices, rows of the last slice) by the header's definition; what the row list is there for
    want = {1: (1, 1), 2: (1, 2), 255: (1, 255), 256: (1, 256), 257: (2, 127), 513: (3, 169), 8191: (32, 255), 8193: (32, 195), 8500: (32, 254)}
    assert sorted(want) == sorted(ar.GRAM_ROWS) and set(ar.GRAM_OTHER_ROWS) <= set(want)
    for rows, (slices, last) in want.items():
        lay = ar.gram_layout(rows)
        assert (len(lay), lay[-1]) == (slices, last) and sum(lay) == rows and min(lay) > 0, (rows, lay)
        assert all(n == ar.gram_slice_rows(rows) and n % 2 == 0 for n in lay[:-1]), (rows, lay)
    assert -(-8191 // ar.GRAM_SLICE_MIN_ROWS) == ar.GRAM_SLICES_MAX and -(-8500 // ar.GRAM_SLICE_MIN_ROWS) == 34       # at the cap; two past it
    odd_tail = {r for r in want if want[r][1] % 2}
    assert odd_tail == {1, 255, 257, 513, 8191, 8193} and {len(ar.gram_layout(r)) for r in want} == {1, 2, 3, 32}
    for rows in (1, 255, 257, 8193, 8500):                    # the fp32 product in numpy's order is the integer one
        T = ar.int_table(rows, ar.GRAM_K)
        assert np.abs(T).max() == ar.INT_MAX and np.array_equal(T, np.rint(T))
        Ti = T.astype(np.int64)
        assert np.array_equal(ar.int_gram(T), Ti.T @ Ti) and np.array_equal(ar.gram(T, np.float32), Ti.T @ Ti)


@pytest.mark.parametrize("K", ar.EXACT_KS)
def test_exact_family(K):
    R, Y, kind, want = ar.exact_family(K)
    assert R.shape == (37, 3 * K) and np.array_equal(ar.gram(Y, np.float32), 3 * np.eye(K))
    assert kind[0] == ar.EMPTY and R[0].sum() == 0 and (kind[3::3] == ar.GENERIC).all() and (kind == ar.EXACT).sum() == 24
    comp = R.reshape(37, ar.EXACT_COPIES, K).sum(axis=1)       # copies of every component a row rates
    ex, ge = kind == ar.EXACT, kind == ar.GENERIC
    assert comp[ex].max() == 1 and np.array_equal(0.5 * comp[ex], want[ex]) and not want[~ex].any()
    sizes = comp[ex].sum(axis=1)
    assert set(sizes) == set(range(1, min(9, K) + 1)) and (K < 4 or {0, 1, 2, 3} == set(sizes % 4))
    assert comp[ex][:, K - 1].any()                            # the last real lane element, next to the pad
    assert (comp[ge].max(axis=1) > 1).all() and (K == 1 or all(len(set(c[c > 0])) > 1 for c in comp[ge]))
    if K >= 10:                                                # components in each position of a group of four, without their neighbours
        for pos in (1, 2):
            c = np.arange(pos, K - 2, 4)
            assert (comp[ex][:, c] > comp[ex][:, c + 3 - 2 * pos]).any()
    for blk in (slice(0, 32), slice(32, 37)):                  # exact and generic rows share the 32-row blocks
        assert ex[blk].any() and ge[blk].any()
    zero = np.zeros((37, K), dtype=np.float32)
    for dtype in (np.float32, np.float64):
        for x0 in (zero, want):                                # from zero: one exact step and the stop; from the solution: r = 0 at once
            got = ar.half_step(R, x0, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA, 3, dtype)
            assert got.dtype == dtype and np.isfinite(got).all() and np.array_equal(got[ex], want[ex]) and not got[0].any()
    hi = ar.half_step(R, zero, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA, 3, np.float64)
    e = ar.err(ar.half_step(R, zero, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA, 3, np.float32)[ge], hi[ge])
    assert e < ar.BOUND_FP32 and ar.err(hi[ge], ar.exact_half_step(R, zero, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA)[ge]) < ar.BOUND_FP32, e
    one = ar.half_step(R, zero, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA, 1, np.float64)
    assert K == 1 or ar.err(one[ge], hi[ge]) > ar.BOUND_GPU    # the generic rows need more than the one step


PAIRS = ((1.0, 0.01), (0.25, 100.0), (8.0, 10.0))
PAIR_KS = (10, 65, 200, 512)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"a{p[0]:g}-l{p[1]:g}")
def test_fp32_restatement_against_fp64_at_other_alpha_and_lambda(pair):
    alpha, lam = pair
    worst = 0.0
    for fx in sorted(FIXTURES):
        R = FIXTURES[fx]()
        for K in PAIR_KS:
            X, Y = ar.tables(R, K)
            for steps in (1, 3):
                for side, (Rs, A, B) in sides(R, X, Y).items():
                    e = ar.err(ar.half_step(Rs, A, B, alpha, lam, steps, np.float32), ar.half_step(Rs, A, B, alpha, lam, steps, np.float64))
                    worst = max(worst, e)
                    assert e < ar.BOUND_FP32, (fx, K, steps, side, e)
    print(f"alpha={alpha} lambda={lam}: worst {worst:.3e}")
