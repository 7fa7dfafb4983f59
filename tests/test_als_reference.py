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
