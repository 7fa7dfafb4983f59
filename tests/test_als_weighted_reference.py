"""CPU: the numpy definition of the WRMF half-step with per-pair confidence weights and of the objective (tests/als_weighted_ref.py)
is checked against itself before the GPU is held to it, and the host header's item-major weight permutation against numpy.

fp32 restatement: every operation in float32 stays within als_ref.BOUND_FP32 = 2.5e-5 of float64 on both fixtures, both sides, every K
of als_ref.KS, at 1 and 3 CG steps, with geometric(0.3) play counts (1 to about 26) as weights, at the four (alpha, lambda) pairs of
als_weighted_ref.PAIRS (measured worst per pair: 3.8e-6, 1.8e-6, 3.3e-8, 1.3e-6).  alpha = 40 is left out: als_weighted_ref says why.
w = 1: the sparse part of A multiplies by 1.0, so it is als_ref.half_step's to the bit; b is sum (1 + alpha) y where the binary form
has (1 + alpha) sum y — the same bits wherever those sums are exact (integer tables: asserted equal), the same to fp64's last digits
on the random tables (asserted under 1e-13)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import als_ref as ar
import als_weighted_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {"F23": ar.F23, "F300": ar.F300}


def sides(R, W, X, Y):
    """side -> (R, W of that side, the table solved, the table frozen)"""
    return {"users": (R, W, X, Y), "items": (R.T, W.T, Y, X)}


@pytest.mark.parametrize("pair", wr.PAIRS, ids=lambda p: f"a{p[0]:g}-l{p[1]:g}")
@pytest.mark.parametrize("fx", sorted(FIXTURES))
def test_fp32_restatement_against_fp64(fx, pair):
    alpha, lam = pair
    R = FIXTURES[fx]()
    W = wr.weights(R)
    assert W[R > 0].min() == 1 and 15 <= W[R > 0].max() <= 40
    worst = 0.0
    for K in ar.KS:
        X, Y = ar.tables(R, K)
        for steps in (1, 3):
            for side, (Rs, Ws, A, B) in sides(R, W, X, Y).items():
                lo = wr.half_step(Rs, Ws, A, B, alpha, lam, steps, np.float32)
                hi = wr.half_step(Rs, Ws, A, B, alpha, lam, steps, np.float64)
                assert lo.dtype == np.float32 and hi.dtype == np.float64
                e = ar.err(lo, hi)
                worst = max(worst, e)
                assert e < ar.BOUND_FP32, (K, steps, side, e)
                empty = Rs.sum(axis=1) == 0
                assert np.array_equal(lo[empty], A[empty])
    print(f"{fx} alpha={alpha} lambda={lam}: worst {worst:.3e}")


def test_unit_weights_are_the_binary_half_step():
    for fx in sorted(FIXTURES):
        R = FIXTURES[fx]()
        ones = np.ones(R.shape)
        for K in (1, 10, 65):
            # integer tables: every sum of b is exact in either order, and everything after b is the same operations
            Xi = np.random.default_rng(5).integers(-2, 3, (R.shape[0], K)).astype(np.float64)
            Yi = np.random.default_rng(6).integers(-2, 3, (R.shape[1], K)).astype(np.float64)
            X, Y = ar.tables(R, K)
            for alpha, lam in wr.PAIRS + ((ar.ALPHA, ar.LAMBDA),):
                for Rs, Ws, A, B in sides(R, ones, Xi, Yi).values():
                    got, want = wr.half_step(Rs, Ws, A, B, alpha, lam, 3), ar.half_step(Rs, A, B, alpha, lam, 3)
                    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (fx, K, alpha)
                for Rs, Ws, A, B in sides(R, ones, X, Y).values():
                    assert ar.err(wr.half_step(Rs, Ws, A, B, alpha, lam, 3), ar.half_step(Rs, A, B, alpha, lam, 3)) < 1e-13


@pytest.mark.parametrize("K", (4, 8))
def test_cg_converges_to_the_solved_weighted_system(K):
    alpha, lam = wr.PAIRS[0]
    for fx in sorted(FIXTURES):
        R = FIXTURES[fx]()
        W = wr.weights(R)
        X, Y = ar.tables(R, K)
        for side, (Rs, Ws, A, B) in sides(R, W, X, Y).items():
            want = wr.exact_half_step(Rs, Ws, A, B, alpha, lam)
            for dtype in (np.float32, np.float64):
                e = ar.err(wr.half_step(Rs, Ws, A, B, alpha, lam, 2 * K, dtype), want)
                print(f"{fx} {side} K={K} {dtype.__name__}: {e:.3e}")
                assert e < ar.BOUND_FP32, (fx, side, dtype, e)


@pytest.mark.parametrize("K", (1, 10, 64))
def test_the_gram_identity_is_the_dense_objective(K):
    for fx in sorted(FIXTURES):
        R = FIXTURES[fx]()
        for W in (np.ones(R.shape), wr.weights(R), np.random.default_rng(2).integers(0, 3, R.shape).astype(np.float64)):
            X, Y = ar.tables(R, K, scale=0.5)
            for alpha, lam in wr.PAIRS:
                dense, gram = wr.objective_dense(R, W, X, Y, alpha, lam), wr.objective_gram(R, W, X, Y, alpha, lam)
                for a, b in zip(dense, gram):
                    assert abs(a - b) <= 1e-11 * abs(a), (fx, K, alpha, a, b)
    # with unit weights the two terms add up to als_ref.objective
    R = ar.F300()
    X, Y = ar.tables(R, 10)
    d, p = wr.objective_dense(R, np.ones(R.shape), X, Y, 5.0, 1.0)
    assert abs(d + p - ar.objective(R, X, Y, 5.0, 1.0)) <= 1e-12 * (d + p)


@pytest.mark.parametrize("K", (10, 64))
def test_every_half_step_lowers_the_weighted_objective(K):
    alpha, lam = wr.PAIRS[0]
    R = ar.F300()
    W = wr.weights(R)
    X, Y = ar.tables(R, K, scale=0.001)
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    obj = [sum(wr.objective_dense(R, W, X, Y, alpha, lam))]
    for _ in range(6):
        X = wr.half_step(R, W, X, Y, alpha, lam, 3)
        obj.append(sum(wr.objective_dense(R, W, X, Y, alpha, lam)))
        Y = wr.half_step(R.T, W.T, Y, X, alpha, lam, 3)
        obj.append(sum(wr.objective_dense(R, W, X, Y, alpha, lam)))
    drops = -np.diff(obj) / np.array(obj[:-1])
    print(f"K={K}: smallest relative drop {drops.min():.3e}")
    assert len(drops) == 12 and (drops > 0).all(), obj


@pytest.mark.parametrize("K", ar.EXACT_KS)
def test_the_exact_weighted_family(K):
    R, Y, kind, _ = ar.exact_family(K)
    W = wr.exact_weights(R, kind)
    want = wr.exact_want(R, W, kind, K)
    ex = kind == ar.EXACT
    assert {float(W[u, np.flatnonzero(R[u])[0]]) for u in np.flatnonzero(ex)} == set(wr.EXACT_WEIGHTS)
    assert set(np.unique(want[ex])) <= {0.0, 0.5, 0.875, 0.96875}
    zero = np.zeros((R.shape[0], K), dtype=np.float32)
    for dtype in (np.float32, np.float64):
        for x0 in (zero, want):
            got = wr.half_step(R, W, x0, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA, 3, dtype)
            assert got.dtype == dtype and np.isfinite(got).all() and np.array_equal(got[ex], want[ex])
    # at the solved point every s is dyadic: the objective by fp32 Grams and dots is the fp64 one exactly
    X = wr.half_step(R, W, zero, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA, 3, np.float32)
    X[~ex] = 0
    lo = wr.objective_gram(R, W, X, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA, np.float32)
    hi = wr.objective_dense(R, W, X, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA)
    assert lo == hi, (lo, hi)


def test_user_major_weights_on_the_item_side_are_an_error_of_order_one():
    """what the item-side cases above are sensitive to: the restatement fed the user-major array where the item-major one belongs"""
    R, W, K = ar.F300(), wr.weights(ar.F300()), 10
    X, Y = ar.tables(R, K)
    wrong = np.zeros(R.T.shape)
    wrong[R.T > 0] = wr.csr_weights(R, W)                       # user-major values poured into the item-major positions
    good = wr.half_step(R.T, W.T, Y, X, *wr.PAIRS[0], 3)
    assert ar.err(wr.half_step(R.T, wrong, Y, X, *wr.PAIRS[0], 3), good) > 100 * ar.BOUND_GPU


# ---- the host header's item-major weights ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "native", "als_weights_cpu.cpp")
    hdr = os.path.join(ROOT, "cdae_amd", "csrc", "cdae_dataset_plan.h")
    out = os.path.join(ROOT, "build", "libcdae_als_weights_cpu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    so = C.CDLL(out)
    so.aw_item_major.argtypes = [C.c_uint64, C.c_uint64] + [C.c_void_p] * 6
    so.aw_item_major.restype = None
    so.aw_check_weights.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    so.aw_check_weights.restype = C.c_size_t
    return so


def test_item_major_weights_are_the_transposed_weights(lib):
    for fx in sorted(FIXTURES):
        R = FIXTURES[fx]()
        U, I = R.shape
        W = wr.weights(R) + 0.25 * np.arange(U)[:, None]               # (no two users of a column share a weight)
        ptr, col = ar.csr(R)
        w = wr.csr_weights(R, W)
        assert w.size == col.size and np.array_equal(w, np.concatenate([W[u, np.flatnonzero(R[u])] for u in range(U)]).astype(np.float32))
        tptr, tcol, tw = np.zeros(I + 1, np.int64), np.zeros(col.size, np.uint32), np.zeros(col.size, np.float32)
        lib.aw_item_major(U, I, ptr.ctypes.data, col.ctypes.data, w.ctypes.data, tptr.ctypes.data, tcol.ctypes.data, tw.ctypes.data)
        want_ptr, want_col = ar.csr(R.T)
        assert np.array_equal(tptr, want_ptr) and np.array_equal(tcol, want_col)
        assert np.array_equal(tw, W.T[R.T > 0].astype(np.float32)) and np.array_equal(tw, wr.csr_weights(R.T, W.T))
        assert not np.array_equal(tw, w)                               # the user-major order is another one
    # no interactions at all
    z = np.zeros(4, np.int64)
    tptr = np.ones(6, np.int64)
    lib.aw_item_major(3, 5, z.ctypes.data, None, None, tptr.ctypes.data, None, None)
    assert not tptr.any()


def test_check_weights(lib):
    buf = C.create_string_buffer(256)
    ok = np.array([0.0, 1.0, 26.0, 3.4e38], dtype=np.float32)
    assert lib.aw_check_weights(ok.ctypes.data, ok.size, buf, 256) == 0
    assert lib.aw_check_weights(None, 0, buf, 256) == 0
    for bad in (-1.0, -0.5, np.nan, np.inf, -np.inf):
        w = ok.copy()
        w[2] = bad
        assert lib.aw_check_weights(w.ctypes.data, w.size, buf, 256) > 0 and b"position 2" in buf.value and b"finite and >= 0" in buf.value
