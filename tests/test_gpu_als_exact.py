"""-m gpu: WRMF (cdae_als_kernels.hpp, cdae_hip_als_solve_rows) on fixtures whose answer is known to the bit, beside the approximate
cases of tests/test_gpu_als.py.  The fixtures and their reasoning are in tests/als_ref.py, their CPU checks in
tests/test_als_reference.py.

1. Integer Grams: tables with entries in [-3, 3], so every product and partial sum is an integer below 2^24 and fp32 is exact in any
   order — G must EQUAL the int64 product at row counts that reach one slice with an odd tail, an even slice, two and three slices
   with an odd last one, the 32-slice cap from both sides, and every Kp tier.  One dropped or doubled row changes an integer.
2. Rows CG solves in one exact step (als_ref.exact_family; alpha = 3, lambda = 2): they must come out as 0.5 1_S to the bit after
   cg_steps = 3 — the row stops at rs = 0 (without the stop the next step is 0 / 0) while generic rows of the same block go on — and
   keep those bits when the solve starts from them.  Generic rows are held to fp64 under the project's 2e-4.
3. The 32 768-row seam of cdae_hip_als_solve_rows: F23's rows tiled past it return the 37-row result tiled, to the bit.
4. Single half-step parity at three more (alpha, lambda) pairs, bound 2e-4 (the fp32 restatement is within 8.7e-7 of fp64 on them).
   With CDAE_ALS_MEASURED set, the figures are appended to the file of that name with ".pairs" added (profiles/als_measured.txt
   has the worst per pair, measured on an MI355X: 1.2e-6, 2.9e-8, 7.5e-7)."""
import functools

import numpy as np
import pytest

import als_ref as ar
import cdae_amd
from cdae_amd import ALS_ITEMS, ALS_USERS, P_W, P_WU
from test_gpu_als import FIXTURES, MEASURED, bits, device_table, make

pytestmark = pytest.mark.gpu

ALPHA, LAMBDA = ar.EXACT_ALPHA, ar.EXACT_LAMBDA


# ---- 1. integer Grams ------------------------------------------------------------------------------------------------------------
def gram_handle(T, side):
    """a handle whose `side` table is T: any valid small interaction set, the other side 8 rows"""
    rows, K = T.shape
    U, I = (rows, 8) if side == ALS_USERS else (8, rows)
    R = np.zeros((U, I))
    for j in range(3):
        R[j % U, j % I] = 1
    m = cdae_amd.WRMF(cdae_amd.WRMFConfig(lambda_=ar.LAMBDA, scalar=ar.ALPHA, num_dim=K, cg_steps=3))
    ptr, col = ar.csr(R)
    m.set_interactions(U, I, ptr, col)
    m.init_params(3)
    m.set(P_WU if side == ALS_USERS else P_W, T)
    return m


GRAM_CASES = ([(ALS_USERS, r, ar.GRAM_K) for r in ar.GRAM_ROWS] + [(ALS_USERS, r, K) for K in ar.GRAM_OTHER_KS for r in ar.GRAM_OTHER_ROWS]
              + [(ALS_ITEMS,) + ar.GRAM_ITEM_SIDE])


@pytest.mark.parametrize("side,rows,K", GRAM_CASES)
def test_integer_gram_is_exact(built, side, rows, K):
    T = ar.int_table(rows, K)
    m = gram_handle(T, side)
    G, want = m.gram(side), ar.int_gram(T)
    bad = np.argwhere(G != want)
    print(f"side={side} rows={rows} K={K} slices={ar.gram_layout(rows)[:2]}..{ar.gram_layout(rows)[-1]}: {len(bad)} entries differ")
    assert G.dtype == np.float32 and G.shape == want.shape == (K, K)
    assert np.array_equal(G, want), (bad[:4], G[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(bits(G), bits(G.T))
    assert np.array_equal(bits(m.gram(side)), bits(G))          # a second call on the same handle: the same bits
    m.close()


# ---- 2. rows CG solves in one exact step, and the stop -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family(K):
    """exact_family(K) with the fp64 three-step result from zero tables, computed once and read-only"""
    R, Y, kind, want = ar.exact_family(K)
    ref = ar.half_step(R, np.zeros((R.shape[0], K)), Y, ALPHA, LAMBDA, 3)
    for a in (R, Y, kind, want, ref):
        a.flags.writeable = False
    return R, Y, kind, want, ref


def start_table(rows, K):
    """zeros, but for the empty row 0: what it holds must come back"""
    X = np.zeros((rows, K), dtype=np.float32)
    X[0] = 1.25 + np.arange(K) % 5
    return X


def check_rows(got, kind, want, ref, start_row0):
    ex, ge = kind == ar.EXACT, kind == ar.GENERIC
    assert np.isfinite(got).all()
    wrong = np.flatnonzero((bits(got[ex]) != bits(want[ex])).any(axis=1))
    assert wrong.size == 0, (np.flatnonzero(ex)[wrong], got[ex][wrong[0]][:12], want[ex][wrong[0]][:12])
    e = ar.err(got[ge], ref[ge])
    print(f"generic rows: {e:.3e}")
    assert e < ar.BOUND_GPU, e
    assert np.array_equal(bits(got[0]), bits(start_row0))


def pad_lanes_are_zero(m, which, rows, host, K):
    T = device_table(m, which, rows)
    assert T.shape[1] in (64, 128, 256, 512) and T.shape[1] >= K
    assert np.array_equal(bits(T[:, :K]), bits(host)) and not T[:, K:].any()


@pytest.mark.parametrize("K", ar.EXACT_KS)
def test_exact_rows_user_side(built, K):
    R, Y, kind, want, ref = family(K)
    U = R.shape[0]
    ge = kind == ar.GENERIC
    X0 = start_table(U, K)
    ptr, col = ar.csr(R)
    m = make(R, K, 3, X0, Y, alpha=ALPHA, lam=LAMBDA)
    from_zero = m.solve_rows(ptr, col)                        # x0 = None
    check_rows(from_zero, kind, want, ref, np.zeros(K, dtype=np.float32))
    m.half_step(ALS_USERS)
    got = m.get(P_WU)
    check_rows(got, kind, want, ref, X0[0])
    assert np.array_equal(bits(got[1:]), bits(from_zero[1:]))
    assert np.array_equal(bits(m.get(P_W)), bits(Y))
    pad_lanes_are_zero(m, P_WU, U, got, K)
    pad_lanes_are_zero(m, P_W, R.shape[1], Y, K)
    # start at the solution: r = 0 at product 0, an exact row is never live and keeps its bits
    ref2 = ar.half_step(R, got, Y, ALPHA, LAMBDA, 3)
    again = m.solve_rows(ptr, col, x0=got)
    check_rows(again, kind, want, ref2, X0[0])
    m.half_step(ALS_USERS)                                    # in place, from the table the first half-step left
    check_rows(m.get(P_WU), kind, want, ref2, X0[0])
    assert np.array_equal(bits(m.get(P_WU)), bits(again))
    assert ar.err(again[ge], ref[ge]) < ar.BOUND_GPU          # the generic rows stay where three steps had put them
    pad_lanes_are_zero(m, P_WU, U, again, K)
    m.close()


@pytest.mark.parametrize("K", ar.EXACT_KS)
def test_exact_rows_item_side(built, K):
    """the roles swapped: the users carry the unit vectors, the 37 items are solved over the host-built item-major CSR"""
    R, Y, kind, want, ref = family(K)
    Rt = np.ascontiguousarray(R.T)                            # [3K users, 37 items]
    Z0 = start_table(Rt.shape[1], K)
    m = make(Rt, K, 3, Y, Z0, alpha=ALPHA, lam=LAMBDA)
    m.half_step(ALS_ITEMS)
    got = m.get(P_W)
    check_rows(got, kind, want, ref, Z0[0])
    assert np.array_equal(bits(m.get(P_WU)), bits(Y))
    pad_lanes_are_zero(m, P_W, Rt.shape[1], got, K)
    pad_lanes_are_zero(m, P_WU, Rt.shape[0], Y, K)
    m.half_step(ALS_ITEMS)                                    # from the solution
    check_rows(m.get(P_W), kind, want, ar.half_step(R, got, Y, ALPHA, LAMBDA, 3), Z0[0])
    m.close()


@pytest.mark.parametrize("K", ar.EXACT_KS)
def test_stopped_rows_and_their_block(built, K):
    R, Y, kind, want, ref = family(K)
    ex, ge = np.flatnonzero(kind == ar.EXACT), np.flatnonzero(kind == ar.GENERIC)
    m = make(R, K, 3, np.zeros((R.shape[0], K), dtype=np.float32), Y, alpha=ALPHA, lam=LAMBDA)
    # a stopped row stages a zero p and does not disturb its neighbours: the generic rows alone, and between exact rows
    alone = m.solve_rows(*ar.csr(R[ge]))
    mixed = m.solve_rows(*ar.csr(R))
    assert ar.err(alone, ref[ge]) < ar.BOUND_GPU and np.array_equal(bits(alone), bits(mixed[ge]))
    order = np.r_[ex[:5], ge[0], ex[5:17], ge[1:4], ex[17:], ge[4:]]      # another interleaving
    assert np.array_equal(bits(m.solve_rows(*ar.csr(R[order]))), bits(mixed[order]))
    # every row of a block stops; then 32 stopped rows and one generic row in a block of its own
    e32 = np.resize(ex, 32)
    out = m.solve_rows(*ar.csr(R[e32]))
    assert np.isfinite(out).all() and np.array_equal(bits(out), bits(want[e32]))
    out = m.solve_rows(*ar.csr(R[np.r_[e32, ge[0]]]))
    assert np.isfinite(out).all() and np.array_equal(bits(out[:32]), bits(want[e32])) and np.array_equal(bits(out[32]), bits(alone[0]))
    # started at their solution the 32 rows are never live
    assert np.array_equal(bits(m.solve_rows(*ar.csr(R[e32]), x0=want[e32])), bits(want[e32]))
    m.close()


# ---- 3. the 32 768-row seam of solve_rows ------------------------------------------------------------------------------------------
SEAM = 32768


@pytest.mark.parametrize("K,extra", ((10, 37 + 5), (300, 37)))
def test_solve_rows_across_the_chunk_seam(built, K, extra):
    R = FIXTURES["F23"]
    X, Y = ar.tables(R, K)
    ptr, col = ar.csr(R)
    m = make(R, K, 3, X, Y)
    n = SEAM + extra
    idx = np.arange(n) % R.shape[0]                           # (a row's result does not depend on its position: tests/test_gpu_als.py)
    assert idx[SEAM] != 0 and n > SEAM                        # the seam falls inside a copy of the 37 rows
    lens = np.diff(ptr)
    nptr = np.r_[0, np.cumsum(lens[idx])].astype(np.int64)
    ncol = np.tile(col, n // R.shape[0] + 1)[:nptr[-1]]
    cut = nptr[SEAM]
    for x0 in (X, None):
        small = m.solve_rows(ptr, col, x0=x0)
        nx0 = None if x0 is None else np.ascontiguousarray(x0[idx])
        whole = m.solve_rows(nptr, ncol, x0=nx0)
        diff = np.flatnonzero((bits(whole) != bits(small[idx])).any(axis=1))
        assert diff.size == 0, (x0 is None, diff[:4], diff.size)
        head = m.solve_rows(nptr[:SEAM + 1], ncol[:cut], x0=None if x0 is None else nx0[:SEAM])
        tail = m.solve_rows(nptr[SEAM:] - cut, ncol[cut:], x0=None if x0 is None else nx0[SEAM:])
        assert np.array_equal(bits(whole), bits(np.vstack([head, tail])))
    m.close()


# ---- 4. other (alpha, lambda) ------------------------------------------------------------------------------------------------------
PAIRS = ((1.0, 0.01), (0.25, 100.0), (8.0, 10.0))


@pytest.mark.parametrize("steps", (1, 3))
@pytest.mark.parametrize("K", (10, 65, 200, 512))
@pytest.mark.parametrize("fx", sorted(FIXTURES))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"a{p[0]:g}-l{p[1]:g}")
def test_single_half_step_parity_at_other_alpha_and_lambda(built, pair, fx, K, steps):
    alpha, lam = pair
    R = FIXTURES[fx]
    X, Y = ar.tables(R, K)
    for side, which, other in ((ALS_USERS, P_WU, P_W), (ALS_ITEMS, P_W, P_WU)):
        m = make(R, K, steps, X, Y, alpha=alpha, lam=lam)
        m.half_step(side)
        want = ar.half_step(R, X, Y, alpha, lam, steps) if side == ALS_USERS else ar.half_step(R.T, Y, X, alpha, lam, steps)
        e = ar.err(m.get(which), want)
        print(f"alpha={alpha} lambda={lam} {fx} side={side} K={K} steps={steps}: {e:.3e}")
        if MEASURED:
            with open(MEASURED + ".pairs", "a") as f:
                f.write(f"{alpha:g} {lam:g} {fx} {side} {K} {steps} {e:.6e}\n")
        assert e < ar.BOUND_GPU, (side, e)
        assert np.array_equal(bits(m.get(other)), bits(Y if side == ALS_USERS else X))
        m.close()
