"""-m gpu: WRMF with per-pair confidence weights (cdae_hip_als_set_confidence, cdae_hip_als_solve_rows_weighted) and the objective
(cdae_hip_als_objective) against tests/als_weighted_ref.py.

Half-steps: als_ref.err against the fp64 restatement under the project's MF tolerance 2e-4 (als_ref.BOUND_GPU), on the grid of
tests/test_als_weighted_reference.py — both fixtures, both sides, every K of als_ref.KS, 1 and 3 CG steps, geometric(0.3) play counts as
weights, the four (alpha, lambda) pairs of als_weighted_ref.PAIRS.  The item side is where a weight array left in user-major order shows:
with weights of 1 to 26 it is an error of order 1 (asserted on the restatement in tests/test_als_weighted_reference.py), not of 1e-4.
Exact pins: als_ref.exact_family with one weight from {1, 9, 41} on every pair of an EXACT row; alpha = 3, lambda = 2, G = 3 I give
A b = (5 + 3w) b and b = (1 + 3w) 1_S, so one CG step from zero lands on 0.5, 0.875 or 0.96875 exactly and the row stops at rs = 0.
Objective: relative error of the data term and of the penalty term against fp64.  The bound is ten times the worst error of the fp32
restatement (fp32 Grams and dot products, fp64 accumulation: als_weighted_ref.objective_gram with dtype float32) over the same cases,
computed here on the CPU — the factor covers the matrix cores' other summation order; the GPU's own output plays no part in it.
With CDAE_ALS_WEIGHTED_MEASURED set, every figure is appended to the file of that name (profiles/als_weighted_measured.txt has them)."""
import functools
import os

import numpy as np
import pytest

import als_ref as ar
import als_weighted_ref as wr
import cdae_amd
from cdae_amd import ALS_ITEMS, ALS_USERS, P_W, P_WU
from test_gpu_als import FIXTURES, bits, device_table, make

pytestmark = pytest.mark.gpu

MEASURED = os.environ.get("CDAE_ALS_WEIGHTED_MEASURED")
WEIGHTS = {fx: wr.weights(R) for fx, R in FIXTURES.items()}
ALPHA, LAMBDA = wr.PAIRS[0]


def note(line):
    print(line)
    if MEASURED:
        with open(MEASURED, "a") as f:
            f.write(line + "\n")


def make_w(R, W, K, steps=3, X=None, Y=None, alpha=ALPHA, lam=LAMBDA):
    m = make(R, K, steps, X, Y, alpha=alpha, lam=lam)
    if W is not None:
        m.set_confidence(wr.csr_weights(R, W))
    return m


def ref_side(R, W, X, Y, side, steps, alpha=ALPHA, lam=LAMBDA):
    if side == ALS_USERS:
        return wr.half_step(R, W, X, Y, alpha, lam, steps)
    return wr.half_step(R.T, W.T, Y, X, alpha, lam, steps)


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", (1, 3))
@pytest.mark.parametrize("K", ar.KS)
@pytest.mark.parametrize("fx", sorted(FIXTURES))
def test_single_half_step_parity(built, fx, K, steps):
    R, W = FIXTURES[fx], WEIGHTS[fx]
    X, Y = ar.tables(R, K)
    for alpha, lam in wr.PAIRS:
        for side, which, other in ((ALS_USERS, P_WU, P_W), (ALS_ITEMS, P_W, P_WU)):
            m = make_w(R, W, K, steps, X, Y, alpha, lam)
            m.half_step(side)
            e = ar.err(m.get(which), ref_side(R, W, X, Y, side, steps, alpha, lam))
            note(f"parity {fx} side={side} K={K} steps={steps} alpha={alpha:g} lambda={lam:g}: {e:.3e}")
            assert e < ar.BOUND_GPU, (alpha, lam, side, e)
            assert np.array_equal(bits(m.get(other)), bits(Y if side == ALS_USERS else X))      # the frozen table is not written
            m.close()


@pytest.mark.parametrize("fx", sorted(FIXTURES))
def test_weights_with_zeros(built, fx):
    R, K = FIXTURES[fx], 65
    W = np.random.default_rng(2).integers(0, 3, R.shape).astype(np.float64)
    assert (W[R > 0] == 0).sum() > 10
    X, Y = ar.tables(R, K)
    for side, which in ((ALS_USERS, P_WU), (ALS_ITEMS, P_W)):
        m = make_w(R, W, K, 3, X, Y)
        m.half_step(side)
        e = ar.err(m.get(which), ref_side(R, W, X, Y, side, 3))
        note(f"zeros {fx} side={side} K={K}: {e:.3e}")
        assert e < ar.BOUND_GPU, (side, e)
        m.close()
    # every weight zero: b = sum y, the sparse part of A is gone
    Z = np.zeros(R.shape)
    m = make_w(R, Z, K, 3, X, Y)
    m.half_step(ALS_USERS)
    assert ar.err(m.get(P_WU), ref_side(R, Z, X, Y, ALS_USERS, 3)) < ar.BOUND_GPU
    m.close()


@pytest.mark.parametrize("K", (10, 200))
def test_empty_rows_keep_their_bits_and_pad_lanes_stay_zero(built, K):
    R = FIXTURES["F300"].copy()
    R[:, 7] = 0                                               # an empty column (user 1 no longer has every item)
    W = WEIGHTS["F300"]
    X, Y = ar.tables(R, K)
    m = make_w(R, W, K, 3, X, Y)
    m.train_one_iteration()
    Xg, Yg = m.get(P_WU), m.get(P_W)
    assert np.array_equal(bits(Xg[0]), bits(X[0])) and np.array_equal(bits(Yg[7]), bits(Y[7]))
    assert not np.array_equal(bits(Xg[2]), bits(X[2])) and not np.array_equal(bits(Yg[5]), bits(Y[5]))
    for which, rows, host in ((P_WU, R.shape[0], Xg), (P_W, R.shape[1], Yg)):
        T = device_table(m, which, rows)
        assert T.shape[1] in (64, 256) and np.array_equal(bits(T[:, :K]), bits(host)) and not T[:, K:].any()
    m.close()


@pytest.mark.parametrize("K", (64, 200))
def test_a_row_does_not_depend_on_its_position(built, K):
    R, W = FIXTURES["F300"], WEIGHTS["F300"]
    X, Y = ar.tables(R, K)
    perm = np.random.default_rng(9).permutation(R.shape[0])
    a, b, c = make_w(R, W, K, 3, X, Y), make_w(R[perm], W[perm], K, 3, X[perm], Y), make_w(R, W, K, 3, X, Y)
    for m in (a, b, c):
        m.half_step(ALS_USERS)
    np.testing.assert_array_equal(bits(b.get(P_WU)), bits(a.get(P_WU)[perm]))        # the weights permuted with their users
    np.testing.assert_array_equal(bits(c.get(P_WU)), bits(a.get(P_WU)))              # two calls from the same state
    a.half_step(ALS_ITEMS)
    c.half_step(ALS_ITEMS)
    np.testing.assert_array_equal(bits(c.get(P_W)), bits(a.get(P_W)))
    # 33 = 32 + 1 rows against the rows solved apart
    ptr, col = ar.csr(R)
    w = wr.csr_weights(R, W)
    whole = a.solve_rows_weighted(ptr[:34], col[:ptr[33]], w[:ptr[33]], x0=X[:33])
    head = a.solve_rows_weighted(ptr[:33], col[:ptr[32]], w[:ptr[32]], x0=X[:32])
    tail = a.solve_rows_weighted(ptr[32:34] - ptr[32], col[ptr[32]:ptr[33]], w[ptr[32]:ptr[33]], x0=X[32:33])
    np.testing.assert_array_equal(bits(whole), bits(np.vstack([head, tail])))
    for m in (a, b, c):
        m.close()


def test_set_confidence_none_and_a_second_data_set_restore_binary(built):
    R, W, K = FIXTURES["F300"], WEIGHTS["F300"], 65
    X, Y = ar.tables(R, K)
    ptr, col = ar.csr(R)
    never = make(R, K, 3, X, Y, alpha=ALPHA, lam=LAMBDA)
    never.train_one_iteration()
    want = (never.get(P_WU), never.get(P_W))
    m = make_w(R, W, K, 3, X, Y)
    m.train_one_iteration()
    assert not np.array_equal(bits(m.get(P_WU)), bits(want[0]))                     # the weights were in force
    m.set_confidence(None)
    m.set(P_WU, X)
    m.set(P_W, Y)
    m.train_one_iteration()
    for which, t in zip((P_WU, P_W), want):
        np.testing.assert_array_equal(bits(m.get(which)), bits(t))
    m.set_confidence(None)                                                         # twice is legal
    # weights again, then a new data set: binary
    m.set_confidence(wr.csr_weights(R, W))
    m.set_interactions(R.shape[0], R.shape[1], ptr, col)
    m.init_params(3)
    m.set(P_WU, X)
    m.set(P_W, Y)
    assert m.objective() == make_and_close_objective(R, None, K, X, Y)
    m.train_one_iteration()
    for which, t in zip((P_WU, P_W), want):
        np.testing.assert_array_equal(bits(m.get(which)), bits(t))
    never.close()
    m.close()


def make_and_close_objective(R, W, K, X, Y):
    m = make_w(R, W, K, 3, X, Y)
    out = m.objective()
    m.close()
    return out


# ---- solve_rows_weighted -----------------------------------------------------------------------------------------------------------
def test_solve_rows_weighted(built):
    R, W, K = FIXTURES["F300"], WEIGHTS["F300"], 64
    X, Y = ar.tables(R, K)
    ptr, col = ar.csr(R)
    w = wr.csr_weights(R, W)
    m = make_w(R, W, K, 3, X, Y)
    before = (m.get(P_WU), m.get(P_W))
    got = m.solve_rows_weighted(ptr, col, w, x0=X)
    other = m.solve_rows_weighted(ptr, col, 2 * w, x0=X)                            # the caller's weights, not the handle's
    assert ar.err(other, wr.half_step(R, 2 * W, X, Y, ALPHA, LAMBDA, 3)) < ar.BOUND_GPU and not np.array_equal(bits(other), bits(got))
    null = m.solve_rows_weighted(ptr, col, None, x0=X)                              # w = NULL: solve_rows' bits, on a weighted handle too
    np.testing.assert_array_equal(bits(null), bits(m.solve_rows(ptr, col, x0=X)))
    assert ar.err(null, ar.half_step(R, X, Y, ALPHA, LAMBDA, 3)) < ar.BOUND_GPU
    for which, t in zip((P_WU, P_W), before):                                       # the handle's parameters are not written
        assert np.array_equal(bits(m.get(which)), bits(t))
    m.half_step(ALS_USERS)
    np.testing.assert_array_equal(bits(got), bits(m.get(P_WU)))                     # an empty row returns its start vector
    m.set(P_WU, X)
    zero = m.solve_rows_weighted(ptr, col, w)
    assert not zero[0].any() and ar.err(zero, wr.half_step(R, W, np.zeros_like(X), Y, ALPHA, LAMBDA, 3)) < ar.BOUND_GPU
    one = m.solve_rows_weighted(ptr, col, w, x0=X, cg_steps=1)
    assert ar.err(one, wr.half_step(R, W, X, Y, ALPHA, LAMBDA, 1)) < ar.BOUND_GPU
    e = np.zeros(0, dtype=np.float32)
    assert m.solve_rows_weighted(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint32), e).shape == (0, K)
    # validation: raised before a launch, the handle stays usable
    two = np.array([0, 2], dtype=np.int64)
    for bad_col, text in (([3, 2], "not ascending and unique"), ([2, 2], "not ascending and unique"), ([1, 300], "out of range")):
        with pytest.raises(cdae_amd.CDAEError, match=text):
            m.solve_rows_weighted(two, np.array(bad_col, dtype=np.uint32), np.ones(2, dtype=np.float32))
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(cdae_amd.CDAEError, match="finite and >= 0"):
            m.solve_rows_weighted(two, np.array([1, 2], dtype=np.uint32), np.array([1.0, bad], dtype=np.float32))
    with pytest.raises(ValueError):
        m.solve_rows_weighted(two, np.array([1, 2], dtype=np.uint32), np.ones(3, dtype=np.float32))
    np.testing.assert_array_equal(bits(m.solve_rows_weighted(ptr, col, w, x0=X)), bits(got))
    fresh = cdae_amd.WRMF(cdae_amd.WRMFConfig(lambda_=LAMBDA, scalar=ALPHA, num_dim=K, cg_steps=3))
    with pytest.raises(cdae_amd.CDAEError, match="cdae_hip_set_interactions first"):
        fresh.solve_rows_weighted(ptr, col, w)
    imf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=K))
    with pytest.raises(cdae_amd.CDAEError, match="applies to a WRMF handle"):
        cdae_amd.binding._chk(imf.lib, imf.lib.cdae_hip_als_solve_rows_weighted(imf.h, 0, None, None, None, None, 0, None))
    for x in (m, fresh, imf):
        x.close()


SEAM = 32768


def test_solve_rows_weighted_across_the_chunk_seam(built):
    R, W, K = FIXTURES["F23"], WEIGHTS["F23"], 10
    X, Y = ar.tables(R, K)
    ptr, col = ar.csr(R)
    w = wr.csr_weights(R, W)
    m = make(R, K, 3, X, Y, alpha=ALPHA, lam=LAMBDA)                                # (a binary handle: the weights are the call's)
    n = SEAM + 37
    idx = np.arange(n) % R.shape[0]
    assert idx[SEAM] != 0
    lens = np.diff(ptr)
    nptr = np.r_[0, np.cumsum(lens[idx])].astype(np.int64)
    reps = n // R.shape[0] + 1
    ncol, nw = np.tile(col, reps)[:nptr[-1]], np.tile(w, reps)[:nptr[-1]]
    small = m.solve_rows_weighted(ptr, col, w, x0=X)
    assert ar.err(small, wr.half_step(R, W, X, Y, ALPHA, LAMBDA, 3)) < ar.BOUND_GPU
    whole = m.solve_rows_weighted(nptr, ncol, nw, x0=np.ascontiguousarray(X[idx]))
    diff = np.flatnonzero((bits(whole) != bits(small[idx])).any(axis=1))
    assert diff.size == 0, (diff[:4], diff.size)
    m.close()


# ---- exact pins ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family(K):
    """als_ref.exact_family(K) with its weights, the exact rows' solution and the fp64 three-step result from zero, read-only"""
    R, Y, kind, _ = ar.exact_family(K)
    W = wr.exact_weights(R, kind)
    want = wr.exact_want(R, W, kind, K)
    ref = wr.half_step(R, W, np.zeros((R.shape[0], K)), Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA, 3)
    for a in (R, Y, kind, W, want, ref):
        a.flags.writeable = False
    return R, Y, kind, W, want, ref


def start_table(rows, K):
    X = np.zeros((rows, K), dtype=np.float32)
    X[0] = 1.25 + np.arange(K) % 5                            # the empty row 0: what it holds must come back
    return X


def check_rows(got, kind, want, ref, row0):
    ex, ge = kind == ar.EXACT, kind == ar.GENERIC
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got[ex], want[ex])
    assert {0.5, 0.875, 0.96875} <= set(np.unique(got[ex])) <= {0.0, 0.5, 0.875, 0.96875}
    e = ar.err(got[ge], ref[ge])
    print(f"generic rows: {e:.3e}")
    assert e < ar.BOUND_GPU, e
    np.testing.assert_array_equal(bits(got[0]), bits(row0))


@pytest.mark.parametrize("K", ar.EXACT_KS)
def test_exact_rows_user_side(built, K):
    R, Y, kind, W, want, ref = family(K)
    U = R.shape[0]
    X0 = start_table(U, K)
    ptr, col = ar.csr(R)
    w = wr.csr_weights(R, W)
    m = make_w(R, W, K, 3, X0, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA)
    from_zero = m.solve_rows_weighted(ptr, col, w)
    check_rows(from_zero, kind, want, ref, np.zeros(K, dtype=np.float32))
    m.half_step(ALS_USERS)
    got = m.get(P_WU)
    check_rows(got, kind, want, ref, X0[0])
    assert np.array_equal(bits(got[1:]), bits(from_zero[1:])) and np.array_equal(bits(m.get(P_W)), bits(Y))
    # started at the solution an exact row is never live
    again = m.solve_rows_weighted(ptr, col, w, x0=got)
    np.testing.assert_array_equal(again[kind == ar.EXACT], want[kind == ar.EXACT])
    m.close()


@pytest.mark.parametrize("K", ar.EXACT_KS)
def test_exact_rows_item_side(built, K):
    """the roles swapped: the users carry the unit vectors, the 37 items are solved over the item-major CSR with the item-major weights"""
    R, Y, kind, W, want, ref = family(K)
    Rt, Wt = np.ascontiguousarray(R.T), np.ascontiguousarray(W.T)
    Z0 = start_table(Rt.shape[1], K)
    m = make_w(Rt, Wt, K, 3, Y, Z0, ar.EXACT_ALPHA, ar.EXACT_LAMBDA)
    m.half_step(ALS_ITEMS)
    check_rows(m.get(P_W), kind, want, ref, Z0[0])
    assert np.array_equal(bits(m.get(P_WU)), bits(Y))
    m.close()


@pytest.mark.parametrize("K", ar.EXACT_KS)
def test_unit_weights_have_the_binary_handles_bits_on_the_exact_family(built, K):
    R, Y, kind, _, _, _ = family(K)
    X0 = start_table(R.shape[0], K)
    Rt = np.ascontiguousarray(R.T)
    Z0 = start_table(Rt.shape[1], K)
    for Rs, A, B, side, which in ((R, X0, Y, ALS_USERS, P_WU), (Rt, Y, Z0, ALS_ITEMS, P_W)):
        a = make_w(Rs, np.ones(Rs.shape), K, 3, A, B, ar.EXACT_ALPHA, ar.EXACT_LAMBDA)
        b = make(Rs, K, 3, A, B, alpha=ar.EXACT_ALPHA, lam=ar.EXACT_LAMBDA)
        a.half_step(side)
        b.half_step(side)
        np.testing.assert_array_equal(bits(a.get(which)), bits(b.get(which)))
        assert a.objective() == b.objective()
        a.close()
        b.close()


# ---- the objective -------------------------------------------------------------------------------------------------------------------
def objective_cases():
    for fx in sorted(FIXTURES):
        for K in wr.OBJECTIVE_KS:
            for weighted in (False, True):
                yield fx, K, weighted


def rel(got, want):
    return max(abs(g - w) / abs(w) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def objective_fp64(fx, K, weighted):
    R = FIXTURES[fx]
    W = WEIGHTS[fx] if weighted else np.ones(R.shape)
    X, Y = ar.tables(R, K)
    return wr.objective_dense(R, W, X, Y, ALPHA, LAMBDA)


@functools.lru_cache(maxsize=None)
def objective_bound():
    """-> (the fp32 restatement's worst relative error over every case, per term; computed on the CPU)"""
    worst = [0.0, 0.0]
    for fx, K, weighted in objective_cases():
        R = FIXTURES[fx]
        W = WEIGHTS[fx] if weighted else np.ones(R.shape)
        X, Y = ar.tables(R, K)
        lo, hi = wr.objective_gram(R, W, X, Y, ALPHA, LAMBDA, np.float32), objective_fp64(fx, K, weighted)
        for t in range(2):
            worst[t] = max(worst[t], abs(lo[t] - hi[t]) / abs(hi[t]))
    assert min(worst) > 0
    return tuple(worst)


@pytest.mark.parametrize("K", wr.OBJECTIVE_KS)
@pytest.mark.parametrize("fx", sorted(FIXTURES))
def test_objective_against_fp64(built, fx, K):
    R = FIXTURES[fx]
    X, Y = ar.tables(R, K)
    restated = objective_bound()
    for weighted in (False, True):
        m = make_w(R, WEIGHTS[fx] if weighted else None, K, 3, X, Y)
        got, want = m.objective(), objective_fp64(fx, K, weighted)
        e = [abs(got[t] - want[t]) / abs(want[t]) for t in range(2)]
        note(f"objective {fx} K={K} weighted={int(weighted)}: data {e[0]:.3e} penalty {e[1]:.3e}; "
             f"fp32 restatement worst: data {restated[0]:.3e} penalty {restated[1]:.3e}, bound = 10 x")
        assert got == m.objective()                                                 # the same state: the same bits
        assert np.array_equal(bits(m.get(P_WU)), bits(X)) and np.array_equal(bits(m.get(P_W)), bits(Y))      # no parameter is written
        assert m.data_loss(0, 0) == 0.0 and m.penalty_loss() == 0.0
        assert e[0] <= 10 * restated[0] and e[1] <= 10 * restated[1], (e, restated)
        m.close()


@pytest.mark.parametrize("K", ar.EXACT_KS)
def test_objective_is_exact_on_the_exact_family(built, K):
    R, Y, kind, W, want, _ = family(K)
    X = np.array(want)                                        # the solved point on the EXACT rows, zero elsewhere: every s is dyadic
    m = make_w(R, W, K, 3, X, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA)
    got, dense = m.objective(), wr.objective_dense(R, W, X, Y, ar.EXACT_ALPHA, ar.EXACT_LAMBDA)
    assert got[0] == dense[0] and got[1] == dense[1], (got, dense)
    m.close()


def test_objective_falls_at_every_half_step(built):
    R, W, K = FIXTURES["F300"], WEIGHTS["F300"], 64
    m = make_w(R, W, K, 3)                                    # init_params: Random() * 0.001
    obj = [sum(m.objective())]
    for _ in range(6):
        for side in (ALS_USERS, ALS_ITEMS):
            m.half_step(side)
            obj.append(sum(m.objective()))
    want = sum(wr.objective_dense(R, W, m.get(P_WU), m.get(P_W), ALPHA, LAMBDA))
    assert len(obj) == 13 and (np.diff(obj) < 0).all(), obj
    assert abs(obj[-1] - want) <= 1e-5 * want
    m.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_weights_in_force(built):
    R, W, K = FIXTURES["F23"], WEIGHTS["F23"], 10
    X, Y = ar.tables(R, K)
    w = wr.csr_weights(R, W)
    m = make_w(R, W, K, 3, X, Y)
    for bad, text in ((w[:-1], "interactions"), (np.r_[w, 1.0], "interactions"), (np.where(np.arange(w.size) == 3, -1.0, w), "finite and >= 0"),
                      (np.where(np.arange(w.size) == 5, np.nan, w), "finite and >= 0"), (np.where(np.arange(w.size) == 0, np.inf, w), "finite and >= 0")):
        with pytest.raises(cdae_amd.CDAEError, match=text):
            m.set_confidence(bad)
    m.half_step(ALS_USERS)                                    # the previous weights are still in force
    good = make_w(R, W, K, 3, X, Y)
    good.half_step(ALS_USERS)
    np.testing.assert_array_equal(bits(m.get(P_WU)), bits(good.get(P_WU)))
    assert m.objective() == good.objective()
    fresh = cdae_amd.WRMF(cdae_amd.WRMFConfig(lambda_=LAMBDA, scalar=ALPHA, num_dim=K, cg_steps=3))
    for call in (lambda: fresh.set_confidence(w), lambda: fresh.objective(), lambda: fresh.set_confidence(None)):
        with pytest.raises(cdae_amd.CDAEError, match="cdae_hip_set_interactions first"):
            call()
    imf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, batch_users=1))
    ptr, col = ar.csr(FIXTURES["F300"][2:])                   # (IMF refuses the empty and the full row)
    imf.set_interactions(38, 300, ptr, col)
    out = np.zeros(2)
    for name, rc in (("cdae_hip_als_set_confidence", lambda: imf.lib.cdae_hip_als_set_confidence(imf.h, None, 0)),
                     ("cdae_hip_als_objective", lambda: imf.lib.cdae_hip_als_objective(imf.h, out.ctypes.data))):
        with pytest.raises(cdae_amd.CDAEError, match=name + " applies to a WRMF handle"):
            cdae_amd.binding._chk(imf.lib, rc())
    for x in (m, good, fresh, imf):
        x.close()
