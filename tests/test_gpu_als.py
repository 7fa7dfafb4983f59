"""-m gpu: WRMF fitted by alternating least squares (cdae_hip_create_als, cdae_als_kernels.hpp) against tests/als_ref.py.

The error measure is als_ref.err — max |a - b| / max(1, the row's max |b|) — and the bound the project's MF tolerance 2e-4
(tests/test_gpu_mf.py); the fp32 restatement in numpy already sits up to 1.3e-5 from fp64 (tests/test_als_reference.py).
Measured on an MI355X (profiles/als_measured.txt has every tier): worst single half-step 1.3e-5.
The fixtures: F23 (37 x 23: a single partial block on the item side, a block and a partial one on the user side) and F300 (40 x 300:
nine blocks and a partial one on the item side), each with an empty row, a row with every item and a column rated by one user."""
import ctypes as C
import os

import numpy as np
import pytest

import als_ref as ar
import cdae_amd
from cdae_amd import ALS_ITEMS, ALS_USERS, P_W, P_WU

pytestmark = pytest.mark.gpu

FIXTURES = {"F23": ar.F23(), "F300": ar.F300()}
MEASURED = os.environ.get("CDAE_ALS_MEASURED")          # a file the parity cases append their figures to (tools/als_bench.py reads it)


def make(R, K, steps=3, X=None, Y=None, seed=3, alpha=ar.ALPHA, lam=ar.LAMBDA):
    m = cdae_amd.WRMF(cdae_amd.WRMFConfig(lambda_=lam, scalar=alpha, num_dim=K, cg_steps=steps))
    ptr, col = ar.csr(R)
    m.set_interactions(R.shape[0], R.shape[1], ptr, col)
    m.init_params(seed)
    if X is not None:
        m.set(P_WU, X)
        m.set(P_W, Y)
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ref_side(R, X, Y, side, steps):
    if side == ALS_USERS:
        return ar.half_step(R, X, Y, ar.ALPHA, ar.LAMBDA, steps)
    return ar.half_step(R.T, Y, X, ar.ALPHA, ar.LAMBDA, steps)


@pytest.mark.parametrize("steps", (1, 3))
@pytest.mark.parametrize("K", ar.KS)
@pytest.mark.parametrize("fx", sorted(FIXTURES))
def test_single_half_step_parity(built, fx, K, steps):
    R = FIXTURES[fx]
    X, Y = ar.tables(R, K)
    for side, which, other in ((ALS_USERS, P_WU, P_W), (ALS_ITEMS, P_W, P_WU)):
        m = make(R, K, steps, X, Y)
        m.half_step(side)
        got, want = m.get(which), ref_side(R, X, Y, side, steps)
        e = ar.err(got, want)
        print(f"{fx} side={side} K={K} steps={steps}: {e:.3e}")
        if MEASURED:
            with open(MEASURED, "a") as f:
                f.write(f"{fx} {side} {K} {steps} {e:.6e}\n")
        assert e < ar.BOUND_GPU, (side, e)
        assert np.array_equal(bits(m.get(other)), bits(Y if side == ALS_USERS else X))      # the frozen table is not written
        m.close()


def test_teacher_forced_epochs(built):
    R, K = FIXTURES["F300"], 64
    X, Y = ar.tables(R, K)
    m = make(R, K, 3, X, Y)
    for epoch in range(3):
        for side, which in ((ALS_USERS, P_WU), (ALS_ITEMS, P_W)):
            Xg, Yg = m.get(P_WU), m.get(P_W)                  # the restatement starts from the GPU's own parameters
            m.half_step(side)
            e = ar.err(m.get(which), ref_side(R, Xg, Yg, side, 3))
            print(f"epoch {epoch} side {side}: {e:.3e}")
            assert e < ar.BOUND_GPU, (epoch, side, e)
    m.close()


@pytest.mark.parametrize("K", (10, 64))
def test_every_half_step_lowers_the_objective(built, K):
    R = FIXTURES["F300"]
    m = make(R, K, 3)                                         # init_params: Random() * 0.001
    assert np.abs(m.get(P_WU)).max() <= 0.001 and np.abs(m.get(P_W)).max() <= 0.001
    obj = [ar.objective(R, m.get(P_WU), m.get(P_W), ar.ALPHA, ar.LAMBDA)]
    for _ in range(6):
        for side in (ALS_USERS, ALS_ITEMS):
            m.half_step(side)
            obj.append(ar.objective(R, m.get(P_WU), m.get(P_W), ar.ALPHA, ar.LAMBDA))
    assert len(obj) == 13 and (np.diff(obj) < 0).all(), obj
    m.close()


def test_cg_converges_to_the_solved_system(built):
    K = 8
    for fx, R in sorted(FIXTURES.items()):
        X, Y = ar.tables(R, K)
        for side, which in ((ALS_USERS, P_WU), (ALS_ITEMS, P_W)):
            m = make(R, K, 16, X, Y)
            m.half_step(side)
            want = ar.exact_half_step(R, X, Y, ar.ALPHA, ar.LAMBDA) if side == ALS_USERS else ar.exact_half_step(R.T, Y, X, ar.ALPHA, ar.LAMBDA)
            e = ar.err(m.get(which), want)
            print(f"{fx} side {side}: {e:.3e}")
            assert e < ar.BOUND_GPU, (fx, side, e)
            m.close()


def test_train_epoch_is_the_two_half_steps(built):
    R, K = FIXTURES["F23"], 10
    X, Y = ar.tables(R, K)
    a, b = make(R, K, 3, X, Y), make(R, K, 3, X, Y)
    st = a.train_one_iteration(123, 9)
    assert (st.users, st.batches, st.examples) == (R.shape[0], 2, 0) and st.wall_seconds > 0
    st = a.train_users(5, 1, 0, R.shape[0])                  # the full range is an epoch too
    assert (st.users, st.batches) == (R.shape[0], 2)
    for _ in range(2):
        b.half_step(ALS_USERS)
        b.half_step(ALS_ITEMS)
    for which in (P_WU, P_W):
        assert np.array_equal(bits(a.get(which)), bits(b.get(which)))
    assert a.data_loss(0, 0) == 0.0 and a.penalty_loss() == 0.0
    a.close()
    b.close()


@pytest.mark.parametrize("K", (64, 200))
def test_a_row_does_not_depend_on_its_position(built, K):
    R = FIXTURES["F300"]
    X, Y = ar.tables(R, K)
    perm = np.random.default_rng(9).permutation(R.shape[0])
    a, b = make(R, K, 3, X, Y), make(R[perm], K, 3, X[perm], Y)
    ga, gb = a.gram(ALS_ITEMS), b.gram(ALS_ITEMS)
    assert np.array_equal(bits(ga), bits(gb)) and np.array_equal(bits(ga), bits(a.gram(ALS_ITEMS))) and np.array_equal(bits(ga), bits(ga.T))
    assert ar.err(ga, ar.gram(Y)) < ar.BOUND_GPU
    a.half_step(ALS_USERS)
    b.half_step(ALS_USERS)
    np.testing.assert_array_equal(bits(b.get(P_WU)), bits(a.get(P_WU)[perm]))
    # two calls from the same state: the same bits
    c = make(R, K, 3, X, Y)
    c.half_step(ALS_USERS)
    np.testing.assert_array_equal(bits(c.get(P_WU)), bits(a.get(P_WU)))
    gu = a.gram(ALS_USERS)                                    # 40 rows; the item side's Gram of the next half-step
    assert np.array_equal(bits(gu), bits(c.gram(ALS_USERS))) and ar.err(gu, ar.gram(a.get(P_WU))) < ar.BOUND_GPU
    for m in (a, b, c):
        m.close()


def device_table(m, which, rows):
    """the padded table [rows, row stride] as it lies on the device, read through param_device_ptr with the process's HIP runtime"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    ptr, n = m.param_device_ptr(which)
    out = np.empty((rows, n // rows), dtype=np.float32)
    assert n == rows * m.lib.cdae_hip_row_stride(m.h) and hip.hipMemcpy(out.ctypes.data, ptr, n * 4, 2) == 0      # device to host
    return out


@pytest.mark.parametrize("K", (10, 65, 200, 300))
def test_empty_rows_keep_their_bits_and_pad_lanes_stay_zero(built, K):
    R = FIXTURES["F300"].copy()
    R[:, 7] = 0                                               # an empty column (user 1 no longer has every item)
    X, Y = ar.tables(R, K)
    m = make(R, K, 3, X, Y)
    m.train_one_iteration()
    Xg, Yg = m.get(P_WU), m.get(P_W)
    assert np.array_equal(bits(Xg[0]), bits(X[0])) and np.array_equal(bits(Yg[7]), bits(Y[7]))
    assert not np.array_equal(bits(Xg[2]), bits(X[2])) and not np.array_equal(bits(Yg[5]), bits(Y[5]))
    for which, rows, host in ((P_WU, R.shape[0], Xg), (P_W, R.shape[1], Yg)):
        T = device_table(m, which, rows)
        assert T.shape[1] in (64, 128, 256, 512) and T.shape[1] >= K
        assert np.array_equal(bits(T[:, :K]), bits(host)) and not T[:, K:].any()
    m.close()


def test_solve_rows(built):
    R, K = FIXTURES["F300"], 64
    X, Y = ar.tables(R, K)
    ptr, col = ar.csr(R)
    m = make(R, K, 3, X, Y)
    before = (m.get(P_WU), m.get(P_W))
    got = m.solve_rows(ptr, col, x0=X)
    for which, t in zip((P_WU, P_W), before):                 # the handle's parameters are not written
        assert np.array_equal(bits(m.get(which)), bits(t))
    m.half_step(ALS_USERS)
    np.testing.assert_array_equal(bits(got), bits(m.get(P_WU)))           # an empty row returns its start vector: what the half-step leaves
    m.set(P_WU, X)
    zero = m.solve_rows(ptr, col)
    np.testing.assert_array_equal(bits(zero), bits(m.solve_rows(ptr, col, x0=np.zeros_like(X))))
    assert not zero[0].any() and ar.err(zero, ar.half_step(R, np.zeros_like(X), Y, ar.ALPHA, ar.LAMBDA, 3)) < ar.BOUND_GPU
    one = m.solve_rows(ptr, col, x0=X, cg_steps=1)
    assert ar.err(one, ar.half_step(R, X, Y, ar.ALPHA, ar.LAMBDA, 1)) < ar.BOUND_GPU
    # 33 rows in one call, and as 32 + 1
    p33, c33 = ptr[:34], col[:ptr[33]]
    whole = m.solve_rows(p33, c33, x0=X[:33])
    head = m.solve_rows(ptr[:33], col[:ptr[32]], x0=X[:32])
    tail = m.solve_rows(ptr[32:34] - ptr[32], col[ptr[32]:ptr[33]], x0=X[32:33])
    np.testing.assert_array_equal(bits(whole), bits(np.vstack([head, tail])))
    np.testing.assert_array_equal(bits(whole), bits(got[:33]))
    assert m.solve_rows(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint32)).shape == (0, K)
    # validation: raised before a launch, the handle stays usable
    for bad_col, text in (([3, 2], "not ascending and unique"), ([2, 2], "not ascending and unique"), ([1, 300], "out of range")):
        with pytest.raises(cdae_amd.CDAEError, match=text):
            m.solve_rows(np.array([0, 2], dtype=np.int64), np.array(bad_col, dtype=np.uint32))
    np.testing.assert_array_equal(bits(m.solve_rows(p33, c33, x0=X[:33])), bits(whole))
    fresh = cdae_amd.WRMF(cdae_amd.WRMFConfig(lambda_=ar.LAMBDA, scalar=ar.ALPHA, num_dim=K, cg_steps=3))
    with pytest.raises(cdae_amd.CDAEError, match="cdae_hip_set_interactions first"):
        fresh.solve_rows(p33, c33)
    with pytest.raises(cdae_amd.CDAEError, match="cdae_hip_set_interactions first"):
        fresh.half_step(ALS_USERS)
    fresh.set_interactions(R.shape[0], R.shape[1], ptr, col)
    fresh.set(P_WU, X)
    fresh.set(P_W, Y)
    np.testing.assert_array_equal(bits(fresh.solve_rows(p33, c33, x0=X[:33])), bits(whole))
    imf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=K))
    with pytest.raises(cdae_amd.CDAEError, match="applies to a WRMF handle"):
        cdae_amd.binding._chk(imf.lib, imf.lib.cdae_hip_als_half_step(imf.h, 0))
    for x in (m, fresh, imf):
        x.close()


def test_serving(built):
    R, K = FIXTURES["F300"], 64
    m = make(R, K, 3)
    m.train_one_iteration()
    m.train_one_iteration()
    X, Y = m.get(P_WU).astype(np.float64), m.get(P_W).astype(np.float64)
    S = X @ Y.T
    S[R > 0] = -np.inf
    order = np.argsort(-S, axis=1, kind="stable")
    top = np.take_along_axis(S, order[:, :11], axis=1)
    with np.errstate(invalid="ignore"):
        clear = np.isfinite(top).all(axis=1) & (np.abs(np.diff(top, axis=1)).min(axis=1) > 1e-5)
    assert clear.mean() > 0.8 and not clear[1]               # (user 1 rated everything: nothing to list)
    rec = m.recommend_all(10)
    assert np.array_equal(rec[clear], order[clear, :10].astype(np.uint32))
    # TOPN against held-out rows: the device's metrics are those of its own lists
    rng = np.random.default_rng(4)
    test_rows = [np.sort(rng.choice(np.flatnonzero(R[u] == 0), size=3, replace=False)) if u != 1 else np.zeros(0, dtype=np.int64)
                 for u in range(R.shape[0])]
    tptr = np.r_[0, np.cumsum([t.size for t in test_rows])].astype(np.int64)
    m.set_test_rows(tptr, np.concatenate(test_rows).astype(np.uint32))
    rets, hits, ids = m.eval_topn(10, with_ids=True)
    assert np.array_equal(ids, rec)
    users = [u for u in range(R.shape[0]) if test_rows[u].size]
    recall10 = np.mean([np.isin(test_rows[u], rec[u]).sum() / test_rows[u].size for u in users])
    assert abs(rets[5] - recall10) < 1e-12
    # similar_items: the bits an IMF handle holding the same tables returns
    ptr, col = ar.csr(FIXTURES["F300"][2:])                  # (IMF refuses the empty and the full row)
    imf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, batch_users=1))
    imf.set_interactions(R.shape[0] - 2, R.shape[1], ptr, col)
    imf.init_params(1)
    imf.set(P_W, m.get(P_W))
    q = np.arange(0, 300, 7, dtype=np.uint32)
    ia, sa = m.similar_items(q, 10, metric="cosine", with_scores=True)
    ib, sb = imf.similar_items(q, 10, metric="cosine", with_scores=True)
    assert np.array_equal(ia, ib) and np.array_equal(bits(sa), bits(sb))
    m.close()
    imf.close()


def test_refusals(built):
    R, K = FIXTURES["F23"], 10
    m = make(R, K)
    U = R.shape[0]
    ptr, col = ar.csr(R[2:4])
    every = "a half-step needs every row"
    with pytest.raises(cdae_amd.CDAEError, match=every):
        m.train_users(0, 0, 0, U - 1)
    with pytest.raises(cdae_amd.CDAEError, match=every):
        m.train_users(0, 0, 1, U)
    with pytest.raises(cdae_amd.CDAEError, match=every):
        m.enqueue_users(0, 0, 0, U)
    with pytest.raises(cdae_amd.CDAEError, match=every):
        m.prefetch_users(0, 0, 0, U)
    imf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, batch_users=1))
    big = FIXTURES["F300"][2:]                                # (IMF refuses the empty and the full row)
    iptr, icol = ar.csr(big)
    imf.set_interactions(big.shape[0], big.shape[1], iptr, icol)
    imf.init_params(1)

    def refusal(model, call):
        with pytest.raises(cdae_amd.CDAEError) as e:
            call(model)
        return str(e.value)

    for call in (lambda x: x.get_hidden_values(np.arange(2, dtype=np.uint32)),
                 lambda x: x.recommend_rows(ptr, col, None, 5),
                 lambda x: x.fold_in_rows(ptr, col, None, n_epochs=1),
                 lambda x: x.recommend_user(2, col[:ptr[1]], 5)):
        assert refusal(m, call) == refusal(imf, call)          # the text IMF / BPR handles are refused with
    assert "IMF / BPR" in refusal(m, lambda x: x.get_hidden_values(np.arange(2, dtype=np.uint32)))
    with pytest.raises(cdae_amd.CDAEError, match="side must be"):
        m.half_step(2)
    # (item shards: cdae_hip_multi_create takes a cdae_hip_config and makes CDAE handles, so no entry point can put a WRMF handle into
    # a sharded model; the library's own guard is the `mf` test IMF / BPR handles share)
    m.train_one_iteration()                                   # still usable
    m.close()
    imf.close()


def test_a_second_smaller_data_set(built):
    big, small, K = FIXTURES["F300"], FIXTURES["F23"], 65
    Xb, Yb = ar.tables(big, K)
    Xs, Ys = ar.tables(small, K, seed=5)
    ps, cs = ar.csr(small)

    def run(m):
        out = {}
        m.half_step(ALS_USERS)
        m.half_step(ALS_ITEMS)
        out["X"], out["Y"] = m.get(P_WU), m.get(P_W)
        out["rows"] = m.solve_rows(ps[:6], cs[:ps[5]], x0=Xs[:5])
        out["gram"] = m.gram(ALS_USERS)
        out["rec"] = m.recommend_all(5)
        return out

    m = make(big, K, 3, Xb, Yb)
    pb, cb = ar.csr(big)
    run(m)
    m.solve_rows(pb, cb, x0=Xb)                                # every workspace at the larger size
    m.set_interactions(small.shape[0], small.shape[1], ps, cs)
    m.init_params(3)
    m.set(P_WU, Xs)
    m.set(P_W, Ys)
    got = run(m)
    fresh = make(small, K, 3, Xs, Ys)
    want = run(fresh)
    for name in want:
        assert got[name].shape == want[name].shape and np.array_equal(bits(got[name]), bits(want[name])), name
    m.close()
    fresh.close()
