"""Shared by tests/test_als_reference.py, tests/test_gpu_als.py and tests/test_gpu_als_exact.py: the definition of the WRMF half-step
(include/cdae_hip.h, "WRMF: weighted-regularised matrix factorisation fitted by alternating least squares") in numpy, the two random
fixtures and, at the end, the exact-arithmetic ones.

R is a dense 0/1 matrix [users, items].  The user half-step solves, for every row u with interactions and the item table Y frozen,
    A_u = Y^T Y + alpha * sum_{i in R_u} y_i y_i^T + lambda * I,   b_u = (1 + alpha) * sum_{i in R_u} y_i
by `steps` iterations of conjugate gradients from the current x_u; A_u is never formed.  The item half-step is half_step(R.T, Y, X, ...).
`dtype` is the precision of EVERY operation (np.float32: the fp32 restatement; np.float64: what the GPU is held against)."""
import numpy as np

RS_STOP = 1e-20
ALPHA, LAMBDA = 40.0, 1.0
KS = (1, 10, 64, 65, 128, 200, 256, 300, 512)
BOUND_FP32 = 2.5e-5          # fp32 restatement against fp64 (tests/test_als_reference.py)
BOUND_GPU = 2e-4             # the project's MF tolerance (tests/test_gpu_mf.py)


def gram(T, dtype=np.float64):
    T = np.asarray(T, dtype=dtype)
    return T.T @ T


def solve_row(G, Yu, x, alpha, lam, steps, dtype):
    """CG on one row: Yu the rows of Y the row interacts with (in item order), x the start vector"""
    alpha, lam = dtype(alpha), dtype(lam)

    def A(p):
        return G @ p + alpha * (Yu.T @ (Yu @ p)) + lam * p

    x = x.copy()
    r = (dtype(1) + alpha) * Yu.sum(axis=0, dtype=dtype) - A(x)
    p = r.copy()
    rs = r @ r
    for _ in range(steps):
        if rs < RS_STOP:
            break
        Ap = A(p)
        a = rs / (p @ Ap)
        x = x + a * p
        r = r - a * Ap
        rs_new = r @ r
        p = r + (rs_new / rs) * p
        rs = rs_new
    return x


def half_step(R, X, Y, alpha, lam, steps, dtype=np.float64):
    """-> the new X [rows of R, K]; a row of R without interactions keeps its X"""
    X = np.asarray(X, dtype=dtype)
    Y = np.asarray(Y, dtype=dtype)
    G = gram(Y, dtype)
    out = X.copy()
    for u in range(R.shape[0]):
        idx = np.flatnonzero(R[u])
        if idx.size:
            out[u] = solve_row(G, Y[idx], X[u], alpha, lam, steps, dtype)
    return out


def exact_half_step(R, X, Y, alpha, lam):
    """the half-step's fixed point: np.linalg.solve on the formed systems, fp64"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    G = Y.T @ Y
    out = X.copy()
    for u in range(R.shape[0]):
        idx = np.flatnonzero(R[u])
        if idx.size:
            Yu = Y[idx]
            out[u] = np.linalg.solve(G + alpha * Yu.T @ Yu + lam * np.eye(Y.shape[1]), (1 + alpha) * Yu.sum(axis=0))
    return out


def objective(R, X, Y, alpha, lam):
    """sum_ui c_ui (p_ui - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2) in fp64, c = 1 + alpha R, p = R"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    E = R - X @ Y.T
    return float(((1.0 + alpha * R) * E * E).sum() + lam * ((X * X).sum() + (Y * Y).sum()))


def err(a, b):
    """max |a - b| / max(1, the row's max |b|)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(b).max(axis=1))).max())


def fixture(users, items, density):
    rng = np.random.default_rng(1)
    R = (rng.random((users, items)) < density).astype(np.float64)
    R[0] = 0                     # an empty row
    R[1] = 1                     # a row with every item
    R[:, 5] = 0
    R[1, 5] = 1                  # column 5 rated by user 1 alone
    return R


def F23():
    return fixture(37, 23, 0.2)


def F300():
    return fixture(40, 300, 0.1)


def tables(R, K, seed=2, scale=0.1):
    """uniform(-1, 1) * scale start tables (X [users, K], Y [items, K]) as float32"""
    rng = np.random.default_rng(seed)
    X = (rng.uniform(-1, 1, (R.shape[0], K)) * scale).astype(np.float32)
    Y = (rng.uniform(-1, 1, (R.shape[1], K)) * scale).astype(np.float32)
    return X, Y


def csr(R):
    rows = [np.flatnonzero(r).astype(np.uint32) for r in R]
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    return ptr, (np.concatenate(rows) if rows else np.zeros(0)).astype(np.uint32)


# ---- exact-arithmetic fixtures (tests/test_gpu_als_exact.py; their CPU checks are in tests/test_als_reference.py) -----------------
# Integer Grams.  The slice layout of als_gram_kernel, restated from cdae_als_kernels.hpp: the rows are cut into
# min(32, ceil(rows / 256)) slices (at least one) of ceil(rows / slices) rows rounded up to an even number (two rows per MFMA); slice s
# takes rows [s * per, min((s + 1) * per, rows)), and the fold adds the slices' partial Grams in slice order.
GRAM_SLICES_MAX, GRAM_SLICE_MIN_ROWS = 32, 256
GRAM_K, GRAM_ROWS = 65, (1, 2, 255, 256, 257, 513, 8191, 8193, 8500)
GRAM_OTHER_KS, GRAM_OTHER_ROWS = (1, 200, 300, 512), (257, 8193, 8500)
GRAM_ITEM_SIDE = (8193, 65)                                  # the one case repeated with the rows in the item table
INT_MAX = 3                                                  # entries in [-3, 3]: every partial sum stays below 9 * rows < 2^24


def gram_slices(rows):
    return max(1, min(GRAM_SLICES_MAX, -(-rows // GRAM_SLICE_MIN_ROWS)))


def gram_slice_rows(rows):
    per = -(-rows // gram_slices(rows))
    return (per + 1) & ~1


def gram_layout(rows):
    """-> the number of rows of every slice, in slice order"""
    per = gram_slice_rows(rows)
    return [max(0, min((s + 1) * per, rows) - s * per) for s in range(gram_slices(rows))]


def int_table(rows, K, seed=11):
    """[rows, K] float32 with integer entries in [-INT_MAX, INT_MAX]"""
    return np.random.default_rng(seed).integers(-INT_MAX, INT_MAX + 1, (rows, K)).astype(np.float32)


def int_gram(T):
    """T.astype(int64).T @ T.astype(int64), through the float64 product: every term and sum is an integer far below 2^53, so it is the
    same integers (numpy's int64 matmul takes ten seconds at 8500 x 512; tests/test_als_reference.py holds the two equal)"""
    T = np.asarray(T).astype(np.float64)
    G = T.T @ T
    assert np.array_equal(G, np.rint(G))
    return G.astype(np.int64)


# Rows that CG solves in one step.  3K items, item i the unit vector e_{i mod K}: G = 3 I.  A row that rates at most one copy of each
# component of a set S has b = (1 + alpha) 1_S = 4 1_S and A b = (3 + alpha + lambda) b = 8 b, so from x = 0 the first step is exact in
# fp32 in any summation order: r = b, a = 16 s / 128 s = 1/8, x = 0.5 1_S, r' = 0, rs = 0 — the row stops.  Started at 0.5 1_S the
# residual of product 0 is 4 - (1.5 + 1.5 + 1) = 0 and the row is never live.
EXACT_ALPHA, EXACT_LAMBDA, EXACT_COPIES = 3.0, 2.0, 3
EXACT_KS = (1, 10, 65, 200, 300, 512)
EMPTY, EXACT, GENERIC = 0, 1, 2


def exact_family(K, users=37, seed=7):
    """-> (R [users, 3K] 0/1, Y [3K, K] float32, kind [users], want [users, K] float32).
    kind: row 0 is EMPTY; every third row is GENERIC — several copies of some components, unequal counts (at K = 1: two or three copies
    of the one component), so A has up to three eigenvalues on b's support and CG needs its three steps; the others are EXACT with
    1 .. min(9, K) distinct components, cycling (the four-at-a-time loop and its tails of 1, 2 and 3), one copy each, and one of them
    holds component K - 1 (the last element before the pad).  want: 0.5 1_S on the EXACT rows, zero elsewhere."""
    rng = np.random.default_rng(seed)
    I = EXACT_COPIES * K
    Y = np.zeros((I, K), dtype=np.float32)
    Y[np.arange(I), np.arange(I) % K] = 1
    R = np.zeros((users, I))
    kind = np.full(users, EXACT)
    kind[0] = EMPTY
    kind[3::3] = GENERIC
    want = np.zeros((users, K), dtype=np.float32)
    n_exact = n_generic = 0
    for u in range(1, users):
        if kind[u] == EXACT:
            s = min(1 + n_exact % 9, K)
            S = rng.choice(K, size=s, replace=False)
            if n_exact == 5 and K - 1 not in S:
                S[0] = K - 1
            R[u, S + K * rng.integers(0, EXACT_COPIES, s)] = 1
            want[u, S] = 0.5
            n_exact += 1
        else:
            s = min(2 + n_generic % 5, K)
            S = rng.choice(K, size=s, replace=False)
            for j, c in enumerate(S):
                copies = 1 + (j + n_generic) % 3 if K > 1 else 2 + n_generic % 2
                R[u, c + K * rng.choice(EXACT_COPIES, size=copies, replace=False)] = 1
            n_generic += 1
    return R, Y, kind, want
