"""Shared by tests/test_als_reference.py and tests/test_gpu_als.py: the definition of the WRMF half-step (include/cdae_hip.h,
"WRMF: weighted-regularised matrix factorisation fitted by alternating least squares") in numpy, and the two fixtures.

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
