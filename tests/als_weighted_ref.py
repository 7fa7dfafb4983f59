"""Shared by tests/test_als_weighted_reference.py and tests/test_gpu_als_weighted.py: the WRMF half-step with per-pair confidence
weights (include/cdae_hip.h, cdae_hip_als_set_confidence) and the objective (cdae_hip_als_objective) in numpy.

R is a dense 0/1 matrix [users, items] and W a dense matrix of the same shape whose entries on R's support are the weights (finite,
>= 0; entries off the support are ignored).  A stored pair has preference 1 and confidence 1 + alpha * w, everything else preference 0
and confidence 1.  The user half-step solves, for every row u with interactions and the item table Y frozen,
    A_u = Y^T Y + alpha * sum_{i in R_u} w_ui y_i y_i^T + lambda * I,   b_u = sum_{i in R_u} (1 + alpha * w_ui) y_i
by `steps` iterations of conjugate gradients from the current x_u (als_ref.solve_row's loop and stop); the item half-step is
half_step(R.T, W.T, Y, X, ...).  `dtype` is the precision of EVERY operation.

alpha = 40 (als_ref.ALPHA) is NOT in the parity grid.  With weights above 1 the system's condition number grows with alpha * w — at
alpha = 40 and play counts up to 26 the sparse part is a thousand times the Gram — and three fp32 CG steps on it differ from fp64 by
up to 4.3e-4 in numpy alone (counts), 1.6e-4 (log-scaled), 3.6e-5 (weights in {0, 1, 2}): nothing a GPU kernel could be held to, the
same reason the reference's literal train_one_index is not offered (include/cdae_hip.h).  The grid below stays under 3.8e-6."""
import numpy as np

from als_ref import F23, F300, csr, err, exact_family, tables  # noqa: F401  (re-exported for the two test files)
import als_ref as ar

PAIRS = ((5.0, 1.0), (1.0, 0.01), (0.25, 100.0), (8.0, 10.0))          # (alpha, lambda) of the parity grid
EXACT_WEIGHTS = (1.0, 9.0, 41.0)                                       # alpha = 3, lambda = 2: x = (1 + 3w) / (5 + 3w) on S
EXACT_VALUES = {1.0: 0.5, 9.0: 0.875, 41.0: 0.96875}
OBJECTIVE_KS = (1, 65, 200, 512)


def weights(R, seed=21):
    """geometric(0.3) play counts, 1 to about 26, on every cell (read on R's support only)"""
    return np.random.default_rng(seed).geometric(0.3, R.shape).astype(np.float64)


def csr_weights(R, W):
    """the weights of the stored pairs in the order of als_ref.csr(R)'s col"""
    return np.ascontiguousarray(W[R > 0], dtype=np.float32)


def solve_row(G, Yu, wu, x, alpha, lam, steps, dtype):
    alpha, lam = dtype(alpha), dtype(lam)
    wu = wu.astype(dtype)

    def A(p):
        return G @ p + alpha * (Yu.T @ (wu * (Yu @ p))) + lam * p

    x = x.copy()
    r = ((dtype(1) + alpha * wu)[:, None] * Yu).sum(axis=0, dtype=dtype) - A(x)
    p = r.copy()
    rs = r @ r
    for _ in range(steps):
        if rs < ar.RS_STOP:
            break
        Ap = A(p)
        a = rs / (p @ Ap)
        x = x + a * p
        r = r - a * Ap
        rs_new = r @ r
        p = r + (rs_new / rs) * p
        rs = rs_new
    return x


def half_step(R, W, X, Y, alpha, lam, steps, dtype=np.float64):
    """-> the new X [rows of R, K]; a row of R without interactions keeps its X"""
    X = np.asarray(X, dtype=dtype)
    Y = np.asarray(Y, dtype=dtype)
    G = ar.gram(Y, dtype)
    out = X.copy()
    for u in range(R.shape[0]):
        idx = np.flatnonzero(R[u])
        if idx.size:
            out[u] = solve_row(G, Y[idx], np.asarray(W[u, idx]), X[u], alpha, lam, steps, dtype)
    return out


def exact_half_step(R, W, X, Y, alpha, lam):
    """the half-step's fixed point: np.linalg.solve on the formed weighted systems, fp64"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    G = Y.T @ Y
    out = X.copy()
    for u in range(R.shape[0]):
        idx = np.flatnonzero(R[u])
        if idx.size:
            Yu, wu = Y[idx], W[u, idx]
            out[u] = np.linalg.solve(G + alpha * (Yu.T * wu) @ Yu + lam * np.eye(Y.shape[1]), ((1 + alpha * wu)[:, None] * Yu).sum(axis=0))
    return out


def objective_dense(R, W, X, Y, alpha, lam):
    """-> (data, penalty) in fp64 from the dense users x items product: sum c (p - x . y)^2 with c = 1 + alpha W on R's support, 1
    elsewhere, and lambda (|X|^2 + |Y|^2)"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    E = R - X @ Y.T
    C = 1.0 + alpha * np.where(R > 0, W, 0.0)
    return float((C * E * E).sum()), float(lam * ((X * X).sum() + (Y * Y).sum()))


def objective_gram(R, W, X, Y, alpha, lam, dtype=np.float64):
    """-> (data, penalty) by the Gram identity: <X^T X, Y^T Y>_F + sum over stored pairs of c (1 - s)^2 - s^2, and
    lambda (tr X^T X + tr Y^T Y).  dtype: the precision of the Grams and of the dot products s; every accumulation is fp64 (what the
    library does with dtype = np.float32)."""
    Xd, Yd = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype)
    Gx, Gy = (Xd.T @ Xd).astype(np.float64), (Yd.T @ Yd).astype(np.float64)
    data = float((Gx * Gy).sum())
    for u in range(R.shape[0]):
        idx = np.flatnonzero(R[u])
        if idx.size:
            s = (Yd[idx] @ Xd[u]).astype(np.float64)
            c = 1.0 + alpha * np.asarray(W[u, idx], dtype=np.float64)
            data += float((c * (1.0 - s) ** 2 - s * s).sum())
    return data, float(lam * (np.trace(Gx) + np.trace(Gy)))


def exact_weights(R, kind, seed=3):
    """-> W for als_ref.exact_family's R: every EXACT row one weight from EXACT_WEIGHTS on all its pairs (cycling, so all three occur
    in both 32-row blocks), GENERIC rows mixed weights from the same set per pair."""
    rng = np.random.default_rng(seed)
    W = np.zeros(R.shape)
    n = 0
    for u in range(R.shape[0]):
        if kind[u] == ar.EXACT:
            W[u] = EXACT_WEIGHTS[n % 3]
            n += 1
        else:
            W[u] = rng.choice(EXACT_WEIGHTS, R.shape[1])
    return W


def exact_want(R, W, kind, K):
    """the EXACT rows' solution: (1 + 3w) / (5 + 3w) on the components of the row's items, zero elsewhere (float32, dyadic)"""
    want = np.zeros((R.shape[0], K), dtype=np.float32)
    for u in np.flatnonzero(kind == ar.EXACT):
        idx = np.flatnonzero(R[u])
        want[u, idx % K] = EXACT_VALUES[float(W[u, idx[0]])]
    return want
