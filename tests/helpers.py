"""Shared helpers for the parity tests (test infrastructure)."""
import numpy as np

import cdae_amd
import oracle as orc
from oracle import binding as ob

PARAMS = range(12)


def make_pair(data, *, K=16, B=1, loss=cdae_amd.CROSS_ENTROPY, seed=11, full_output=False, **kw):
    """A HIP model and an oracle that start from the same fp32 parameters."""
    flags = dict(using_adagrad=True, asymmetric=False, user_factor=True, linear=False, scaled=True, tanh=False,
                 linear_function=False)
    hyper = dict(lambda_=0.01, learn_rate=0.1, corruption_ratio=0.5, beta=1.0, num_neg=5, num_corruptions=1)
    for k, v in kw.items():
        (flags if k in flags else hyper)[k] = v
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=loss, batch_users=B, full_output=full_output, **flags, **hyper)
    model = cdae_amd.CDAE(cfg)
    model.reset(data, seed=seed)
    ocfg = orc.OracleConfig(num_dim=K, loss_type=loss, **flags, **hyper)
    o = orc.Oracle(ocfg, data.num_users, data.num_items, data.train_ptr, data.train_col)
    o.init_params(seed)
    sync_oracle_from_gpu(model, o)
    return model, o


def record_measured(name, **values):
    """Developer aid for the bf16 guards: with CDAE_RECORD_MEASURED=<file> every guarded quantity is appended to that file as it is measured
    (one line per call), so that a bound can be set at <= 1.3 x what a full run of the suite actually sees."""
    import os
    path = os.environ.get("CDAE_RECORD_MEASURED")
    if path:
        with open(path, "a") as f:
            f.write(name + " " + " ".join(f"{k}={float(v):.5g}" for k, v in values.items()) + "\n")


def sync_oracle_from_gpu(model, o):
    for which in PARAMS:
        if o.get(which).size:
            o.set(which, model.get(which).astype(np.float64))


def max_param_err(model, o):
    """max over parameters of max|gpu - oracle| / (1e-3 + max|oracle|)"""
    worst, name = 0.0, None
    for which in PARAMS:
        ref = o.get(which)
        if not ref.size:
            continue
        got = model.get(which).astype(np.float64).ravel()
        err = np.abs(got - ref).max() / (1e-3 + np.abs(ref).max())
        if err > worst:
            worst, name = err, which
    return worst, name


# ---- the host layer's own binary cache (src/base/data.hpp Data::write; src/base/io/file.hpp save) -------------------------------
def read_data_cache(path):
    """-> dict(user_names, item_names, users, items, labels) from a cache written by libcf::save(Data) of this repository's
    host layer: magic, columnar tag, the two first-seen dictionaries, then the columns."""
    import struct
    buf = open(path, "rb").read()
    off = 0

    def u64():
        nonlocal off
        v = struct.unpack_from("<Q", buf, off)[0]
        off += 8
        return v
    assert u64() == 0x3145414443464C43, "not a cache of this build"          # "CLFCDAE1"
    assert u64() == 0x324C4F4345414443, "not the columnar format"            # "CDAECOL2"
    assert u64() == 2
    names = []
    for _ in range(2):
        u64(); u64()                         # feature type, dense length
        n = u64()
        grp = []
        for _ in range(n):
            ln = u64()
            grp.append(buf[off:off + ln].decode())
            off += ln
        names.append(grp)
    n, uniform = u64(), u64()
    uniform_label = struct.unpack_from("<d", buf, off)[0]
    off += 8
    users = np.frombuffer(buf, np.uint32, n, off); off += 4 * n
    items = np.frombuffer(buf, np.uint32, n, off); off += 4 * n
    labels = np.full(n, uniform_label) if uniform else np.frombuffer(buf, np.float64, n, off)
    off += 0 if uniform else 8 * n
    assert off == len(buf)
    return dict(user_names=names[0], item_names=names[1], users=users, items=items, labels=labels)


def csr_of(users, items, num_users):
    """uid -> sorted unique item ids (what Data::to_csr / the reference's uid -> {iid -> label} table hold)"""
    key = np.unique(users.astype(np.int64) << 32 | items.astype(np.int64))
    ptr = np.zeros(num_users + 1, np.int64)
    np.add.at(ptr, (key >> 32) + 1, 1)
    return np.cumsum(ptr), (key & 0xFFFFFFFF).astype(np.uint32)


def fnv1a64(*arrays):
    """FNV-1a over the little-endian bytes of the arrays, as src/model/recsys/cdae.hpp logs for the rows it hands to the device"""
    h = 0xcbf29ce484222325
    for a in arrays:
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- exact ranking reference: models whose every score is an integer multiple of a power of two, exact in fp32 in any order ------
SENTINEL = 0xFFFFFFFF          # what a top-k place beyond the user's unrated items holds (include/cdae_hip.h cdae_hip_recommend_all)


def _units(a, unit):
    """a / unit as int64; asserts that every element is a multiple of `unit` (a power of two <= 1)"""
    assert unit > 0 and unit <= 1 and np.log2(unit) == int(np.log2(unit)), unit
    q = np.asarray(a, dtype=np.float64) / unit
    r = np.rint(q)
    assert np.array_equal(q, r), "parameter is not a multiple of the unit"
    return r.astype(np.int64)


def _imatmul(A, B):
    """A @ B.T of int64 matrices through fp64 BLAS, asserted exact (every sum of magnitudes < 2^53)"""
    Af, Bf = A.astype(np.float64), B.astype(np.float64)
    assert (np.abs(Af) @ np.abs(Bf).T).max(initial=0) < 2.0 ** 53
    return np.rint(Af @ Bf.T).astype(np.int64)


def exact_scores(train_ptr, train_col, *, W=None, b=None, Wu=None, bp=None, V=None, uv=None, iv=None, ib=None, ub=None,
                 unit=1.0, saturated_sigmoid=False):
    """-> (Z, S, D, bq) as int64: the hidden rows in units of `unit`, the scores of all items and b' in units of unit^2, the decoder
    in units of `unit`.
    CDAE with linear = 1 (encode_finish_kernel: z = 1 * sum_k W[k] + b + Wu[u], scale 1 at inference): D = W, or V when given
    (asymmetric).  saturated_sigmoid: the default activation on hidden sums that all lie beyond +-18, where it returns exactly 0 or
    1 (activate(), cdae_kernels.hpp) — z then counts in whole units whatever `unit` is, so unit must be 1.
    IMF / BPR (uv given): z = uv, D = iv, b' = ib; ub shifts all scores of a user alike and is left out."""
    if uv is not None:
        Z, D, bq = _units(uv, unit), _units(iv, unit), _units(ib, unit * unit)
        if ub is not None:
            _units(ub, unit * unit)
    else:
        Wq, Wuq, bq0 = _units(W, unit), _units(Wu, unit), _units(b, unit)
        U = Wuq.shape[0]
        ptr = np.asarray(train_ptr, dtype=np.int64)
        col = np.asarray(train_col, dtype=np.int64)
        H, mag = np.zeros_like(Wuq), np.zeros_like(Wuq)
        for u in range(U):
            rows = Wq[col[ptr[u]:ptr[u + 1]]]
            H[u], mag[u] = rows.sum(axis=0), np.abs(rows).sum(axis=0)
        assert (mag + np.abs(bq0) + np.abs(Wuq)).max(initial=0) < 2 ** 24, "the hidden sums are not exact in fp32"
        Z = H + bq0 + Wuq
        if saturated_sigmoid:
            assert unit == 1.0 and (np.abs(Z) > 18).all(), "saturated_sigmoid needs every |h| > 18"
            Z = (Z > 0).astype(np.int64)
        D = Wq if V is None else _units(V, unit)
        bq = _units(bp, unit * unit)
    return Z, _imatmul(Z, D) + bq, D, bq


def assert_fp32_exact(Z, D, bp):
    """The condition on the INPUTS under which a fp32 dot product z . D[j] + b'[j] is exact in every summation order, fused or not:
    all terms are integers (in units of a power of two) and max_j (sum_k |z_k D_jk| + |b'_j|) < 2^24, so no partial sum needs more
    than 24 bits.  Z, D, bp: the integer arrays of exact_scores."""
    for a in (Z, D, bp):
        assert np.asarray(a).dtype == np.int64
    worst = ((np.abs(Z).astype(np.float64) @ np.abs(D).astype(np.float64).T) + np.abs(bp)).max(initial=0)
    assert worst < 2 ** 24, worst


def rank_total_order(S, train_ptr, train_col, topk, rated=None):
    """The documented order of cdae_hip_recommend_all (include/cdae_hip.h): per user the unrated items by descending score, equal
    scores by ascending item id; uint32 [U, topk], places beyond the number of unrated items hold SENTINEL.
    rated: a list with one array of item ids per row of S, instead of the CSR rows."""
    S = np.asarray(S)
    U, I = S.shape
    out = np.full((U, topk), SENTINEL, dtype=np.uint32)
    ids_all = np.arange(I, dtype=np.int64)
    for u in range(U):
        r = np.asarray(rated[u] if rated is not None else train_col[train_ptr[u]:train_ptr[u + 1]], dtype=np.int64)
        keep = np.ones(I, dtype=bool)
        keep[r] = False
        ids, s = ids_all[keep], S[u][keep]
        if ids.size > 4 * topk:                         # only the items at or above the topk-th best score can appear
            thr = np.partition(s, ids.size - topk)[ids.size - topk]
            sel = s >= thr
            ids, s = ids[sel], s[sel]
        order = np.lexsort((ids, -s))[:topk]
        out[u, :order.size] = ids[order]
    return out


def assert_valid_topk(model, data, rec, topk, K, eps=None, users=None, rated=None, Z=None):
    """rec[u] must be a correct top-k of the unrated items under fp64 scores z_u . D[j] + b'[j], up to fp32 noise.
    eps None: the slack test_recommend_matrix_core_path has always used.  eps "derived": per user
    2 (Kc + 2) 2^-24 max_j (sum_k |z_k D_jk| + |b'_j|), Kc the padded contraction length (the row stride of the handle: pad
    columns are zero) — the textbook bound for a fp32 dot product in any order, doubled because two scores are compared; z is the
    fp32 z the device returns, D and b' the fp32 parameters, all taken to fp64.
    users: the user ids of the rows of rec (default all); rated + Z: one item array per row instead of the train rows, and the
    fp32 z a handle returned for those sets."""
    import cdae_amd
    users = np.arange(data.num_users, dtype=np.uint32) if users is None else np.asarray(users, dtype=np.uint32)
    if rated is None:
        Z = model.get_hidden_values(users, seed=0, epoch=0, mode=0)
        rated = [data.train_col[data.train_ptr[u]:data.train_ptr[u + 1]] for u in users]
    assert Z.dtype == np.float32
    Z = Z.astype(np.float64)
    which = cdae_amd.P_V if getattr(model.cfg, "asymmetric", False) else cdae_amd.P_W
    D = model.get(which).astype(np.float64).reshape(data.num_items, -1)[:, :K]
    bp = model.get(cdae_amd.P_BP).astype(np.float64)
    S = Z[:, :K] @ D.T + bp
    if eps is None:
        eps_u = np.full(users.size, 2e-5 * (1.0 + np.abs(S).max()))
    else:
        assert eps == "derived"
        Kc = int(model.lib.cdae_hip_row_stride(model.h))
        assert Kc >= K
        eps_u = 2.0 * (Kc + 2) * 2.0 ** -24 * (np.abs(Z[:, :K]) @ np.abs(D).T + np.abs(bp)).max(axis=1)
    for n in range(users.size):
        ids, e = rec[n], eps_u[n]
        assert len(set(ids.tolist())) == topk and not np.intersect1d(ids, rated[n]).size
        sc = S[n, ids]
        assert np.all(np.diff(sc) <= e), (users[n], sc)                    # descending
        s = S[n].copy()
        s[np.asarray(rated[n], dtype=np.int64)] = -np.inf
        kth = np.sort(s)[::-1][topk - 1]
        assert sc.min() >= kth - e, (users[n], sc.min(), kth)              # nothing better was left out

