"""-m gpu: batched fold-in of user nodes for rows outside the training set (cdae_hip_fold_in_rows) and the guest table that serves
the fitted nodes (cdae_hip_set_guest_nodes, CDAE_GUEST_USER).

Pinned here, on the shapes of tests/test_gpu_rows.py (300 users x 977 items, two epochs of training):
  1. every fitted array against the fp64 yardstick tests/fold_in_ref.py, on rows of both work splits (a wavefront per row up to 42
     items at num_neg = 5, a workgroup per row beyond) including a 976-item row whose every negative is the sampler's linear fallback;
  2. against the device's own training step: a twin handle with batch_users = 1 whose train rows are the foreign rows;
  3. a row's bits do not depend on what else the call holds, and the handle's parameters are not written;
  4. n_epochs = 0 and empty rows return the gathered start nodes exactly;
  5. serving through the guest table: bit identity with a twin handle whose private rows are the returned arrays;
  6. more than one chunk of rows;
  7. every refusal leaves the handle usable and the guest table as it was;
  8. recorded, not asserted: Recall@10 of held-out users with and without fitted nodes, and the wall clock next to the twin-handle loop.
"""
import ctypes as C
import dataclasses
import functools
import time

import numpy as np
import pytest

import cdae_amd
import oracle as orc
from cdae_amd import synth
from helpers import fnv1a64, record_measured
from test_gpu_rows import I_T, NO_USER, U_T, csr, gathered, trained

import fold_in_ref as ref

pytestmark = pytest.mark.gpu

GUEST = cdae_amd.GUEST_USER
AG = np.float32(1e-4)
SEED = 9
LONG_EXAMPLES = 256                  # FOLD_LONG_EXAMPLES (cdae_foldin_kernels.hpp): a row of more examples per step takes a workgroup
LF, TANH, ASYM, NC2 = (("linear_function", True),), (("tanh", True),), (("asymmetric", True),), (("num_corruptions", 2),)
SQ_SGD = (("lt", cdae_amd.SQUARE), ("using_adagrad", False), ("learn_rate", 0.01))
CONFIGS = [(200, ()), (300, ()), (40, LF), (40, TANH), (40, ASYM), (40, SQ_SGD), (40, NC2)]


@functools.lru_cache(maxsize=None)
def model_of(K, flags=()):
    """test_gpu_rows.trained(K, flags); a configuration that names its own loss is trained here the same way"""
    if "lt" not in dict(flags):
        return trained(K, flags)
    d = synth.generate(U_T, I_T, U_T * 40, seed=7, min_items=5)
    m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, beta=1.0, batch_users=64, **dict(flags)))
    m.reset(d, seed=3)
    for ep in range(2):
        m.train_one_iteration(3, ep)
    return m, d


@functools.lru_cache(maxsize=None)
def fold_rows(seed=21):
    """lengths 1, 2, 63, 64, 65, 129, 300 and 976 (one unrated item left: every negative is the linear fallback, all of them
    duplicates), the two lengths either side of the short / long threshold at num_neg = 5, a few more very short rows, then 60
    ordinary rows of 1-60 items; start nodes a mix of real users and NO_USER"""
    rng = np.random.default_rng(seed)
    lens = [1, 2, 63, 64, 65, 129, 300, 976, 42, 43, 3, 4, 5, 6] + [int(rng.integers(1, 61)) for _ in range(60)]
    rows = [np.sort(rng.choice(I_T, n, replace=False)).astype(np.uint32) for n in lens]
    uids = rng.integers(0, U_T, len(rows)).astype(np.uint32)
    uids[rng.random(len(rows)) < 0.35] = NO_USER
    uids[6], uids[7] = 17, NO_USER                   # a long row with a user node, one without
    assert 42 * 6 <= LONG_EXAMPLES < 43 * 6
    return csr(rows) + (uids,)


def oracle_config(cfg):
    return orc.OracleConfig(num_dim=cfg.num_dim, num_neg=cfg.num_neg, num_corruptions=cfg.num_corruptions, loss_type=cfg.lt,
                            using_adagrad=cfg.using_adagrad, asymmetric=cfg.asymmetric, user_factor=cfg.user_factor, linear=cfg.linear,
                            scaled=cfg.scaled, tanh=cfg.tanh, linear_function=cfg.linear_function, lambda_=cfg.lambda_,
                            learn_rate=cfg.learn_rate, corruption_ratio=cfg.corruption_ratio, beta=cfg.beta)


def start_nodes(model, uids, R=None):
    """the four [R, K] float32 arrays a fold-in starts from: copies of the users' rows, zeros / 1e-4 / ones / 1e-4 without a user"""
    K = model.cfg.num_dim
    u = np.full(R, NO_USER, np.uint32) if uids is None else uids
    lf = model.cfg.linear_function
    ones, small = np.ones((len(u), K), np.float32), np.full((len(u), K), AG, np.float32)
    return (gathered(model.get(cdae_amd.P_WU), u, 0.0), gathered(model.get(cdae_amd.P_WU_AG), u, AG),
            gathered(model.get(cdae_amd.P_UU), u, 1.0) if lf else ones, gathered(model.get(cdae_amd.P_UU_AG), u, AG) if lf else small)


def fold_all(model, ptr, col, uids, *, seed=SEED, epoch_begin=0, n_epochs=3, stream_id_base=0, install=False):
    """all four arrays through the C entry point (the Python method returns the ones its configuration fits)"""
    rp, rc, ru = model._rows(ptr, col, uids)
    R, K = rp.size - 1, model.cfg.num_dim
    out = [np.full((R, K), np.nan, np.float32) for _ in range(4)]
    rc_ = model.lib.cdae_hip_fold_in_rows(model.h, R, None if ru is None else ru.ctypes.data, rp.ctypes.data, rc.ctypes.data, seed, epoch_begin,
                                          n_epochs, stream_id_base, int(install), *[a.ctypes.data for a in out])
    if rc_:
        raise cdae_amd.CDAEError(model.lib.cdae_hip_last_error().decode())
    return out


def reference(model, ptr, col, uids, seed, epoch_begin, n_epochs):
    """the fp64 yardstick from the model's fp32 parameters and start nodes"""
    R = ptr.size - 1
    o = orc.Oracle(oracle_config(model.cfg), R, I_T, ptr, col)
    P = dict(W=model.get(cdae_amd.P_W).astype(np.float64), b=model.get(cdae_amd.P_B).astype(np.float64),
             bp=model.get(cdae_amd.P_BP).astype(np.float64), V=model.get(cdae_amd.P_V).astype(np.float64) if model.cfg.asymmetric else None)
    return ref.fold_in(o, P, [a.astype(np.float64) for a in start_nodes(model, uids, R)], seed, epoch_begin, n_epochs)


def same_bits(got, want, msg=""):
    for name, a, b in zip(("wu", "wu_ag", "uu", "uu_ag"), got, want):
        np.testing.assert_array_equal(a, b, err_msg=f"{msg} {name}")


def param_hashes(model):
    ids = [cdae_amd.P_W, cdae_amd.P_W_AG, cdae_amd.P_WU, cdae_amd.P_WU_AG, cdae_amd.P_B, cdae_amd.P_B_AG, cdae_amd.P_BP, cdae_amd.P_BP_AG]
    ids += [cdae_amd.P_V, cdae_amd.P_V_AG] if model.cfg.asymmetric else []
    ids += [cdae_amd.P_UU, cdae_amd.P_UU_AG] if model.cfg.linear_function else []
    return [fnv1a64(model.get(w)) for w in ids]


# ---- 1. against fp64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags", CONFIGS)
def test_against_the_fp64_yardstick(built, K, flags):
    """max|gpu - ref| / (1e-3 + max|ref|) < 2e-4 for each of wu, wu_ag, uu, uu_ag after three epochs: the bound tests/test_gpu_parity.py
    holds two epochs of fp32 AdaGrad to; a node here takes 3-6 steps."""
    model, _ = model_of(K, flags)
    ptr, col, uids = fold_rows()
    lens = np.diff(ptr)
    assert {1, 2, 63, 64, 65, 129, 300, 976} <= set(lens.tolist()) and (uids == NO_USER).any() and (uids != NO_USER).any()
    got = fold_all(model, ptr, col, uids, epoch_begin=2, n_epochs=3)
    want = reference(model, ptr, col, uids, SEED, 2, 3)
    start = start_nodes(model, uids)
    for name, g, w, s0 in zip(("wu", "wu_ag", "uu", "uu_ag"), got, want, start):
        assert np.isfinite(g).all(), name
        err = np.abs(g.astype(np.float64) - w).max() / (1e-3 + np.abs(w).max())
        print(f"K={K} {dict(flags)} {name}: err {err:.3e}, max|ref| {np.abs(w).max():.4g}, moved {np.abs(w - s0).max():.3g}")
        record_measured("fold_in_vs_fp64", K=K, which=("wu", "wu_ag", "uu", "uu_ag").index(name), err=err)
        assert err < 2e-4, (name, err)
    # the fit moved what the configuration fits, and nothing else
    lf = model.cfg.linear_function
    assert np.abs(want[0] - start[0]).max() > 1e-3 and (np.abs(want[2] - start[2]).max() > 1e-3) == lf
    if not lf:
        assert (got[2] == 1).all() and (got[3] == AG).all()
    if model.cfg.using_adagrad:
        assert (got[1] >= start[1]).all() and (got[1] > start[1]).any()        # (a row whose z saturates has delta = 0: it may stay)
    # the Python method returns the arrays of the configuration, the same bits
    py = model.fold_in_rows(ptr, col, uids, seed=SEED, epoch_begin=2, n_epochs=3, with_accumulators=True)
    same_bits(py, got if lf else got[:2], "with_accumulators")
    py = model.fold_in_rows(ptr, col, uids, seed=SEED, epoch_begin=2, n_epochs=3)
    same_bits(py if lf else (py,), (got[0], got[2]) if lf else (got[0],), "method")


# ---- 2. against the device's own training step ---------------------------------------------------------------------------------------
def rows_without_duplicate_negatives(cfg, seed, epoch, lens=(1, 2, 3, 4, 5, 6)):
    """six short rows whose negatives of (seed, epoch, stream id = row index) hold no duplicate: a row is redrawn until that holds"""
    rng = np.random.default_rng(77)
    rows = [np.sort(rng.choice(I_T, n, replace=False)).astype(np.uint32) for n in lens]
    for r in range(len(rows)):
        for _ in range(200):
            o = orc.Oracle(oracle_config(cfg), len(rows), I_T, *csr(rows))
            if all(np.unique(neg).size == neg.size for neg in (o.draw_negatives(seed, epoch, r, c) for c in range(cfg.num_corruptions))):
                break
            rows[r] = np.sort(rng.choice(I_T, lens[r], replace=False)).astype(np.uint32)
        else:
            raise AssertionError("no duplicate-free row found")
    return csr(rows)


@pytest.mark.parametrize("K,flags", [(200, ()), (300, ()), (40, LF), (40, ASYM)])
def test_against_the_training_step_of_a_twin_handle(built, K, flags):
    """train_users(seed, e, r, r + 1) of a batch_users = 1 handle whose train rows are the foreign rows and whose parameters are the
    model's takes the same step as a one-epoch fold-in of row r at stream_id_base = 0: rtol 2e-5, atol 2e-6, test_gpu_parity.py's bound
    for two device paths that take the same step."""
    model, _ = model_of(K, flags)
    cfg = model.cfg
    e = 4
    ptr, col = rows_without_duplicate_negatives(cfg, SEED, e)
    R = ptr.size - 1
    uids = np.array([5, NO_USER, 250, 17, NO_USER, 99], np.uint32)
    start = start_nodes(model, uids)
    got = fold_all(model, ptr, col, uids, epoch_begin=e, n_epochs=1)
    tw = cdae_amd.CDAE(dataclasses.replace(cfg, batch_users=1))
    tw.set_interactions(R, I_T, ptr, col)
    tw.init_params(0)
    shared = [cdae_amd.P_W, cdae_amd.P_W_AG, cdae_amd.P_B, cdae_amd.P_B_AG, cdae_amd.P_BP, cdae_amd.P_BP_AG]
    shared += [cdae_amd.P_V, cdae_amd.P_V_AG] if cfg.asymmetric else []
    saved = {w: model.get(w) for w in shared}
    private = dict(zip((cdae_amd.P_WU, cdae_amd.P_WU_AG, cdae_amd.P_UU, cdae_amd.P_UU_AG), start))
    if not cfg.linear_function:
        del private[cdae_amd.P_UU], private[cdae_amd.P_UU_AG]
    for r in range(R):
        for w, a in {**saved, **private}.items():                     # the twin's parameters are reset between rows
            tw.set(w, a)
        tw.train_users(SEED, e, r, r + 1)
        np.testing.assert_allclose(tw.get(cdae_amd.P_WU)[r], got[0][r], rtol=2e-5, atol=2e-6, err_msg=f"Wu row {r}")
        np.testing.assert_allclose(tw.get(cdae_amd.P_WU_AG)[r], got[1][r], rtol=2e-5, atol=2e-6, err_msg=f"Wu_ag row {r}")
        assert np.abs(got[0][r] - start[0][r]).max() > 1e-4
        if cfg.linear_function:
            np.testing.assert_allclose(tw.get(cdae_amd.P_UU)[r], got[2][r], rtol=2e-5, atol=2e-6, err_msg=f"Uu row {r}")
            np.testing.assert_allclose(tw.get(cdae_amd.P_UU_AG)[r], got[3][r], rtol=2e-5, atol=2e-6, err_msg=f"Uu_ag row {r}")
    tw.close()


# ---- 3. a function of the row alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags", [(200, ()), (40, LF)])
def test_a_row_alone_returns_the_bits_it_gets_in_the_full_call(built, K, flags):
    model, _ = model_of(K, flags)
    ptr, col, uids = fold_rows()
    before = param_hashes(model)
    full = fold_all(model, ptr, col, uids, epoch_begin=1, n_epochs=3)
    lens = np.diff(ptr[:21])
    assert (lens * 6 > LONG_EXAMPLES).any() and (lens * 6 <= LONG_EXAMPLES).any()       # both work splits among the first 20 rows
    for r in range(20):
        row = col[ptr[r]:ptr[r + 1]]
        alone = fold_all(model, np.array([0, row.size], np.int64), row, uids[r:r + 1], epoch_begin=1, n_epochs=3, stream_id_base=r)
        same_bits(alone, [a[r:r + 1] for a in full], f"row {r} alone")
    # somewhere else in a call, among other rows: rows 8.. moved to the front, the stream ids following them
    back = fold_all(model, ptr[8:] - ptr[8], col[ptr[8]:], uids[8:], epoch_begin=1, n_epochs=3, stream_id_base=8)
    same_bits(back, [a[8:] for a in full], "rows 8..")
    same_bits(fold_all(model, ptr, col, uids, epoch_begin=1, n_epochs=3), full, "repeat")
    assert param_hashes(model) == before


# ---- 4. start nodes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags", [(200, ()), (40, LF)])
def test_no_epochs_and_empty_rows_return_the_start_nodes(built, K, flags):
    model, _ = model_of(K, flags)
    ptr, col, uids = fold_rows()
    same_bits(fold_all(model, ptr, col, uids, n_epochs=0), start_nodes(model, uids), "n_epochs = 0")
    same_bits(fold_all(model, ptr, col, None, n_epochs=0), start_nodes(model, None, ptr.size - 1), "n_epochs = 0, no uids")
    rows = [col[ptr[r]:ptr[r + 1]] for r in range(12)]
    for r in (0, 3, 7, 11):
        rows[r] = np.empty(0, np.uint32)
    eptr, ecol = csr(rows)
    eu = uids[:12].copy()
    eu[0], eu[3] = 44, NO_USER
    got = fold_all(model, eptr, ecol, eu, n_epochs=3)
    start = start_nodes(model, eu)
    empty = np.diff(eptr) == 0
    same_bits([a[empty] for a in got], [a[empty] for a in start], "empty rows")
    assert (got[0][3] == 0).all() and (got[1][3] == AG).all() and (got[2][3] == 1).all() and (got[3][3] == AG).all()
    assert (got[0][~empty] != start[0][~empty]).any(axis=1).sum() >= 6           # (the others took their steps)


# ---- 5. serving --------------------------------------------------------------------------------------------------------------------
def twin_with_nodes(model, ptr, col, wu, uu):
    """a handle with the model's shared parameters whose TRAIN rows are the caller's rows and whose private rows are the given arrays"""
    cfg = model.cfg
    tw = cdae_amd.CDAE(cfg)
    tw.set_interactions(ptr.size - 1, I_T, ptr, col)
    tw.init_params(0)
    for which in (cdae_amd.P_W, cdae_amd.P_B, cdae_amd.P_BP) + ((cdae_amd.P_V,) if cfg.asymmetric else ()):
        tw.set(which, model.get(which))
    tw.set(cdae_amd.P_WU, wu)
    if cfg.linear_function:
        tw.set(cdae_amd.P_UU, uu)
    return tw


@pytest.mark.parametrize("K,flags", [(200, ()), (300, ()), (40, LF)])
def test_the_guest_table_serves_the_fitted_nodes(built, K, flags):
    model, _ = model_of(K, flags)
    ptr, col, uids = fold_rows()
    R = ptr.size - 1
    rng = np.random.default_rng(31)
    rows = [col[ptr[r]:ptr[r + 1]] for r in range(R)]
    free = [np.setdiff1d(np.arange(I_T, dtype=np.uint32), row) for row in rows]
    tptr, tcol = csr([np.sort(rng.choice(f, min(f.size, (1, 4, 9)[r % 3]), replace=False)).astype(np.uint32) for r, f in enumerate(free)])
    cptr, ccol = csr([np.sort(rng.choice(I_T, 20, replace=False)).astype(np.uint32) for _ in range(R)])
    model.set_guest_nodes(np.zeros((0, K), np.float32))
    assert model.num_guest_nodes == 0
    wu, wa, uu, ua = fold_all(model, ptr, col, uids, n_epochs=3, install=True)
    assert model.num_guest_nodes == R
    tw = twin_with_nodes(model, ptr, col, wu, uu)
    own, guests = np.arange(R, dtype=np.uint32), GUEST(np.arange(R))

    def served(m, u):
        return ([m.recommend_rows(ptr, col, u, topk, with_scores=True) for topk in (10, 24)]
                + [m.score_rows(ptr, col, cptr, ccol, u, with_ranks=True), m.full_rank_rows(ptr, col, tptr, tcol, u, with_scores=True)])

    def check(msg):
        for got, want in zip(served(model, guests), served(tw, own)):
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b, err_msg=msg)
    check("installed")
    # the nodes make a difference, and guest ids mix with users and NO_USER in one call
    plain = model.recommend_rows(ptr, col, uids, 10)
    assert (plain != model.recommend_rows(ptr, col, guests, 10)).any()
    mixed = uids.copy()
    mixed[::2] = guests[::2]
    got = model.recommend_rows(ptr, col, mixed, 10)
    np.testing.assert_array_equal(got[::2], tw.recommend_rows(ptr, col, own, 10)[::2])
    np.testing.assert_array_equal(got[1::2], plain[1::2])
    # the returned host arrays, handed back
    model.set_guest_nodes(np.zeros((0, K), np.float32))
    with pytest.raises(cdae_amd.CDAEError, match="guest"):
        model.recommend_rows(ptr, col, guests, 10)
    model.set_guest_nodes(wu, wa, uu, ua)
    assert model.num_guest_nodes == R
    check("set_guest_nodes")
    # two more epochs from the guests are epochs 3 and 4 of one five-epoch fit
    more = fold_all(model, ptr, col, guests, epoch_begin=3, n_epochs=2, install=True)
    same_bits(more, fold_all(model, ptr, col, uids, n_epochs=5), "3 + 2 epochs")
    tw.close()
    tw = twin_with_nodes(model, ptr, col, more[0], more[2])
    check("continued")
    tw.close()
    # without the accumulators the table takes reset()'s: a first step from them is what NO_USER takes, from the given wu
    model.set_guest_nodes(wu)
    w2 = fold_all(model, ptr, col, guests, n_epochs=0)
    same_bits(w2, [wu, np.full_like(wu, AG), np.ones_like(wu), np.full_like(wu, AG)], "defaults")
    model.set_guest_nodes(np.zeros((0, K), np.float32))


# ---- 6. more than one chunk ---------------------------------------------------------------------------------------------------------
def test_rows_beyond_one_chunk(built):
    model, _ = model_of(40)
    R = 33_000
    rng = np.random.default_rng(66)
    lens = rng.integers(1, 4, R)
    flat = np.sort(np.argsort(rng.random((R, 64)), axis=1)[:, :3].astype(np.uint32) * 15 + rng.integers(0, 15, (R, 1)).astype(np.uint32), axis=1)
    rows = [flat[r, :lens[r]] for r in range(R)]
    assert all(np.unique(r).size == r.size for r in rows[-64:]) and flat.max() < I_T
    ptr, col = csr(rows)
    uids = rng.integers(0, U_T, R).astype(np.uint32)
    uids[rng.random(R) < 0.3] = NO_USER
    got = fold_all(model, ptr, col, uids, n_epochs=1)
    for r in range(R - 8, R):
        alone = fold_all(model, np.array([0, rows[r].size], np.int64), rows[r], uids[r:r + 1], n_epochs=1, stream_id_base=r)
        same_bits(alone, [a[r:r + 1] for a in got], f"row {r}")
    assert all(np.isfinite(a).all() for a in got) and (got[0] != start_nodes(model, uids)[0]).any(axis=1).all()
    inst = fold_all(model, ptr, col, uids, n_epochs=1, install=True)      # an installing call keeps every chunk
    same_bits(inst, got, "install")
    assert model.num_guest_nodes == R
    tail = np.arange(R - 8, R)
    same_bits(fold_all(model, ptr[tail[0]:] - ptr[tail[0]], col[ptr[tail[0]]:], GUEST(tail), n_epochs=0), [a[tail] for a in got], "guests of chunk 2")
    model.set_guest_nodes(np.zeros((0, 40), np.float32))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(built):
    K = 40
    model, d = model_of(K)
    ptr, col, uids = fold_rows()
    R = ptr.size - 1
    want = fold_all(model, ptr, col, uids, n_epochs=2, install=True)
    guests = GUEST(np.arange(R))
    served = model.recommend_rows(ptr, col, guests, 10)

    def still_right():
        assert model.num_guest_nodes == R
        np.testing.assert_array_equal(model.recommend_rows(ptr, col, guests, 10), served)
        same_bits(fold_all(model, ptr, col, uids, n_epochs=2), want, "after a refusal")
    big = 6                                                              # the 300-item row
    a = int(ptr[big])
    c1 = col.copy(); c1[a], c1[a + 1] = c1[a + 1], c1[a]                 # unsorted
    c2 = col.copy(); c2[a + 1] = c2[a]                                   # duplicate
    c3 = col.copy(); c3[ptr[big + 1] - 1] = I_T                          # out of range
    full_ptr, full_col = csr([col[ptr[0]:ptr[1]], np.arange(I_T, dtype=np.uint32), col[ptr[2]:ptr[3]]])
    u_bad = uids.copy(); u_bad[5] = U_T
    g_bad = guests.copy(); g_bad[9] = GUEST(R)
    bad = [(dict(col=c1), f"row {big}"), (dict(col=c2), f"row {big}"), (dict(col=c3), f"row {big}"), (dict(uids=u_bad), "row 5"),
           (dict(uids=g_bad), "row 9.*guest"), (dict(ptr=full_ptr, col=full_col, uids=uids[:3]), "row 1 holds all")]
    for kw, word in bad:
        args = dict(ptr=ptr, col=col, uids=uids)
        args.update(kw)
        for install in (False, True):
            with pytest.raises(cdae_amd.CDAEError, match=word):
                fold_all(model, args["ptr"], args["col"], args["uids"], n_epochs=2, install=install)
        still_right()
    with pytest.raises(cdae_amd.CDAEError, match="row 9.*guest"):
        model.score_rows(ptr, col, ptr, col, g_bad)
    still_right()
    # no rows: success, nothing touched — except that an installing call clears the table
    assert model.lib.cdae_hip_fold_in_rows(model.h, 0, None, None, None, 0, 0, 3, 0, 0, None, None, None, None) == 0
    still_right()
    assert model.lib.cdae_hip_fold_in_rows(model.h, 0, None, None, None, 0, 0, 3, 0, 1, None, None, None, None) == 0
    assert model.num_guest_nodes == 0
    for call in (lambda: fold_all(model, ptr, col, guests, n_epochs=1), lambda: model.recommend_rows(ptr, col, guests, 10),
                 lambda: model.full_rank_rows(ptr, col, np.zeros(R + 1, np.int64), np.empty(0, np.uint32), guests)):
        with pytest.raises(cdae_amd.CDAEError, match="no guest table"):
            call()
    same_bits(fold_all(model, ptr, col, uids, n_epochs=2), want, "without a table")
    # handles the fold-in does not apply to
    wu = want[0]
    for pairwise in (False, True):                                                 # IMF, BPR
        mf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=8, batch_users=1, pairwise=pairwise))
        mf.reset(d, seed=1)
        with pytest.raises(cdae_amd.CDAEError, match="IMF / BPR"):
            mf.fold_in_rows(ptr, col)
        with pytest.raises(cdae_amd.CDAEError, match="IMF / BPR"):
            mf.set_guest_nodes(np.zeros((4, 8), np.float32))
        np.testing.assert_array_equal(mf.recommend_all(10).shape, (U_T, 10))       # (still usable)
        mf.close()
    mm = cdae_amd.MultiCDAE(model.cfg, devices=[0, 0], item_rows=True)
    mm.reset(d, seed=1)
    shard, out = C.c_void_p(), np.empty((R, K), np.float32)
    assert mm.lib.cdae_hip_multi_shard(mm.h, 0, C.byref(shard), None, None) == 0
    rc = mm.lib.cdae_hip_fold_in_rows(shard, R, None, ptr.ctypes.data, col.ctypes.data, 0, 0, 1, 0, 0, out.ctypes.data, None, None, None)
    assert rc != 0 and b"item shard" in mm.lib.cdae_hip_last_error()
    rc = mm.lib.cdae_hip_set_guest_nodes(shard, R, wu.ctypes.data, None, None, None)
    assert rc != 0 and b"item shard" in mm.lib.cdae_hip_last_error()
    np.testing.assert_array_equal(mm.recommend_all(10).shape, (U_T, 10))
    fresh = cdae_amd.CDAE(model.cfg)
    with pytest.raises(cdae_amd.CDAEError, match="set_interactions"):
        fresh.fold_in_rows(ptr, col)
    with pytest.raises(cdae_amd.CDAEError, match="set_interactions"):
        fresh.set_guest_nodes(wu)
    assert fresh.num_guest_nodes == 0
    for kw, word in ((dict(full_output=True), "full_output"), (dict(user_factor=False), "no user node")):
        other = cdae_amd.CDAE(dataclasses.replace(model.cfg, **kw))
        other.reset(d, seed=1)
        with pytest.raises(cdae_amd.CDAEError, match=word):
            other.fold_in_rows(ptr, col, n_epochs=1)
        with pytest.raises(cdae_amd.CDAEError, match=word):
            other.set_guest_nodes(wu)
        other.train_one_iteration(3, 0)                                            # (still usable)
        assert other.recommend_rows(ptr, col, None, 10).shape == (R, 10)
        other.close()
    # a new data set drops the table
    fresh.reset(d, seed=1)
    fresh.set_guest_nodes(wu)
    assert fresh.num_guest_nodes == R
    fresh.reset(d, seed=1)
    assert fresh.num_guest_nodes == 0
    same_bits(fold_all(model, ptr, col, uids, n_epochs=2), want, "at the end")


# ---- 8. recorded, not asserted --------------------------------------------------------------------------------------------------------
def test_recorded_recall_of_held_out_users_and_wall_clock(built):
    """Measurements, through helpers.record_measured and printed (DESIGN.md §8h quotes a run); nothing here is a promise.
    fold_in_recall: 400 synthetic users, a K = 200 model trained for ten epochs on the first 300; for each of the other 100 the node is
    fitted on 80 % of the user's items (ten epochs) and the remaining 20 % are ranked in the whole catalogue — Recall@10 with NO_USER and
    with the fitted nodes.
    fold_in_wall_clock: one 2 048-row x 10-epoch fold-in on the trained K = 200 model, next to the twin-handle loop of case 2 (reset the
    twin's parameters, train_users on one row) — timed over 64 of the rows for one epoch, so the loop's figure for all rows and epochs
    is 320 x what is recorded as loop_64x1_s."""
    K = 200
    d = synth.generate(400, I_T, 400 * 40, seed=7, min_items=5)
    tr = d.user_range(0, 300)
    m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64))
    m.reset(tr, seed=3)
    for ep in range(10):
        m.train_one_iteration(3, ep)
    rng = np.random.default_rng(4)
    fit, held = [], []
    for u in range(300, 400):
        row = d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]
        out = np.zeros(row.size, bool)
        out[rng.choice(row.size, max(1, row.size // 5), replace=False)] = True
        fit.append(row[~out]); held.append(row[out])
    fptr, fcol = csr(fit)
    hptr, hcol = csr(held)
    base = m.eval_ranking_rows(fptr, fcol, hptr, hcol, None, ks=(10,))
    m.fold_in_rows(fptr, fcol, None, seed=11, n_epochs=10, install=True)
    fitted = m.eval_ranking_rows(fptr, fcol, hptr, hcol, GUEST(np.arange(100)), ks=(10,))
    print(f"held-out Recall@10: NO_USER {base['recall@10']:.4f}, fitted nodes {fitted['recall@10']:.4f}")
    record_measured("fold_in_recall", no_user=base["recall@10"], fitted=fitted["recall@10"])
    m.close()

    model, _ = model_of(K)
    R = 2048
    rows = [np.sort(rng.choice(I_T, int(rng.integers(1, 61)), replace=False)).astype(np.uint32) for _ in range(R)]
    ptr, col = csr(rows)
    uids = rng.integers(0, U_T, R).astype(np.uint32)
    model.fold_in_rows(ptr, col, uids, seed=SEED, n_epochs=10)                       # warm-up: the grow-only buffers
    t0 = time.perf_counter()
    model.fold_in_rows(ptr, col, uids, seed=SEED, n_epochs=10)
    t_fold = time.perf_counter() - t0
    n_loop = 64
    tw = cdae_amd.CDAE(dataclasses.replace(model.cfg, batch_users=1))
    tw.set_interactions(n_loop, I_T, *csr(rows[:n_loop]))
    tw.init_params(0)
    shared = {w: model.get(w) for w in (cdae_amd.P_W, cdae_amd.P_W_AG, cdae_amd.P_B, cdae_amd.P_B_AG, cdae_amd.P_BP, cdae_amd.P_BP_AG)}

    def loop():
        for r in range(n_loop):
            for w, a in shared.items():
                tw.set(w, a)
            tw.train_users(SEED, 0, r, r + 1)
    loop()
    t0 = time.perf_counter()
    loop()
    t_loop = time.perf_counter() - t0
    tw.close()
    print(f"fold_in_rows {R} rows x 10 epochs {1e3 * t_fold:.3f} ms; twin loop {n_loop} rows x 1 epoch {1e3 * t_loop:.3f} ms "
          f"(x {R * 10 // n_loop} for the same work: {t_loop * R * 10 / n_loop:.3f} s)")
    record_measured("fold_in_wall_clock", rows=R, epochs=10, fold_s=t_fold, loop_64x1_s=t_loop)
