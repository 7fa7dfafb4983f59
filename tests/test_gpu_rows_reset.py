"""-m gpu: a handle that has served caller-supplied rows is given new interactions and serves rows again.

Every rows entry point keeps its device arrays in grow-only workspaces of the handle.  cdae_hip_set_interactions frees them all; a
workspace that were freed while its capacity stayed would be believed by the next call that needs no more than that, which would then
write through a null pointer.  So: a LARGER data set first (64 users x 5 000 items, 48 rows), every rows entry point once on both
top-k paths, then a SMALLER one (40 users x 300 items, 12 rows) on the same handle — and every array the second round returns must
carry the bits a fresh handle returns that has only ever seen the second data set.  The guest table does not survive the new
interactions either: a row that names a guest is refused until the next install.
"""
import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth

pytestmark = pytest.mark.gpu

NO_USER = cdae_amd.NO_USER
K, BATCH = 32, 64
N_FOLD = 8


def csr(rows):
    return np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64), np.concatenate(rows).astype(np.uint32)


def draw(rng, I, n):
    return np.sort(rng.choice(I, size=int(n), replace=False)).astype(np.uint32)


def start(model, d):
    model.set_interactions(d.num_users, d.num_items, d.train_ptr, d.train_col)
    model.init_params(5)
    model.train_one_iteration(5, 0)


def serve(model, U, I, R, n_allow, seed):
    """every rows entry point once, on R caller rows of 1-40 items -> {name: array}"""
    rng = np.random.default_rng(seed)
    rows = [draw(rng, I, rng.integers(1, 41)) for _ in range(R)]
    ptr, col = csr(rows)
    uids = rng.integers(0, U, R).astype(np.uint32)
    uids[rng.random(R) < 0.2] = NO_USER
    unrated = [np.setdiff1d(np.arange(I, dtype=np.uint32), r) for r in rows]
    tptr, tcol = csr([np.sort(rng.choice(u, size=int(rng.integers(0, 6)), replace=False)) for u in unrated[:-1]] + [unrated[-1][:3]])
    eptr, ecol = csr([draw(rng, I, rng.integers(0, 11)) for _ in range(R)])
    cptr, ccol = csr([draw(rng, I, rng.integers(1, 31)) for _ in range(R)])
    allow = draw(rng, I, n_allow)
    out = {}
    for topk in (10, 32):                                            # the matrix cores; the general path (above REC_TOPK_MAX = 16)
        out[f"ids{topk}"], out[f"scores{topk}"] = model.recommend_rows(ptr, col, uids, topk, with_scores=True)
    out["rets"], out["hits"], out["eval_ids"] = model.eval_topn_rows(ptr, col, tptr, tcol, uids, 10, with_ids=True)
    out["flt_ids"], out["flt_scores"] = model.recommend_rows_filtered(ptr, col, uids, 10, exclude=(eptr, ecol), allow=allow, with_scores=True)
    out["cand_scores"], out["cand_ranks"] = model.score_rows(ptr, col, cptr, ccol, uids, with_ranks=True)
    out["fr_ranks"], out["fr_scores"] = model.full_rank_rows(ptr, col, tptr, tcol, uids, with_scores=True)
    fold = model.fold_in_rows(ptr[:N_FOLD + 1], col[:ptr[N_FOLD]], uids[:N_FOLD], seed=7, n_epochs=3, install=True, with_accumulators=True)
    out["fold_wu"], out["fold_wu_ag"] = fold
    assert model.num_guest_nodes == N_FOLD
    out["guest_ids"] = model.recommend_rows(ptr[:N_FOLD + 1], col[:ptr[N_FOLD]], cdae_amd.GUEST_USER(np.arange(N_FOLD)), 10)
    return out


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def test_rows_after_a_second_set_interactions(built):
    big = synth.generate(64, 5000, 64 * 20, seed=11, min_items=5)
    small = synth.generate(40, 300, 40 * 20, seed=12, min_items=5)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=BATCH, user_factor=True)
    model = cdae_amd.CDAE(cfg)
    start(model, big)
    first = serve(model, big.num_users, big.num_items, 48, 200, seed=21)
    assert all(a.size for a in first.values())
    start(model, small)
    assert model.num_guest_nodes == 0
    one_ptr, one_col = csr([np.arange(3, dtype=np.uint32)])
    with pytest.raises(cdae_amd.CDAEError, match="has no guest table"):
        model.recommend_rows(one_ptr, one_col, cdae_amd.GUEST_USER(np.arange(1)), 10)
    got = serve(model, small.num_users, small.num_items, 12, 20, seed=22)
    fresh = cdae_amd.CDAE(cfg)
    start(fresh, small)
    want = serve(fresh, small.num_users, small.num_items, 12, 20, seed=22)
    assert got.keys() == want.keys()
    for name in want:
        assert got[name].shape == want[name].shape and np.array_equal(bits(got[name]), bits(want[name])), name
    model.close()
    fresh.close()
