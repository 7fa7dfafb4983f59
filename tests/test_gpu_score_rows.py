"""-m gpu: scores and ranks of caller-supplied candidate sets (cdae_hip_score_rows / CDAE.score_rows), the batched counterpart of
the reference's get_output_values(z, idx) (cdae.hpp:418-426).  Pinned here:
  * every score and every rank, exactly, on integer models whose scores fp32 holds in any summation order (helpers.exact_scores),
    over all four row strides, candidate rows around every tile boundary, candidates inside the rated set, plateaus of equal scores;
  * every score against fp64 (tests/score_rows_ref.py, itself checked against the oracle by tests/test_score_rows_reference.py) on
    trained models, within the textbook bound of ONE fp32 dot product;
  * agreement with recommend_rows on both of its paths; position independence (equal bits whatever else the call holds);
  * ranks == the order of the returned scores, the cap of RANK_CANDIDATES_MAX; both chunk bounds; every refusal; training untouched;
  * the wall-clock comparison with the only route the library had for the same numbers (a full ranking of every row).
"""
import functools
import time

import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth
from helpers import SENTINEL, assert_fp32_exact, exact_scores, record_measured
from score_rows_ref import magnitudes64, ranks_of, row_of_position, scores64

pytestmark = pytest.mark.gpu

NO_USER = cdae_amd.NO_USER
EVAL_CHUNK = 32768                   # rows per chunk (cdae_hip.hip)
CAND_CHUNK = 65536                   # candidates per chunk (include/cdae_hip.h)
I_T = 977


def csr(rows):
    return np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64), (np.concatenate(rows) if rows else np.empty(0)).astype(np.uint32)


def pick(rng, I, n):
    return np.sort(rng.choice(I, size=int(n), replace=False)).astype(np.uint32)


def draw_uids(rng, U, R):
    """users with repeats, a fifth of the rows without a user node"""
    uids = rng.integers(0, U, R).astype(np.uint32)
    uids[rng.random(R) < 0.2] = NO_USER
    return uids


def gathered(M, uids, fill):
    """M[uids], rows of `fill` where the row has no user node"""
    out = np.full((len(uids), M.shape[1]), fill, dtype=M.dtype)
    real = np.asarray(uids) != NO_USER
    out[real] = M[np.asarray(uids)[real].astype(np.int64)]
    return out


def train_data(U, I, seed):
    rng = np.random.default_rng(seed)
    ptr, col = csr([pick(rng, I, rng.integers(1, 41)) for _ in range(U)])
    return synth.Interactions(U, I, ptr, col, np.zeros(U + 1, np.int64), np.empty(0, np.uint32))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. every score and every rank, exactly, on integer models ----------------------------------------------------------------------
def int_params(mode, U, I, K, asymmetric, seed):
    """Integer parameters as float64 arrays.  "levels": every decoder row is the same vector, so z . D[j] is one number per row and
    b' — three levels, each on long runs of item ids — decides every comparison: most ranks come from the tie rule."""
    rng = np.random.default_rng(seed)
    p = dict(W=rng.integers(-2, 3, (I, K)), b=rng.integers(-3, 4, K), Wu=rng.integers(-3, 4, (U, K)), bp=rng.integers(-4, 5, I))
    if asymmetric:
        p["V"] = rng.integers(-2, 3, (I, K))
    if mode == "levels":
        r = np.zeros(K, dtype=np.int64)
        at = rng.choice(K, min(K, 16), replace=False)
        r[at] = rng.integers(1, 3, at.size) * rng.choice([-1, 1], at.size)
        p["V" if asymmetric else "W"] = np.tile(r, (I, 1))
        j = np.arange(I)
        p["bp"] = (5 * j + j // 8 + j // 32) % 3
    return {k: v.astype(np.float64) for k, v in p.items()}


def load(model, p):
    model.set(cdae_amd.P_W, p["W"]); model.set(cdae_amd.P_B, p["b"]); model.set(cdae_amd.P_WU, p["Wu"]); model.set(cdae_amd.P_BP, p["bp"])
    if "V" in p:
        model.set(cdae_amd.P_V, p["V"])


def linear_model(d, K, asymmetric):
    m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, linear=True, asymmetric=asymmetric, batch_users=32))
    m.reset(d, seed=1)
    return m


def int_sets(rng, I, R=80):
    """rated rows of 0, 1, 64, 65, 129, 300 items and ordinary ones; candidate rows of every length around the 64-candidate tile
    (0, 1, 63, 64, 65, 101, 128, 129), all items, ordinary ones; the first rows' candidates hold the row's own rated items"""
    rated = [pick(rng, I, n) for n in (0, 1, 64, 65, 129, 300)] + [pick(rng, I, rng.integers(1, 41)) for _ in range(R - 6)]
    lens = [0, 1, 63, 64, 65, 101, 128, 129, I] + [int(rng.integers(1, 121)) for _ in range(R - 9)]
    order = rng.permutation(R)
    cands = [None] * R
    for n, r in zip(lens, order):
        own = rated[r][:min(rated[r].size, n // 2)] if r % 2 == 0 else np.empty(0, np.uint32)
        free = np.setdiff1d(np.arange(I, dtype=np.uint32), own)
        cands[r] = np.sort(np.r_[own, rng.choice(free, n - own.size, replace=False)]).astype(np.uint32)
    assert sum(np.intersect1d(c, r).size > 0 for c, r in zip(cands, rated)) >= 10
    return csr(rated), csr(cands)


def expected_exact(p, ptr, col, uids, cptr, ccol):
    q = dict(p, Wu=gathered(p["Wu"], uids, 0.0))
    Z, S, D, bq = exact_scores(ptr, col, **q)
    assert_fp32_exact(Z, D, bq)                      # a condition on the inputs, checked before the GPU is touched
    sc = S[row_of_position(cptr), ccol.astype(np.int64)].astype(np.float32)
    return sc, ranks_of(sc, cptr, ccol)


@pytest.mark.parametrize("asymmetric", [False, True])
@pytest.mark.parametrize("K", [5, 64, 100, 200, 300, 512])       # the four row strides, each with and without pad columns
def test_every_score_and_every_rank_exactly(built, K, asymmetric):
    U, I = 60, I_T
    d = train_data(U, I, seed=K)
    model = linear_model(d, K, asymmetric)
    rng = np.random.default_rng(2000 + K)
    (ptr, col), (cptr, ccol) = int_sets(rng, I)
    uids = draw_uids(rng, U, ptr.size - 1)
    assert (uids == NO_USER).any() and (uids != NO_USER).any()
    for mode in ("random", "levels"):
        p = int_params(mode, U, I, K, asymmetric, seed=K + I)
        load(model, p)
        want, want_rank = expected_exact(p, ptr, col, uids, cptr, ccol)
        if mode == "levels":                        # three scores per row: the tie rule decides most ranks
            assert max(np.unique(want[a:b]).size for a, b in zip(cptr[:-1], cptr[1:])) <= 3
        sc, rk = model.score_rows(ptr, col, cptr, ccol, uids, with_ranks=True)
        assert sc.dtype == np.float32 and rk.dtype == np.uint32 and sc.shape == rk.shape == (cptr[-1],)
        np.testing.assert_array_equal(sc, want, err_msg=mode)
        np.testing.assert_array_equal(rk, want_rank, err_msg=mode)
        np.testing.assert_array_equal(model.score_rows(ptr, col, cptr, ccol, uids), want)              # without ranks
    none, none_rank = expected_exact(p, ptr, col, np.full(ptr.size - 1, NO_USER, np.uint32), cptr, ccol)
    sc, rk = model.score_rows(ptr, col, cptr, ccol, None, with_ranks=True)
    np.testing.assert_array_equal(sc, none)
    np.testing.assert_array_equal(rk, none_rank)


# ---- trained real-valued models, shared by cases 2, 3, 4, 5 and 9 -------------------------------------------------------------------
U_T = 500


@functools.lru_cache(maxsize=None)
def trained(K, flags=()):
    d = synth.generate(U_T, I_T, U_T * 40, seed=7, min_items=5)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64, **dict(flags))
    m = cdae_amd.CDAE(cfg)
    m.reset(d, seed=3)
    for ep in range(2):
        m.train_one_iteration(3, ep)
    return m, d


@functools.lru_cache(maxsize=None)
def foreign(R=120, seed=5):
    """rows that are no train rows: two of several summation groups (300 and 257 items), one of a single item, ordinary ones; user
    ids with repeats, some rows without a user node; candidate rows of 1-150 items, half of them holding rated items of the row"""
    rng = np.random.default_rng(seed)
    rows = [pick(rng, I_T, n) for n in (300, 257, 129, 1)] + [pick(rng, I_T, rng.integers(1, 61)) for _ in range(R - 4)]
    uids = rng.permutation(U_T)[:R].astype(np.uint32)
    uids[rng.random(R) < 0.15] = NO_USER
    uids[0], uids[1] = 17, NO_USER                  # a long row with a user node, one without
    cands = []
    for r, row in enumerate(rows):
        c = pick(rng, I_T, rng.integers(1, 151))
        cands.append(np.union1d(c, row[:5]).astype(np.uint32) if r % 2 == 0 else c)
    return csr(rows) + (uids,) + csr(cands)


def twin_z(model, ptr, col, uids):
    """the fp32 z a handle encodes from those sets: a handle with the same configuration whose TRAIN rows are the caller's rows and
    whose private rows are the gathered ones.  corruption_ratio == 1: the rows entry points encode the empty input, which is what
    the twin's training-form encode (mode 1, every input dropped, scale 1 with scaled = False) gives."""
    cfg = model.cfg
    tw = cdae_amd.CDAE(cfg)
    tw.set_interactions(ptr.size - 1, model.num_items, ptr, col)
    tw.init_params(0)
    for which in (cdae_amd.P_W, cdae_amd.P_B, cdae_amd.P_BP) + ((cdae_amd.P_V,) if cfg.asymmetric else ()):
        tw.set(which, model.get(which))
    tw.set(cdae_amd.P_WU, gathered(model.get(cdae_amd.P_WU), uids, 0.0))
    if cfg.linear_function:
        tw.set(cdae_amd.P_UU, gathered(model.get(cdae_amd.P_UU), uids, 1.0))
    empty = cfg.corruption_ratio == 1.0
    assert not (empty and cfg.scaled)
    z = tw.get_hidden_values(np.arange(ptr.size - 1, dtype=np.uint32), mode=1 if empty else 0)
    tw.close()
    assert z.dtype == np.float32 and np.isfinite(z).all()
    return z


def one_score_bound(model, z, cptr, ccol):
    """(Kc + 2) 2^-24 (sum_k |z_k D_jk| + |b'_j|) per pair, Kc the row stride: the bound helpers.assert_valid_topk derives, for ONE
    score (not doubled); with the fp64 scores of the fp32 z, D and b'"""
    which = cdae_amd.P_V if model.cfg.asymmetric else cdae_amd.P_W
    D, bp = model.get(which), model.get(cdae_amd.P_BP)
    Kc = int(model.lib.cdae_hip_row_stride(model.h))
    assert Kc >= model.cfg.num_dim and Kc in (64, 128, 256, 512)
    return scores64(z, D, bp, cptr, ccol), (Kc + 2) * 2.0 ** -24 * magnitudes64(z, D, bp, cptr, ccol)


# ---- 2. against fp64 on trained models ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags", [(200, ()), (300, ()), (40, (("tanh", True),)), (40, (("linear_function", True),)),
                                     (40, (("corruption_ratio", 1.0), ("scaled", False)))])
def test_every_score_against_fp64(built, K, flags):
    model, d = trained(K, flags)
    ptr, col, uids, cptr, ccol = foreign()
    assert np.diff(ptr).max() == 300 and 257 in np.diff(ptr) and (uids == NO_USER).any()
    z = twin_z(model, ptr, col, uids)
    assert np.unique(z[:, 0]).size > (1 if dict(flags).get("corruption_ratio") == 1.0 else 50)
    want, eps = one_score_bound(model, z, cptr, ccol)
    got = model.score_rows(ptr, col, cptr, ccol, uids)
    err = np.abs(got.astype(np.float64) - want)
    print(f"K {K} {dict(flags)}: worst |got - fp64| / bound = {(err / eps).max():.4f} over {got.size} pairs")
    assert (err <= eps).all(), (err / eps).max()
    assert np.abs(want).max() > 1e-3 and np.unique(got).size > got.size // 2


# ---- 3. agreement with recommend_rows ------------------------------------------------------------------------------------------------
def lists_as_candidates(ids):
    keep = ids != SENTINEL
    rows = [np.sort(ids[r][keep[r]]) for r in range(ids.shape[0])]
    return csr(rows)


@pytest.mark.parametrize("K", [100, 300])
def test_scores_and_ranks_reproduce_recommend_rows_on_an_integer_model(built, K):
    U, I = 60, I_T
    d = train_data(U, I, seed=K)
    model = linear_model(d, K, False)
    rng = np.random.default_rng(3000 + K)
    (ptr, col), _ = int_sets(rng, I)
    uids = draw_uids(rng, U, ptr.size - 1)
    load(model, int_params("random", U, I, K, False, seed=K + I))
    for topk in (10, 24):                           # 10: matrix cores when K <= 256; 24: general path
        ids, listed = model.recommend_rows(ptr, col, uids, topk, with_scores=True)
        assert (ids != SENTINEL).all()
        cptr, ccol = lists_as_candidates(ids)
        sc, rk = model.score_rows(ptr, col, cptr, ccol, uids, with_ranks=True)
        for r in range(ids.shape[0]):
            at = cptr[r] + np.searchsorted(ccol[cptr[r]:cptr[r + 1]], ids[r])
            np.testing.assert_array_equal(sc[at], listed[r], err_msg=f"topk {topk} row {r}")
            np.testing.assert_array_equal(rk[at], np.arange(topk), err_msg=f"topk {topk} row {r}")


@pytest.mark.parametrize("K", [200, 300])
def test_scores_agree_with_recommend_rows_on_a_trained_model(built, K):
    model, d = trained(K)
    ptr, col, uids, _, _ = foreign()
    z = twin_z(model, ptr, col, uids)
    for topk in (10, 24):
        ids, listed = model.recommend_rows(ptr, col, uids, topk, with_scores=True)
        cptr, ccol = lists_as_candidates(ids)
        _, eps = one_score_bound(model, z, cptr, ccol)
        sc = model.score_rows(ptr, col, cptr, ccol, uids)
        for r in range(ids.shape[0]):
            at = cptr[r] + np.searchsorted(ccol[cptr[r]:cptr[r + 1]], ids[r])
            assert (np.abs(sc[at].astype(np.float64) - listed[r]) <= 2 * eps[at]).all(), (topk, r)


# ---- 4. position independence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [200, 300])
def test_a_pair_has_the_same_bits_wherever_it_sits(built, K):
    model, d = trained(K)
    ptr, col, uids, _, _ = foreign()
    R = 40
    rows = [col[ptr[r]:ptr[r + 1]] for r in range(R)]
    every = np.arange(I_T, dtype=np.uint32)
    full = model.score_rows(*csr(rows), *csr([every] * R), uids[:R]).reshape(R, I_T)
    rng = np.random.default_rng(40 + K)
    perm = list(rng.permutation(R)) + [7]                                  # permuted, row 7 a second time
    thin = [pick(rng, I_T, rng.integers(1, 300)) for _ in perm]
    thin[3] = np.empty(0, np.uint32)
    rows2 = [rows[0]] + [rows[r] for r in perm]                            # a long all-items row in front
    cands2 = [every] + thin
    uids2 = np.r_[uids[0], uids[perm]].astype(np.uint32)
    cp2, cc2 = csr(cands2)
    got = model.score_rows(*csr(rows2), cp2, cc2, uids2)
    np.testing.assert_array_equal(bits(got[:I_T]), bits(full[0]))
    for n, r in enumerate(perm):
        a, b = cp2[n + 1], cp2[n + 2]
        np.testing.assert_array_equal(bits(got[a:b]), bits(full[r, cc2[a:b].astype(np.int64)]), err_msg=f"row {r}")
    assert np.unique(full).size > full.size // 4


# ---- 5. ranks are the order of the returned scores -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_model(I, U=64, K=8):
    d = train_data(U, I, seed=I)
    m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=32))
    m.reset(d, seed=4)
    m.train_one_iteration(4, 0)
    return m, d


def test_ranks_are_the_order_of_the_returned_scores(built):
    model, d = trained(200)
    ptr, col, uids, cptr, ccol = foreign()
    sc, rk = model.score_rows(ptr, col, cptr, ccol, uids, with_ranks=True)
    np.testing.assert_array_equal(rk, ranks_of(sc, cptr, ccol))
    np.testing.assert_array_equal(bits(sc), bits(model.score_rows(ptr, col, cptr, ccol, uids)))
    wide, dw = wide_model(5000)
    I, cap = 5000, cdae_amd.RANK_CANDIDATES_MAX
    assert cap == 4096
    rng = np.random.default_rng(51)
    rows = [pick(rng, I, n) for n in (30, 1, 0, 12, 40, 7)]
    cands = [pick(rng, I, n) for n in (64, cap, 65, 0, 1, 700)]
    u = np.array([3, NO_USER, 9, 3, 60, 11], dtype=np.uint32)
    (rp, rc), (cp, cc) = csr(rows), csr(cands)
    sc, rk = wide.score_rows(rp, rc, cp, cc, u, with_ranks=True)
    np.testing.assert_array_equal(rk, ranks_of(sc, cp, cc))
    for a, b in zip(cp[:-1], cp[1:]):
        np.testing.assert_array_equal(np.sort(rk[a:b]), np.arange(b - a))
    assert np.unique(sc[cp[1]:cp[2]]).size > 1000
    cands[4] = pick(rng, I, cap + 1)
    cp, cc = csr(cands)
    with pytest.raises(cdae_amd.CDAEError, match="row 4"):
        wide.score_rows(rp, rc, cp, cc, u, with_ranks=True)
    over = wide.score_rows(rp, rc, cp, cc, u)                                # scores alone have no cap
    np.testing.assert_array_equal(bits(over[:cp[4]]), bits(sc[:cp[4]]))
    np.testing.assert_array_equal(ranks_of(over, cp, cc)[:cp[4]], rk[:cp[4]])


# ---- 6. chunk boundaries -------------------------------------------------------------------------------------------------------------
def test_more_rows_and_more_candidates_than_one_chunk(built):
    U, I, K, R = 129, 96, 8, EVAL_CHUNK + 129
    model, d = wide_model(I, U, K)
    rng = np.random.default_rng(61)
    lens = rng.integers(0, 6, R)
    flat = np.argsort(rng.random((R, I)), axis=1)[:, :8].astype(np.uint32)
    rows = [np.sort(flat[r, :lens[r]]) for r in range(R)]
    cands = [np.sort(flat[r, 3:6]) for r in range(R)]                        # three candidates each, some of them rated
    mid = 20_000
    cands[mid] = np.arange(I, dtype=np.uint32)
    uids = draw_uids(rng, U, R)
    (ptr, col), (cptr, ccol) = csr(rows), csr(cands)
    assert R > EVAL_CHUNK and cptr[-1] > CAND_CHUNK and cptr[EVAL_CHUNK] > CAND_CHUNK
    sc, rk = model.score_rows(ptr, col, cptr, ccol, uids, with_ranks=True)
    cut = mid + 1
    for a, b in ((0, cut), (cut, R)):
        s2, r2 = model.score_rows(*csr(rows[a:b]), *csr(cands[a:b]), uids[a:b], with_ranks=True)
        np.testing.assert_array_equal(bits(sc[cptr[a]:cptr[b]]), bits(s2))
        np.testing.assert_array_equal(rk[cptr[a]:cptr[b]], r2)
    np.testing.assert_array_equal(rk, ranks_of(sc, cptr, ccol))
    assert np.unique(sc).size > 1000


def test_one_row_of_more_candidates_than_one_chunk(built):
    I = 70_000
    model, d = wide_model(I, 40, 8)
    assert I > CAND_CHUNK
    rng = np.random.default_rng(62)
    rows = [pick(rng, I, 30), pick(rng, I, 5), pick(rng, I, 12)]
    cands = [pick(rng, I, 200), np.arange(I, dtype=np.uint32), pick(rng, I, 100)]      # before, across and behind the cut row
    uids = np.array([3, NO_USER, 39], dtype=np.uint32)
    (ptr, col), (cptr, ccol) = csr(rows), csr(cands)
    z = twin_z(model, ptr, col, uids)
    want, eps = one_score_bound(model, z, cptr, ccol)
    got = model.score_rows(ptr, col, cptr, ccol, uids)
    err = np.abs(got.astype(np.float64) - want)
    print(f"70 000 candidates in one row: worst |got - fp64| / bound = {(err / eps).max():.4f}")
    assert (err <= eps).all(), (err / eps).max()
    alone = model.score_rows(*csr(rows[1:2]), *csr(cands[1:2]), uids[1:2])
    np.testing.assert_array_equal(bits(got[cptr[1]:cptr[2]]), bits(alone))
    assert np.unique(got).size > 10_000


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(built):
    model, d = trained(40, (("tanh", True),))
    U, I = U_T, I_T
    ptr, col, uids, cptr, ccol = foreign()
    R = ptr.size - 1
    before_s, before_r = model.score_rows(ptr, col, cptr, ccol, uids, with_ranks=True)

    def unchanged():
        s, r = model.score_rows(ptr, col, cptr, ccol, uids, with_ranks=True)
        np.testing.assert_array_equal(bits(s), bits(before_s))
        np.testing.assert_array_equal(r, before_r)
    big = int(np.argmax(np.diff(cptr) >= 2))
    a = int(cptr[big])

    def swapped():
        c = ccol.copy(); c[a], c[a + 1] = c[a + 1], c[a]
        return dict(cand_col=c)

    def duplicate():
        c = ccol.copy(); c[a + 1] = c[a]
        return dict(cand_col=c)

    def out_of_range():
        c = ccol.copy(); c[cptr[big + 1] - 1] = I
        return dict(cand_col=c)

    def decreasing():
        p = cptr.copy(); p[9] = p[8] - 1
        return dict(cand_ptr=p)

    def uid_out_of_range():
        u = uids.copy(); u[5] = U
        return dict(uids=u)

    def rated_unsorted():
        c = col.copy(); c[0], c[1] = c[1], c[0]
        return dict(col=c)
    bad = [(swapped(), f"candidate row {big}"), (duplicate(), f"candidate row {big}"), (out_of_range(), f"candidate row {big}"),
           (decreasing(), "candidate row_ptr decreases at row 8"), (uid_out_of_range(), "row 5"), (rated_unsorted(), "rated row 0")]
    for kw, word in bad:
        args = dict(row_ptr=ptr, col=col, cand_ptr=cptr, cand_col=ccol, uids=uids)
        args.update(kw)
        for with_ranks in (False, True):
            with pytest.raises(cdae_amd.CDAEError, match=word):
                model.score_rows(with_ranks=with_ranks, **args)
        unchanged()
    # ranks over the cap: the row is named before anything is launched
    wide, _ = wide_model(5000)
    rng = np.random.default_rng(71)
    rp, rc = csr([pick(rng, 5000, 3), pick(rng, 5000, 4)])
    cp, cc = csr([pick(rng, 5000, 10), pick(rng, 5000, cdae_amd.RANK_CANDIDATES_MAX + 1)])
    ok = wide.score_rows(rp, rc, cp, cc)
    with pytest.raises(cdae_amd.CDAEError, match="row 1"):
        wide.score_rows(rp, rc, cp, cc, with_ranks=True)
    np.testing.assert_array_equal(bits(wide.score_rows(rp, rc, cp, cc)), bits(ok))
    # a null out_scores with candidates present
    u32 = np.ascontiguousarray(uids)
    assert model.lib.cdae_hip_score_rows(model.h, R, u32.ctypes.data, ptr.ctypes.data, col.ctypes.data, cptr.ctypes.data, ccol.ctypes.data,
                                         None, None) != 0
    assert b"out_scores" in model.lib.cdae_hip_last_error()
    unchanged()
    # no rows; rows without any candidate: success, nothing written
    assert model.lib.cdae_hip_score_rows(model.h, 0, None, None, None, None, None, None, None) == 0
    assert model.score_rows(np.zeros(1, np.int64), np.empty(0, np.uint32), np.zeros(1, np.int64), np.empty(0, np.uint32)).shape == (0,)
    zero = np.zeros(R + 1, np.int64)
    assert model.lib.cdae_hip_score_rows(model.h, R, u32.ctypes.data, ptr.ctypes.data, col.ctypes.data, zero.ctypes.data, None, None, None) == 0
    s, r = model.score_rows(ptr, col, zero, np.empty(0, np.uint32), uids, with_ranks=True)
    assert s.shape == r.shape == (0,)
    unchanged()
    # an IMF / BPR handle; a handle without interactions
    mf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=8, batch_users=1))
    mf.reset(d, seed=1)
    with pytest.raises(cdae_amd.CDAEError, match="IMF / BPR"):
        mf.score_rows(ptr, col, cptr, ccol)
    assert mf.recommend_all(10).shape == (U, 10)                             # (still usable)
    fresh = cdae_amd.CDAE(model.cfg)
    with pytest.raises(cdae_amd.CDAEError, match="set_interactions"):
        fresh.score_rows(ptr, col, cptr, ccol)
    fresh.reset(d, seed=1)
    for which in (cdae_amd.P_W, cdae_amd.P_B, cdae_amd.P_BP, cdae_amd.P_WU):
        fresh.set(which, model.get(which))
    np.testing.assert_array_equal(bits(fresh.score_rows(ptr, col, cptr, ccol, uids)), bits(before_s))
    fresh.close()
    unchanged()


# ---- 8. training is untouched --------------------------------------------------------------------------------------------------------
def test_training_is_untouched(built):
    d = synth.generate(200, I_T, 200 * 30, seed=8, min_items=5)
    ptr, col, uids, cptr, ccol = foreign()
    uids = np.where(uids == NO_USER, NO_USER, uids % 200).astype(np.uint32)
    models = []
    for scoring in (False, True):
        m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=40, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64))
        m.reset(d, seed=3)
        for ep in range(3):
            m.train_one_iteration(3, ep)
            if scoring:
                m.score_rows(ptr, col, cptr, ccol, uids, with_ranks=True)
                m.score_rows(ptr, col, cptr, ccol, None)
        models.append(m)
    for which in (cdae_amd.P_W, cdae_amd.P_W_AG, cdae_amd.P_B, cdae_amd.P_B_AG, cdae_amd.P_BP, cdae_amd.P_BP_AG, cdae_amd.P_WU, cdae_amd.P_WU_AG):
        np.testing.assert_array_equal(bits(models[0].get(which)), bits(models[1].get(which)), err_msg=str(which))
    for m in models:
        m.close()


# ---- 9. measurement ------------------------------------------------------------------------------------------------------------------
def test_one_call_is_faster_than_a_full_ranking_of_every_row(built):
    """2 048 foreign rows of 1-60 items, 101 candidates each, trained K = 200 model over 977 items: one score_rows call against the
    only route the library had for the same numbers, recommend_rows(topk = 977, with_scores) — every item scored and fully sorted.
    Wall clock after one warm-up of each route, the minimum of three; asserted only as "faster" (both times are printed and go to
    helpers.record_measured as score_rows_vs_full_ranking; DESIGN.md 8f has the table).
    Measured on an MI355X: score_rows 0.482 ms, recommend_rows(topk = 977) 2.477 ms."""
    model, d = trained(200)
    R = 2048
    rng = np.random.default_rng(9)
    (ptr, col), (cptr, ccol) = csr([pick(rng, I_T, rng.integers(1, 61)) for _ in range(R)]), csr([pick(rng, I_T, 101) for _ in range(R)])
    uids = rng.integers(0, U_T, R).astype(np.uint32)

    def batched():
        return model.score_rows(ptr, col, cptr, ccol, uids, with_ranks=True)

    def full():
        return model.recommend_rows(ptr, col, uids, I_T, with_scores=True)

    def best(f):
        f()
        times = []
        for _ in range(3):
            t0 = time.perf_counter(); out = f(); times.append(time.perf_counter() - t0)
        return min(times), out
    batched_s, (sc, rk) = best(batched)
    full_s, (ids, listed) = best(full)
    record_measured("score_rows_vs_full_ranking", rows=R, batched_s=batched_s, full_s=full_s)
    print(f"score_rows {1e3 * batched_s:.3f} ms, recommend_rows(topk = {I_T}) {1e3 * full_s:.3f} ms")
    assert batched_s < full_s
    # the same numbers: the full ranking lists every unrated candidate with a score within two one-score bounds of ours
    z = twin_z(model, ptr[:65], col[:ptr[64]], uids[:64])
    _, eps = one_score_bound(model, z, cptr[:65], ccol[:cptr[64]])
    for r in range(64):
        where = {int(j): t for t, j in enumerate(ids[r]) if j != SENTINEL}
        for p in range(cptr[r], cptr[r + 1]):
            if int(ccol[p]) in where:
                assert abs(float(sc[p]) - float(listed[r, where[int(ccol[p])]])) <= 2 * eps[p]
    np.testing.assert_array_equal(rk, ranks_of(sc, cptr, ccol))
