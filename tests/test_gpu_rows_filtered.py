"""-m gpu: batched top-k with an item allow list and exclusions apart from the inputs (cdae_hip_recommend_rows_filtered).

The contract (include/cdae_hip.h) is exact: row r's list is cdae_hip_recommend_rows' list of unbounded length with the items outside
C_r = allow \\ excl_r (\\ rated_r when exclude_rated) deleted, the scores the same bits; neither excl nor allow enters z.  Every
comparison here is assert_array_equal on the ids and on the bit patterns of the scores, over every row and every place:
  * the documented order on integer models whose scores fp32 holds exactly (tests/filtered_ref.py over helpers.exact_scores), allow
    lists and excl rows aimed at the masks of both top-k kernels;
  * on trained float models, the deletion property against recommend_rows' whole list (general path) and against full_rank_rows'
    scores and ranks of every unrated item (matrix cores: the packed sweep puts an item into another row of another tile, and its
    score must not notice), no filter == recommend_rows, and the three readings of exclude_rated = 0;
  * position independence across the chunk boundary; item spaces beyond 65 536; guests; every refusal; and a recorded timing.
"""
import time

import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth
from filtered_ref import candidate_mask, csr, delete_outside, filtered_topk, rows_of
from helpers import SENTINEL, assert_fp32_exact, exact_scores, record_measured
from test_gpu_rank_exact import cdae_model, int_model, load, make_data, special_rows
from test_gpu_rows import I_T, draw_uids, foreign, foreign_int_rows, gathered, trained

pytestmark = pytest.mark.gpu

NO_USER = cdae_amd.NO_USER
TOPKS = (1, 10, 16, 17, 24)          # <= 16: matrix cores when K <= 256; 17, 24 and every K > 256: general path
EVAL_CHUNK = 32768                   # rows per launch group (cdae_hip.hip)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, msg=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{msg} ids")
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]), err_msg=f"{msg} scores")


def int_scores(p, ptr, col, uids):
    """the exact integer scores of every (row, item) for integer parameters p; the fp32-exactness of the inputs is asserted"""
    u = np.full(ptr.size - 1, NO_USER, dtype=np.uint32) if uids is None else uids
    Z, S, D, bq = exact_scores(ptr, col, **dict(p, Wu=gathered(p["Wu"], u, 0.0)))
    assert_fp32_exact(Z, D, bq)                      # a condition on the inputs, checked before the GPU is touched
    return S


def allow_lists(rng, I):
    """name -> ascending allow list (None: no list), aimed at the masks: whole 32-item tiles gone (the first, one inside, the last,
    partial one), one lane half of recommend_mfma_kernel only, exactly n items with some in the last tile, and a list whose places
    cross the tile boundaries differently from its ids"""
    ids = np.arange(I, dtype=np.uint32)
    out = {"none": None, "every": ids, "tiles": ids[~np.isin(ids // 32, (0, 3, (I - 1) // 32))], "half0": ids[(ids & 4) == 0], "third": ids[::3]}
    for n in (1, 7, 16, 17, 24, 33):
        out[f"n{n}"] = np.sort(np.r_[rng.choice(I - 32, n - n // 2, replace=False), I - 1 - rng.choice(32, n // 2, replace=False)]).astype(np.uint32)
    return out


def excl_rows(rng, I, rated, allow):
    """row r takes kind r % 5: empty; the rated row; all of allow (every place the sentinel); only items outside allow (no effect);
    random items, rated ones and not-allowed ones among them"""
    every = np.arange(I, dtype=np.uint32)
    al = every if allow is None else allow
    rows = []
    for r, row in enumerate(rated):
        kind = r % 5
        if kind == 0:
            rows.append(np.empty(0, np.uint32))
        elif kind == 1:
            rows.append(row.copy())
        elif kind == 2:
            rows.append(al.copy())
        elif kind == 3:
            rows.append(np.setdiff1d(every, al)[:int(rng.integers(0, 50))].astype(np.uint32))
        else:
            rows.append(np.sort(rng.choice(I, int(rng.integers(1, 61)), replace=False)).astype(np.uint32))
    return rows


# ---- 1. exact order on integer models ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,asymmetric", [(8, False), (61, True), (200, False), (250, True), (300, False), (300, True)])
def test_every_place_of_every_row(built, K, asymmetric):
    U, I, R = 129, 977, 301
    d = make_data(U, I, seed=K)
    model = cdae_model(d, K, asymmetric)
    rng = np.random.default_rng(2000 + K)
    rated = foreign_int_rows(rng, I, R)
    ptr, col = csr(rated)
    uids = draw_uids(rng, U, R)
    allows = allow_lists(rng, I)
    excls = {name: excl_rows(rng, I, rated, allow) for name, allow in allows.items()}
    ecsr = {name: csr(rows) for name, rows in excls.items()}
    seen_short = False
    for mode in ("random", "levels", "half0", "half1", "last", "low"):
        p = int_model(mode, U, I, K, asymmetric, seed=K + I)
        S = int_scores(p, ptr, col, uids)
        load(model, p)
        for name, allow in allows.items():
            if mode not in ("random", "levels") and name not in ("none", "tiles", "half0", "third", "n17", "n33"):
                continue                                 # (every list on the two dense models; the plateau models take the lists that cut them)
            excl = excls[name]
            for exclude_rated in (True, False):
                want = filtered_topk(S, rated, excl, allow, exclude_rated, max(TOPKS))
                seen_short |= bool(((want[0] != SENTINEL).sum(axis=1) < max(TOPKS)).any())
                for topk in TOPKS:
                    got = model.recommend_rows_filtered(ptr, col, uids, topk, exclude=ecsr[name], allow=allow, exclude_rated=exclude_rated,
                                                        with_scores=True)
                    same(got, (want[0][:, :topk], want[1][:, :topk]), f"{mode} allow {name} exclude_rated {exclude_rated} topk {topk}")
        if mode == "random":                             # without scores, without uids, without an excl CSR
            want = filtered_topk(S, rated, None, allows["third"], True, 17)
            for topk in (16, 17):
                np.testing.assert_array_equal(model.recommend_rows_filtered(ptr, col, uids, topk, allow=allows["third"]), want[0][:, :topk])
            S0 = int_scores(p, ptr, col, None)
            want = filtered_topk(S0, rated, None, allows["n33"], False, 17)
            for topk in (16, 17):
                same(model.recommend_rows_filtered(ptr, col, None, topk, allow=allows["n33"], exclude_rated=False, with_scores=True),
                     (want[0][:, :topk], want[1][:, :topk]))
    assert seen_short


# ---- 2. no filter equals recommend_rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [200, 300])
def test_no_filter_is_recommend_rows(built, K):
    model, d = trained(K)
    ptr, col, uids, _, _ = foreign()
    for topk in (10, 16, 17, 24):                        # K = 200: 10 and 16 on the matrix cores
        want = model.recommend_rows(ptr, col, uids, topk, with_scores=True)
        same(model.recommend_rows_filtered(ptr, col, uids, topk, with_scores=True), want, f"topk {topk}")
        empty = (np.zeros(ptr.size, np.int64), np.empty(0, np.uint32))
        same(model.recommend_rows_filtered(ptr, col, uids, topk, exclude=empty, allow=np.arange(I_T, dtype=np.uint32), with_scores=True), want,
             f"topk {topk}, an empty excl CSR and an allow list of every item")
        np.testing.assert_array_equal(model.recommend_rows_filtered(ptr, col, uids, topk), want[0])
    assert np.isfinite(want[1]).all() and np.unique(want[1]).size > 1000


# ---- 3. the deletion property on float models -------------------------------------------------------------------------------------
def float_filters(rng, rated):
    """(name, allow, excl rows) for the trained 977-item models"""
    ids = np.arange(I_T, dtype=np.uint32)
    allows = allow_lists(rng, I_T)
    return [(n, allows[n], excl_rows(rng, I_T, rated, allows[n])) for n in ("none", "third", "half0", "tiles", "n33", "n7")] + \
           [("random", np.sort(rng.choice(ids, 600, replace=False)), None)]


def whole_lists_general(model, ptr, col, uids):
    """recommend_rows at topk = num_items: every unrated item of every row, in order, with its score (general path)"""
    return model.recommend_rows(ptr, col, uids, I_T, with_scores=True)


def whole_lists_mfma(model, ptr, col, uids):
    """the same from the matrix cores: full_rank_rows with every unrated item as a target gives every score and every place"""
    rated = rows_of(ptr, col)
    every = np.arange(I_T, dtype=np.uint32)
    targets = [np.setdiff1d(every, r) for r in rated]
    tptr, tcol = csr(targets)
    ranks, scores = model.full_rank_rows(ptr, col, tptr, tcol, uids, with_scores=True)
    ids = np.full((len(rated), I_T), SENTINEL, dtype=np.uint32)
    sc = np.full((len(rated), I_T), -np.inf, dtype=np.float32)
    for r in range(len(rated)):
        a, b = tptr[r], tptr[r + 1]
        assert np.array_equal(np.sort(ranks[a:b]), np.arange(b - a))
        ids[r, ranks[a:b]] = tcol[a:b]
        sc[r, ranks[a:b]] = scores[a:b]
    return ids, sc


@pytest.mark.parametrize("K,topks,whole_of", [(300, (24,), whole_lists_general), (200, (17, 24), whole_lists_general),
                                              (200, (1, 10, 16), whole_lists_mfma)], ids=["general-300", "general-200", "mfma-200"])
def test_the_list_is_the_whole_list_with_the_rest_deleted(built, K, topks, whole_of):
    """matrix cores: the test of tile-row independence — in the packed sweep an allowed item sits in another row of another tile than in
    the full sweep full_rank_rows ran, and must get the same bits"""
    model, d = trained(K)
    ptr, col, uids, _, _ = foreign()
    rated = rows_of(ptr, col)
    whole = whole_of(model, ptr, col, uids)
    rng = np.random.default_rng(31 + K)
    for name, allow, excl in float_filters(rng, rated):
        masks = [candidate_mask(I_T, rated[r], None if excl is None else excl[r], allow, True) for r in range(len(rated))]
        for topk in topks:
            got = model.recommend_rows_filtered(ptr, col, uids, topk, exclude=None if excl is None else csr(excl), allow=allow, with_scores=True)
            same(got, delete_outside(whole[0], whole[1], masks, topk), f"{name} topk {topk}")


# ---- 4. exclude_rated = 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [200, 300])
def test_rated_items_as_candidates(built, K):
    model, d = trained(K)
    ptr, col, uids, _, _ = foreign()
    rated = rows_of(ptr, col)
    R = len(rated)
    unrated = [candidate_mask(I_T, r, None, None, True) for r in rated]
    # general path: every item comes back; without the rated ones it is recommend_rows' whole list
    everything = model.recommend_rows_filtered(ptr, col, uids, I_T, exclude_rated=False, with_scores=True)
    assert (everything[0] != SENTINEL).all() and all(np.array_equal(np.sort(everything[0][r]), np.arange(I_T)) for r in range(R))
    same(delete_outside(everything[0], everything[1], unrated, I_T), model.recommend_rows(ptr, col, uids, I_T, with_scores=True), "general")
    assert sum(np.isin(everything[0][r, :24], rated[r]).sum() for r in range(R)) > R // 4      # (rated items do stand near the head)
    if K <= 256:                                         # matrix cores: what is left of a top-16 list is a prefix of recommend_rows'
        top = model.recommend_rows_filtered(ptr, col, uids, 16, exclude_rated=False, with_scores=True)
        plain = model.recommend_rows(ptr, col, uids, 16, with_scores=True)
        left = delete_outside(top[0], top[1], unrated, 16)
        n = (left[0] != SENTINEL).sum(axis=1)
        assert (n < 16).any() and (n > 0).any()
        for r in range(R):
            np.testing.assert_array_equal(left[0][r, :n[r]], plain[0][r, :n[r]])
            np.testing.assert_array_equal(bits(left[1][r, :n[r]]), bits(plain[1][r, :n[r]]))
    # both paths: the rated rows handed over as exclusions are the rated rows excluded
    third = np.arange(0, I_T, 3, dtype=np.uint32)
    for topk in (10, 24):
        for allow in (None, third):
            same(model.recommend_rows_filtered(ptr, col, uids, topk, exclude=(ptr, col), allow=allow, exclude_rated=False, with_scores=True),
                 model.recommend_rows_filtered(ptr, col, uids, topk, allow=allow, with_scores=True), f"topk {topk}")


# ---- 5. position independence -----------------------------------------------------------------------------------------------------
def test_a_rows_bits_do_not_depend_on_the_call(built):
    U, I, K, R = 129, 97, 8, EVAL_CHUNK + 5
    rng = np.random.default_rng(55)
    train = [np.sort(rng.choice(I, int(rng.integers(1, 6)), replace=False)).astype(np.uint32) for _ in range(U)]
    tp, tc = csr(train)
    d = synth.Interactions(U, I, tp, tc, np.zeros(U + 1, np.int64), np.empty(0, np.uint32))
    model = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, batch_users=32))
    model.reset(d, seed=1)
    for ep in range(2):
        model.train_one_iteration(3, ep)                 # a float model: sigmoid hidden layer, real-valued scores
    lens = rng.integers(1, 6, R)
    flat = np.argsort(rng.random((R, I)), axis=1)[:, :10].astype(np.uint32)
    rated = [np.sort(flat[r, :lens[r]]) for r in range(R)]
    excl = [np.sort(flat[r, 5:5 + lens[(r + 1) % R]]) for r in range(R)]
    uids = draw_uids(rng, U, R)
    ptr, col = csr(rated)
    eptr, ecol = csr(excl)
    small = np.r_[np.arange(150), np.arange(R - 150, R)]              # rows of both chunks of the big call

    def call(rows, topk, allow):
        p, c = csr([rated[r] for r in rows])
        return model.recommend_rows_filtered(p, c, uids[rows], topk, exclude=csr([excl[r] for r in rows]), allow=allow, with_scores=True)
    for allow in (None, np.setdiff1d(np.arange(I), np.arange(2, I, 5)).astype(np.uint32)):
        for topk in (16, 17):                            # matrix cores (two launch groups), general path
            big = model.recommend_rows_filtered(ptr, col, uids, topk, exclude=(eptr, ecol), allow=allow, with_scores=True)
            assert np.unique(bits(big[1][:300])).size > 500
            same(call(small, topk, allow), (big[0][small], big[1][small]), f"topk {topk}: the small call")
            back = call(small[::-1], topk, allow)
            same((back[0][::-1], back[1][::-1]), (big[0][small], big[1][small]), f"topk {topk}: reversed")
            for r in (0, 77, EVAL_CHUNK - 1, EVAL_CHUNK, R - 1):
                same(call(np.array([r]), topk, allow), (big[0][r:r + 1], big[1][r:r + 1]), f"topk {topk}: row {r} alone")


# ---- 6. item spaces beyond RATED_LDS_WORDS * 32 -----------------------------------------------------------------------------------
def test_more_than_65536_items(built):
    """70 001 items: 2 188 words per row, filter_bits_kernel's global-memory form (2 188 % 4 == 0 but the allow list of 66 003 items has
    2 063 words: rows start off a 16-byte boundary); the general path keeps its scores in the global workspace for both; a list of 50
    items goes back to LDS on both sides"""
    U, I, K, R = 40, 70_001, 8, 40
    d = make_data(U, I, seed=K, which=("tiles", "lowest"))
    model = cdae_model(d, K, False)
    rng = np.random.default_rng(6)
    rated = list(special_rows(rng, I, ("tiles", "half1", "lowest", "leaves7", "leaves24")).values()) + [np.empty(0, np.uint32)]
    rated += [np.sort(rng.choice(I, size=int(rng.integers(1, 41)), replace=False)).astype(np.uint32) for _ in range(R - len(rated))]
    ptr, col = csr(rated)
    uids = draw_uids(rng, U, R)
    ids = np.arange(I, dtype=np.uint32)
    big = np.setdiff1d(ids, np.r_[rng.choice(I, 3990, replace=False), np.arange(64, 72)]).astype(np.uint32)
    allows = {"none": None, "66k": big, "50": np.sort(np.r_[rng.choice(I - 32, 40, replace=False), I - 1 - np.arange(10)]).astype(np.uint32)}
    assert (I + 31) // 32 > 2048 and (big.size + 31) // 32 > 2048 and ((big.size + 31) // 32) % 4 != 0 and big.size * 4 + 64 > 160 * 1024
    for mode in ("random", "last"):
        p = int_model(mode, U, I, K, False, seed=K + 1, wmax=1)
        S = int_scores(p, ptr, col, uids)
        load(model, p)
        for name, allow in allows.items():
            excl = excl_rows(rng, I, rated, allow)
            for exclude_rated in (True, False):
                want = filtered_topk(S, rated, excl, allow, exclude_rated, 17)
                for topk in (10, 17):
                    got = model.recommend_rows_filtered(ptr, col, uids, topk, exclude=csr(excl), allow=allow, exclude_rated=exclude_rated, with_scores=True)
                    same(got, (want[0][:, :topk], want[1][:, :topk]), f"{mode} allow {name} exclude_rated {exclude_rated} topk {topk}")


# ---- 7. guests and NO_USER --------------------------------------------------------------------------------------------------------
def test_guest_rows_are_served_like_recommend_rows_serves_them(built):
    K = 200
    model, d = trained(K)
    ptr, col, uids, _, _ = foreign()
    rated = rows_of(ptr, col)
    R = len(rated)
    rng = np.random.default_rng(17)
    try:
        model.set_guest_nodes(rng.normal(0, 0.3, (R, K)).astype(np.float32))
        guests = cdae_amd.GUEST_USER(np.arange(R))
        guests[::7] = NO_USER
        guests[3::7] = uids[3::7]
        for topk in (10, 24):
            plain = model.recommend_rows(ptr, col, guests, topk, with_scores=True)
            assert not np.array_equal(plain[0], model.recommend_rows(ptr, col, uids, topk))
            same(model.recommend_rows_filtered(ptr, col, guests, topk, with_scores=True), plain, f"topk {topk}")
        allow = np.arange(1, I_T, 3, dtype=np.uint32)
        excl = excl_rows(rng, I_T, rated, allow)
        masks = [candidate_mask(I_T, rated[r], excl[r], allow, True) for r in range(R)]
        for topk, whole_of in ((16, whole_lists_mfma), (24, whole_lists_general)):
            whole = whole_of(model, ptr, col, guests)
            same(model.recommend_rows_filtered(ptr, col, guests, topk, exclude=csr(excl), allow=allow, with_scores=True),
                 delete_outside(whole[0], whole[1], masks, topk), f"filtered, topk {topk}")
    finally:
        model.set_guest_nodes(np.zeros((0, K), np.float32))
    with pytest.raises(cdae_amd.CDAEError, match="guest"):
        model.recommend_rows_filtered(ptr, col, guests, 10)


# ---- 8. refusals and state --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_and_its_parameters_as_they_were(built):
    """(the data set, configuration and seeds of test_gpu_parity's two-epoch bit-identity tests: training there is reproducible bit
    for bit, so "an epoch after the refusals gives the bits it would have given" can be asserted against a twin handle)"""
    U, I, K, R = 1200, 500, 40, 301
    d = synth.generate(U, I, 60_000, seed=9)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64)
    model = cdae_amd.CDAE(cfg)
    model.reset(d, seed=5)
    model.train_one_iteration(5, 0)
    rng = np.random.default_rng(7)
    rated = foreign_int_rows(rng, I, R)
    ptr, col = csr(rated)
    uids = draw_uids(rng, U, R)
    allow = np.arange(0, I, 3, dtype=np.uint32)
    excl = excl_rows(rng, I, rated, allow)
    eptr, ecol = csr(excl)
    big = int(np.argmax(np.diff(eptr) >= 2))             # an excl row with at least two items
    a = int(eptr[big])

    params = [w for w in range(12) if _has(model, w)]
    before = {w: model.get(w).copy() for w in params}
    plain = {topk: model.recommend_rows(ptr, col, uids, topk, with_scores=True) for topk in (10, 17)}
    good = {topk: model.recommend_rows_filtered(ptr, col, uids, topk, exclude=(eptr, ecol), allow=allow, with_scores=True) for topk in (10, 17)}
    for w in params:                                     # a filtered call changes no parameter
        np.testing.assert_array_equal(bits(model.get(w)), bits(before[w]))

    def ecol_with(f):
        c = ecol.copy(); f(c); return (eptr, c)

    def allow_with(f):
        c = allow.copy(); f(c); return c

    def swap(c, i):
        c[i], c[i + 1] = c[i + 1], c[i]
    bad_ptr = eptr.copy(); bad_ptr[5] = bad_ptr[6] + 1
    bad = [(dict(allow=allow_with(lambda c: swap(c, 20))), r"position 21"), (dict(allow=allow_with(lambda c: c.__setitem__(9, c[8]))), r"position 9"),
           (dict(allow=allow_with(lambda c: c.__setitem__(c.size - 1, I))), rf"allow_items\[{allow.size - 1}\]"),
           (dict(allow=np.empty(0, np.uint32)), "n_allow = 0"),
           (dict(exclude=ecol_with(lambda c: swap(c, a))), f"excl row {big}"), (dict(exclude=ecol_with(lambda c: c.__setitem__(a + 1, c[a]))), f"excl row {big}"),
           (dict(exclude=ecol_with(lambda c: c.__setitem__(a, I))), f"excl row {big}"), (dict(exclude=(bad_ptr, ecol)), "excl row_ptr decreases at row 5"),
           (dict(topk=0), "topk"), (dict(topk=I + 1), "topk"), (dict(uids=np.where(np.arange(R) == 5, U, uids).astype(np.uint32)), "row 5")]
    twin = cdae_amd.CDAE(cfg)                            # an epoch after the refusals must be the epoch without them
    twin.reset(d, seed=5)
    twin.train_one_iteration(5, 0)
    for w in params:
        np.testing.assert_array_equal(bits(twin.get(w)), bits(before[w]), err_msg=f"parameter {w}: the twin")
    for kw, word in bad:
        args = dict(row_ptr=ptr, col=col, uids=uids, topk=10, exclude=(eptr, ecol), allow=allow)
        args.update(kw)
        with pytest.raises(cdae_amd.CDAEError, match=word):
            model.recommend_rows_filtered(**args)
        for topk in (10, 17):
            same(model.recommend_rows(ptr, col, uids, topk, with_scores=True), plain[topk], f"after {word}")
            same(model.recommend_rows_filtered(ptr, col, uids, topk, exclude=(eptr, ecol), allow=allow, with_scores=True), good[topk], f"after {word}")
    # topk above the allow list's size is no error: the surplus places hold the sentinel
    ids = model.recommend_rows_filtered(ptr, col, uids, 16, allow=allow[:5])
    assert (ids[:, 5:] == SENTINEL).all() and (ids[:, 0] != SENTINEL).any()
    model.train_one_iteration(5, 1); twin.train_one_iteration(5, 1)
    for w in params:
        np.testing.assert_array_equal(bits(model.get(w)), bits(twin.get(w)), err_msg=f"parameter {w} after an epoch")
    twin.close()
    # no rows: success, nothing touched
    assert model.recommend_rows_filtered(np.zeros(1, np.int64), np.empty(0, np.uint32), None, 10).shape == (0, 10)
    assert model.lib.cdae_hip_recommend_rows_filtered(model.h, 0, None, None, None, None, None, 1, None, 0, 10, None, None) == 0
    # an IMF / BPR handle; a handle without interactions
    mf = cdae_amd.MF(cdae_amd.MFConfig(num_dim=8, batch_users=1))
    mf.reset(d, seed=1)
    with pytest.raises(cdae_amd.CDAEError, match="IMF / BPR"):
        mf.recommend_rows_filtered(ptr, col, None, 10, allow=allow)
    np.testing.assert_array_equal(mf.recommend_all(10).shape, (U, 10))           # (still usable)
    mf.close()
    fresh = cdae_amd.CDAE(model.cfg)
    with pytest.raises(cdae_amd.CDAEError, match="set_interactions"):
        fresh.recommend_rows_filtered(ptr, col, None, 10, allow=allow)
    fresh.close()


def _has(model, which):
    try:
        return model.get(which).size > 0
    except cdae_amd.CDAEError:
        return False


# ---- 9. recorded, not asserted ----------------------------------------------------------------------------------------------------
def test_timing_of_a_category_page_is_recorded(built):
    """An allow list of 1 / 32 of a 20 000-item catalogue, 4 096 rows, top-10, K = 200: the filtered call, the unfiltered
    recommend_rows(topk = 10), and the only alternative before — recommend_rows deep enough to leave 10 allowed items in every row,
    filtered on the host.  Median of five after a warm call, a synchronisation around each; handed to helpers.record_measured as
    rows_filtered.  No ratio is asserted: n_allow / num_items is only the bound on the sweep's share."""
    U, I, K, R, topk = 512, 20_000, 200, 4096, 10
    d = synth.generate(U, I, U * 30, seed=4, min_items=5)
    model = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64))
    model.reset(d, seed=3)
    model.train_one_iteration(3, 0)
    rng = np.random.default_rng(9)
    ptr, col = csr([np.sort(rng.choice(I, int(rng.integers(1, 61)), replace=False)).astype(np.uint32) for _ in range(R)])
    uids = rng.integers(0, U, R).astype(np.uint32)
    allow = np.sort(rng.choice(I, I // 32, replace=False)).astype(np.uint32)
    allowed = np.zeros(I, dtype=bool)
    allowed[allow] = True

    def deep_enough():
        depth = 512
        while True:
            ids = model.recommend_rows(ptr, col, uids, depth)
            if (allowed[np.minimum(ids, I - 1)] & (ids != SENTINEL)).sum(axis=1).min() >= topk or depth == I:
                return depth
            depth = min(2 * depth, I)
    depth = deep_enough()

    def host_filter():
        ids = model.recommend_rows(ptr, col, uids, depth)
        ok = allowed[np.minimum(ids, I - 1)] & (ids != SENTINEL)
        first = np.argsort(~ok, axis=1, kind="stable")[:, :topk]
        return np.take_along_axis(ids, first, axis=1)

    def median_of_five(f):
        f()
        times = []
        for _ in range(5):
            model.synchronize(); t0 = time.perf_counter(); out = f(); model.synchronize(); times.append(time.perf_counter() - t0)
        return float(np.median(times)), out
    t_filtered, got = median_of_five(lambda: model.recommend_rows_filtered(ptr, col, uids, topk, allow=allow))
    t_plain, _ = median_of_five(lambda: model.recommend_rows(ptr, col, uids, topk))
    t_host, _ = median_of_five(host_filter)
    record_measured("rows_filtered", rows=R, items=I, n_allow=allow.size, depth=depth, filtered_s=t_filtered, unfiltered_s=t_plain, deep_host_filter_s=t_host)
    print(f"rows_filtered: filtered {1e3 * t_filtered:.3f} ms, unfiltered top-{topk} {1e3 * t_plain:.3f} ms, "
          f"recommend_rows(topk={depth}) + host filter {1e3 * t_host:.3f} ms")
    assert allowed[got].all() and (got != SENTINEL).all()
