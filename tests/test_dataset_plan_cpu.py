"""CPU: the data-set plan of cdae_hip_set_interactions (cdae_amd/csrc/cdae_dataset_plan.h), compiled by g++ into a small library
(tests/native/dataset_plan_cpu.cpp) and compared EXACTLY with its numpy restatement (tests/plan_ref.py), on the smallest inputs at
which each rule can go wrong.  Every case also states what it expects in plain numbers, so that slice and restatement cannot be wrong
together unnoticed.
"""
import os
import subprocess

import numpy as np
import pytest

import plan_ref as pr
from cdae_amd import P_B, P_B_AG, P_BP, P_BP_AG, P_V, P_V_AG, P_W, P_W_AG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_slice():
    src = os.path.join(ROOT, "tests", "native", "dataset_plan_cpu.cpp")
    hdr = os.path.join(ROOT, "cdae_amd", "csrc", "cdae_dataset_plan.h")
    out = os.path.join(ROOT, "build", "libcdae_dataset_plan_cpu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    return out


@pytest.fixture(scope="module")
def sl():
    return pr.Slice(build_slice())


def csr(rows):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, np.array([i for r in rows for i in r], np.uint32)


def rand_rows(rng, U, I, lo, hi):
    return [sorted(rng.choice(I, int(rng.integers(lo, hi + 1)), replace=False).tolist()) for _ in range(U)]


def both(sl, rows, I, **kw):
    """the plan of the slice, after it has been found equal to numpy's"""
    ptr, col = csr(rows)
    kw = dict(dict(U=len(rows), I=I, row_ptr=ptr, col=col, K=24, Kp=64, num_neg=5), **kw)
    got, want = sl.plan(**kw), pr.plan(sl.limits, **kw)
    assert pr.same(got, want) == [], (got, want)
    return got


B = 4
KINDS = dict(cdae={}, full=dict(full_output=1, num_neg=0), imf=dict(kind=1), bpr=dict(kind=2), imf_seq=dict(kind=1, mf_seq=1), wrmf=dict(kind=3, mf_seq=1))


def test_the_limits_come_from_the_header(sl):
    L = sl.limits
    assert set(L) >= {"LATE_MAX", "LATE_BITS_WORDS", "UNIT_POS_MAX", "BKC_MAX_RANGES", "BKC_ITEM_BITS", "BK_ITEMS", "BK_MAX_RANGES", "BK_CELL_UNITS_MAX",
                      "TILE_SORT_MAX_ITEMS", "DUP_STRIPES"}
    assert L["BK_ITEMS"] <= 1 << L["BKC_ITEM_BITS"] and L["BKC_MAX_RANGES"] <= L["BK_MAX_RANGES"] and L["LATE_MAX"] % 4 == 0


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("U", [1, B - 1, B, B + 1, 2 * B, 2 * B + 3, 3 * B])
def test_windows_units_and_activity_groups(sl, kind, U):
    rng = np.random.default_rng(100 * U + len(kind))
    rows = rand_rows(rng, U, 300, 1, 200)
    rows[-1] = list(range(250))                      # the heaviest user is the LAST one: the last window of B users holds the maximum
    p = both(sl, rows, 300, batch_users=B, **KINDS[kind])
    lens = np.array([len(r) for r in rows])
    grouped = kind in ("imf", "bpr") and U > B
    assert p["permuted"] == int(grouped)
    if grouped:
        perm = p["user_perm"]
        assert sorted(perm.tolist()) == list(range(U)) and np.array_equal(p["user_inv"][perm], np.arange(U))
        plens = lens[perm]
        # groups of B by descending activity; the short last group (the least active users) stays last
        groups = [plens[k:k + B] for k in range(0, U, B)]
        assert all((np.diff(g) <= 0).all() for g in groups)
        if U % B:
            assert sorted(groups[-1].tolist()) == sorted(lens.tolist())[:U % B]
        if U // B >= 3:                             # three full groups or more: the full ones are visited out of activity order
            assert [g[0] for g in groups[:U // B]] != sorted([g[0] for g in groups[:U // B]], reverse=True)
        lens = plens
    if kind == "wrmf":
        assert (p["Ecap"], p["unit_cap"], p["unit_ptr"].tolist()) == (0, 0, [0] * (U + 1))
        return
    n = min(B, U)
    best = max(int(lens[s:s + n].sum()) for s in range(U))
    assert p["emax"] == best and p["Ecap"] == best * p["ex_per_pos"] and p["B"] == n
    assert p["ex_per_pos"] == dict(cdae=6, full=1, imf=6, bpr=10, imf_seq=6)[kind]
    units = -(-lens // 64)
    assert np.array_equal(np.diff(p["unit_ptr"].astype(np.int64)), units) and np.array_equal(p["unit_user"], np.repeat(np.arange(U), units))
    assert p["unit_cap"] == max(max(int(units[s:s + n].sum()) for s in range(U)), int(np.sort(units)[::-1][:n].sum()))


@pytest.mark.parametrize("U,Bw", [(1, 4), (3, 4), (4, 4), (5, 4), (11, 4), (8, 4), (7, 1), (6, 100)])
def test_window_max_alone(sl, U, Bw):
    rng = np.random.default_rng(U * 7 + Bw)
    for heavy in range(U):                             # the maximum in every place, the last window and the truncated ones included
        lens = rng.integers(0, 5, U)
        lens[heavy] = 1000
        want = max(int(lens[s:s + Bw].sum()) for s in range(U))
        for t in (np.int64, np.uint32):
            prefix = np.concatenate([[0], np.cumsum(lens)]).astype(t)
            assert sl.window_max(prefix, U, Bw) == want == pr.window_max(prefix, U, Bw)


def test_encode_bound_exceeds_every_window(sl):
    rows = [list(range(200)) if u % 3 == 0 else [0] for u in range(10)]      # the heavy users are never neighbours
    p = both(sl, rows, 300, batch_users=3)
    assert p["unit_cap"] == 3 * 4 and pr.window_max(p["unit_ptr"], 10, 3) == 4 + 1 + 1


def hot_case(sl, I, pops, **kw):
    """64 users in one batch (share 1): item i is rated by the first pops[i] users"""
    rows = [[i for i in range(len(pops)) if u < pops[i]] for u in range(64)]
    return both(sl, rows, I, batch_users=64, **kw)


def test_hot_rows_round_up_to_four_capped_at_the_items(sl):
    # I = 1: only a handle that samples nothing may hold it (WRMF) — one hot row, not four
    assert hot_case(sl, 1, [64], kind=3, mf_seq=1)["hot_rows"] == 1
    # I = 3, all hot, on a sampled item shard (full local rows are legal there): hot and late rows are 3
    p = hot_case(sl, 3, [64, 64, 64], item_shard=1, I_global=9, whole_row_ptr=np.arange(65, dtype=np.int64) * 5)
    assert (p["hot_rows"], p["late_rows"], p["late_bits"].tolist()) == (3, 3, [7])
    # I = 5: three hot rows round to four; five hot rows round to eight and are capped at five
    rows = [[0, 1, 2] + ([3] if u < 47 else [])for u in range(64)]
    p = both(sl, rows, 5, batch_users=64)
    assert (p["hot_rows"], p["late_rows"]) == (4, 4) and p["late_bits"].tolist() == [0b1111]      # item 3 (47 expected positives) is taken along
    rows = [[i for i in range(5) if i != u % 5] for u in range(64)]
    assert min(both(sl, rows, 5, batch_users=64)["pop"]) >= 51 and both(sl, rows, 5, batch_users=64)["hot_rows"] == 5
    # I = 117: the thresholds are >= 48 expected positives; 6 hot rows -> 8, of which the late rows are the same 8
    p = hot_case(sl, 117, [64, 63, 50, 49, 48, 48, 47, 47, 1] + [2] * 100)
    assert (p["hot_rows"], p["late_rows"]) == (8, 8) and p["order"][:8].tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    # the two thresholds apart: 2 late rows -> 4, 5 hot rows -> 8
    p = hot_case(sl, 117, [64, 63, 50, 49, 48, 48, 47, 47, 1] + [2] * 100, hot_pos=49.0, late_pos=63.0)
    assert (p["hot_rows"], p["late_rows"]) == (4, 4)
    p = hot_case(sl, 117, [64, 63, 50, 49, 48, 48, 47, 47, 1] + [2] * 100, hot_pos=48.0, late_pos=63.0)
    assert (p["hot_rows"], p["late_rows"], int(p["late_bits"][0])) == (8, 4, 0b1111)
    # kinds without the hybrid decode have hot rows (reported as 0 by cdae_hip_decode_plan) and no late rows
    for kw in (dict(kind=1), dict(full_output=1, num_neg=0), dict(K=300, Kp=512), dict(no_late_rows=1)):
        p = hot_case(sl, 117, [64, 63, 50, 49, 48, 48, 47, 47, 1] + [2] * 100, **kw)
        assert (p["hot_rows"], p["late_rows"], p["late_bits"].size) == (8, 0, 0)


def test_late_rows_stop_at_late_max_and_at_the_bitmap(sl):
    L = sl.limits
    n = L["LATE_MAX"] + 6
    p = hot_case(sl, 117, [64] * n)
    assert (p["hot_rows"], p["late_rows"]) == ((n + 3) & ~3, L["LATE_MAX"]) and sum(bin(int(w)).count("1") for w in p["late_bits"]) == L["LATE_MAX"]
    wide = 32 * L["LATE_BITS_WORDS"]
    p = hot_case(sl, wide, [64] * n)
    assert (p["hot_rows"], p["late_rows"], p["late_bits"].size, p["bucket_on"]) == ((n + 3) & ~3, L["LATE_MAX"], L["LATE_BITS_WORDS"], 1)
    p = hot_case(sl, wide + 1, [64] * n)              # one item more than the LDS bitmap holds: no late rows (and no 16-bit keys)
    assert (p["hot_rows"], p["late_rows"], p["late_bits"].size, p["bucket_on"]) == ((n + 3) & ~3, 0, 0, 0)


def test_popularity_ties_keep_item_order(sl):
    rows = [[1, 3, 5, 6], [0, 1, 3, 6], [2, 3, 4, 6], [3, 6]]        # popularity 1 2 1 4 1 1 4 0
    p = both(sl, rows, 8, batch_users=2)
    assert p["pop"].tolist() == [1, 2, 1, 4, 1, 1, 4, 0] and p["order"].tolist() == [3, 6, 1, 0, 2, 4, 5, 7]
    assert p["rank_of"][p["order"]].tolist() == list(range(8))
    share, neg = 2 / 4, (2 / 4) * 14 * 5 / 8
    assert p["rank_len"].tolist() == [np.float32(c * share + neg) for c in (4, 4, 2, 1, 1, 1, 1, 0)]


def test_a_batch_too_small_for_any_hot_row(sl):
    rows = [[0, 1] for _ in range(200)]               # popularity 200, batch share 2 / 200: two expected positives
    p = both(sl, rows, 9, batch_users=2)
    assert (p["hot_rows"], p["late_rows"], p["late_bits"].size) == (0, 0, 0)
    p = both(sl, rows, 9, batch_users=48)             # 48 of 200 users: exactly the threshold
    assert (p["hot_rows"], p["late_rows"]) == (4, 4)
    p = both(sl, rows, 9, batch_users=47)
    assert (p["hot_rows"], p["late_rows"]) == (0, 0)


def test_bucket_ranges_cut_by_weight_and_by_width(sl):
    L = sl.limits
    rng = np.random.default_rng(3)
    rows = rand_rows(rng, 40, 117, 1, 60)
    p = both(sl, rows, 117, batch_users=8)
    assert p["bucket_on"] and p["cut"][0] == 0 and p["cut"][-1] == 117 and (np.diff(p["cut"].astype(np.int64)) > 0).all()
    assert np.array_equal(p["range_of"], np.repeat(np.arange(p["cut"].size - 1), np.diff(p["cut"].astype(np.int64))))
    # 20 000 items of weight 0.6 each: an eighth of the total would be 2 500 items, the width limit cuts at BK_ITEMS
    rows = [list(range(200 * u, 200 * u + 200)) for u in range(100)]
    p = both(sl, rows, 20000, batch_users=10)
    assert p["bucket_on"] and np.diff(p["cut"].astype(np.int64)).tolist() == [L["BK_ITEMS"]] * 9 + [20000 - 9 * L["BK_ITEMS"]]
    # who may not have it, and who has it without cells
    small = rand_rows(rng, 12, 50, 1, 20)
    assert both(sl, small, 50, batch_users=4)["range_of"].size == 50
    for kw, on, cells in ((dict(kind=1), 1, 0), (dict(kind=2), 1, 0), (dict(kind=1, mf_seq=1), 0, 0), (dict(sort_library=1), 0, 0), (dict(sort_tile=1), 0, 0),
                          (dict(sort_scan=1), 1, 0), (dict(full_output=1, num_neg=0), 1, 1)):
        p = both(sl, small, 50, batch_users=4, **kw)
        assert (p["bucket_on"], int(p["range_of"].size > 0), p["counting_sort"]) == (on, cells, int("sort_tile" in kw)), kw
    assert both(sl, small, L["TILE_SORT_MAX_ITEMS"] + 1, batch_users=4, sort_tile=1)["counting_sort"] == 0


def test_more_ranges_than_the_sort_has_workgroup_words(sl):
    """Pinned as it is: while the 65 536-key limit stands, no data set reaches this refusal (every range but the width-cut ones weighs
    at least 1/256 of the total: at most 256 + 32 ranges) — so the rule is driven alone, by items that weigh nothing."""
    L = sl.limits
    for I, want_on, want_cells in ((L["BKC_MAX_RANGES"], True, True), (L["BKC_MAX_RANGES"] + 1, True, False), (L["BK_MAX_RANGES"], True, False),
                                   (L["BK_MAX_RANGES"] + 1, False, False)):
        args = (10, I, 5, I, 100, 600000, float(I), 0.0, 0, np.zeros(I, np.uint64), 1, 1)
        on, cut, rof = sl.bucket_cuts(*args)
        ron, rcut, rrof = pr.bucket_cuts(*args, sl.limits)
        assert (on, rof is not None) == (want_on, want_cells) == (ron, rrof is not None)
        if on:
            assert np.array_equal(cut, rcut) and cut.tolist() == list(range(I + 1))
        if want_cells:
            assert np.array_equal(rof, rrof)
    # cells need the example index to fit beside BKC_ITEM_BITS bits of item
    top = 1 << (32 - L["BKC_ITEM_BITS"])
    for Ecap, cells in ((top - 1, True), (top, False)):
        assert (sl.bucket_cuts(10, 8, 5, 8, Ecap, top, 8.0, 40.0, 5, np.arange(8, dtype=np.uint64), 1, 1)[2] is not None) == cells


@pytest.mark.parametrize("full", [0, 1])
def test_bucket_sort_up_to_the_example_limit(sl, full):
    L = sl.limits
    limit = L["BUCKET_MAX_EXAMPLES_FULL"] if full else L["BUCKET_MAX_EXAMPLES_SAMPLED"]
    assert limit == (100000 if full else 600000)
    per = 1 if full else 6
    for extra, on in ((0, 1), (1, 0)):
        n = limit // per + extra                       # interactions of the one batch
        rows = [list(range(2000)) for _ in range(n // 2000)] + [list(range(n % 2000))] * (n % 2000 > 0)
        p = both(sl, rows, 4000, batch_users=len(rows), full_output=full, num_neg=0 if full else 5)
        assert (p["Ecap"], p["bucket_on"]) == (n * per, on)


def shard_case():
    # local items [0, 4) of 500: user 0 has none of them, user 1 all of them; the whole rows are far longer
    rows = [[], [0, 1, 2, 3], [1], [0, 3], [], [2]]
    whole = np.concatenate([[0], np.cumsum([3, 200, 130, 5, 70, 64])]).astype(np.int64)
    return rows, whole


def test_item_shard_takes_capacity_and_units_from_the_whole_rows(sl):
    rows, whole = shard_case()
    p = both(sl, rows, 4, batch_users=2, item_shard=1, I_global=500, whole_row_ptr=whole, own_u0=2, own_u1=5)
    assert (p["emax"], p["Ecap"], p["unit_cap"]) == (5, 330 * 6, 4 + 3) and (p["own_u0"], p["own_u1"]) == (2, 5)
    assert p["gunit_ptr"].tolist() == [0, 1, 5, 8, 9, 11, 12] and p["gunit_user"].tolist() == [0, 1, 1, 1, 1, 2, 2, 2, 3, 4, 4, 5]
    assert p["sort_bits"] == 3 and p["bucket_on"] == 1             # five keys: the four items and VOID
    p = both(sl, rows, 4, batch_users=2, item_shard=1, I_global=500, whole_row_ptr=whole)
    assert (p["own_u0"], p["own_u1"]) == (0, 6)                    # never set: every user
    # the full-output shard has no whole rows: its own (possibly empty) rows size everything; all rows empty: no examples, no bucket sort
    p = both(sl, rows, 4, batch_users=2, item_shard=1, I_global=500, full_output=1, num_neg=0)
    assert (p["Ecap"], p["unit_cap"], p["gunit_ptr"].size, p["sort_bits"]) == (5, 2, 0, 2)
    p = both(sl, [[], [], []], 4, batch_users=2, item_shard=1, I_global=500, full_output=1, num_neg=0)
    assert (p["Ecap"], p["bucket_on"], p["unit_cap"], p["hot_rows"]) == (0, 0, 0, 0)


def test_wrmf_item_major_rows(sl):
    rows = [[0, 4], [], [0, 1, 4], [4], [0, 1, 2, 4]]             # an empty row, item 3 in nobody's
    p = both(sl, rows, 5, kind=3, mf_seq=1, batch_users=256)
    assert p["tptr"].tolist() == [0, 3, 5, 6, 6, 10] and p["tcol"].tolist() == [0, 2, 4, 2, 4, 4, 0, 2, 3, 4]
    p = both(sl, [[], []], 3, kind=3, mf_seq=1, batch_users=256)
    assert p["tptr"].tolist() == [0, 0, 0, 0] and p["tcol"].tolist() == [0]


@pytest.mark.parametrize("asym", [0, 1])
def test_parameter_block(sl, asym):
    p = both(sl, [[0], [1]], 3, batch_users=2, asymmetric=asym, Kp=64)
    ids = [P_W, P_W_AG, P_V, P_V_AG, P_BP, P_BP_AG, P_B, P_B_AG]                 # the block's order: [W | W_ag | (V | V_ag) | bp | bp_ag | b | b_ag]
    want = [0, 192, 384, 576, 768, 771, 774, 838] if asym else [0, 192, 0, 0, 384, 387, 390, 454]
    assert p["off"][ids].tolist() == want and p["cnt"][ids].tolist() == [192, 192, 192 * asym, 192 * asym, 3, 3, 64, 64]
    rest = [i for i in range(p["off"].size) if i not in ids]
    assert (p["n_matrix"], p["n_shared"]) == ((768, 902) if asym else (384, 518)) and not p["off"][rest].any() and not p["cnt"][rest].any()


def test_unit_size_follows_the_batch(sl):
    rows = [[0]] * 1026
    assert both(sl, rows, 2, batch_users=1024)["unit_pos"] == 64 and both(sl, rows, 2, batch_users=1025)["unit_pos"] == sl.limits["UNIT_POS_MAX"]


REFUSALS = [
    ("row_ptr is not monotone at user 1", dict(rows=[[0], [1], [0]], ptr=[0, 2, 1, 3])),
    ("row_ptr is not monotone at user 2", dict(rows=[[0], [1], [0], [1]], ptr=[0, 1, 3, 2, 4], kind=1, batch_users=2)),      # found before the users are grouped
    ("user 1 has no training item (the reference CHECK-fails too, cdae.hpp:139)", dict(rows=[[0], [], [1]])),
    ("user 2 rated every item: no negative can be sampled", dict(rows=[[0], [1], [0, 1, 2]])),
    ("item id 3 out of range at position 2", dict(rows=[[0, 1], [3]])),
    ("row 1 is not strictly ascending at position 3", dict(rows=[[0, 1], [1, 1]])),
    ("row 0 is not strictly ascending at position 1", dict(rows=[[2, 0]])),
    ("owned user range [1, 4) outside the 3 users", dict(rows=[[0], [], [1]], item_shard=1, full_output=1, own_u0=1, own_u1=4)),
    ("owned user range [3, 2) outside the 3 users", dict(rows=[[0], [], [1]], item_shard=1, full_output=1, own_u0=3, own_u1=2)),
    ("whole-row row_ptr[0] must be 0", dict(rows=[[0], [], [1]], item_shard=1, I_global=9, whole_row_ptr=np.array([1, 2, 3, 4], np.int64))),
    ("batch_users 1024 x row stride 524288 floats exceeds the 2 GiB the batch's Z may occupy; lower batch_users", dict(rows=[[0]] * 1025, batch_users=1024, Kp=1 << 19)),
    ("batch of 2 users holds 4294967298 examples (> 2^32); lower batch_users", dict(rows=[[0], [1], [0]], batch_users=2, num_neg=1 << 31)),
]


@pytest.mark.parametrize("text,case", REFUSALS, ids=[t[:28] for t, _ in REFUSALS])
def test_every_refusal_and_its_text(sl, text, case):
    case = dict(case)
    ptr, col = csr(case.pop("rows"))
    if "ptr" in case:
        ptr = np.array(case.pop("ptr"), np.int64)
    kw = dict(dict(U=ptr.size - 1, I=3, row_ptr=ptr, col=col, K=24, Kp=64, num_neg=5, batch_users=4), **case)
    assert sl.plan(**kw) == text == pr.plan(sl.limits, **kw)


def test_the_kinds_exempt_from_the_row_refusals(sl):
    rows = [[], [0, 1, 2]]                            # an empty and a full row: an item shard's slices and WRMF's rows may be either
    assert both(sl, rows, 3, batch_users=2, item_shard=1, full_output=1, num_neg=0)["pop"].tolist() == [1, 1, 1]
    assert both(sl, rows, 3, kind=3, mf_seq=1, batch_users=256)["pop"].tolist() == [1, 1, 1]
    assert isinstance(sl.plan(U=2, I=3, row_ptr=csr(rows)[0], col=csr(rows)[1], Kp=64, batch_users=2, kind=1), str)
    # FISM: a user without train items takes no step, so a row may be empty; a full one leaves no negative to draw and is refused
    p = both(sl, [[], [0, 1], [], []], 3, kind=5, mf_seq=1, asymmetric=1, batch_users=1)
    assert p["pop"].tolist() == [1, 1, 0] and p["unit_ptr"].tolist() == [0] * 5 and (p["Ecap"], p["unit_cap"]) == (0, 0)
    kw = dict(U=2, I=3, row_ptr=csr(rows)[0], col=csr(rows)[1], K=24, Kp=64, num_neg=5, batch_users=1, kind=5, mf_seq=1, asymmetric=1)
    assert sl.plan(**kw) == "user 1 rated every item: no negative can be sampled" == pr.plan(sl.limits, **kw)
    # the 2 GiB limit is on the largest batch, not on batch_users: fewer users than that are fine
    assert both(sl, [[0]] * 1023, 2, batch_users=1 << 20, Kp=1 << 19)["B"] == 1023
