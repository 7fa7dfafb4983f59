"""-m gpu: batched top-k item neighbours by dot product or cosine (cdae_hip_similar_items).

The contract (include/cdae_hip.h) is exact, and every comparison here is assert_array_equal on the ids and on the bit patterns of the
scores, over every query and every place; no tolerance appears anywhere:
  * the documented order on tables whose every fp32 dot product is exact in any order (tests/similar_ref.py; the condition is asserted
    on the inputs before the GPU is touched): integer tables for the dot product, and for the cosine rows of exactly 1, 4 or 16
    non-zeros of one power-of-two magnitude, whose norm is m, 2m or 4m and whose normalised entries are +-1, +-1/2 or +-1/4 —
    identical rows by the hundred, all-zero rows (as items and as queries), plateaus in one lane half and in the last tile, allow lists
    and excl rows aimed at the masks of both top-k kernels;
  * on float tables, the library against what it already pins: the dot product against recommend_rows of one-item rows on a linear,
    bias-free model; the cosine against the dot product on a handle loaded with the reference's normalised table; s(q, i) against s(i, q);
  * position independence across the chunk boundary; item spaces beyond 65 536; IMF / BPR, asymmetric and full_output handles; every
    refusal; and a recorded timing.
"""
import ctypes as C
import time

import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth
from filtered_ref import csr
from helpers import SENTINEL, record_measured
from similar_ref import assert_exact_products, lists_of, normalise, operand, scores
from test_gpu_rank_exact import bias_pattern, cdae_model, int_model, make_data
from test_gpu_rows_filtered import allow_lists, bits, excl_rows, same

pytestmark = pytest.mark.gpu

TOPKS = (1, 10, 16, 17, 24)          # <= 16: matrix cores when K <= 256; 17, 24 and every K > 256: general path
EVAL_CHUNK = 32768                   # queries per launch group (cdae_hip.hip)
MODES = ("random", "levels", "half0", "half1", "last", "low")
TABLE_OF = {"output": lambda asymmetric: "V" if asymmetric else "W", "input": lambda asymmetric: "W"}


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def zero_rows(I):
    return np.array([7, 36, 333, I - 33, I - 1])         # all-zero rows: early, inside, in the last tile, the last item


def dot_table(mode, I, K, seed):
    """integers, float64 [I, K].  random: int_model's random rows, [100, 320) one and the same row (ties by ascending id); else
    int_model's one row r for every item times 1 + bias_pattern(mode): s(q, i) = l_q l_i |r|^2, the plateaus of bias_pattern."""
    T = int_model(mode, 1, I, K, False, seed, wmax=2 if I < 10_000 else 1)["W"]
    if mode == "random":
        T[100:320] = T[100]
    else:
        T = T * (1 + bias_pattern(mode, I))[:, None]
    T[zero_rows(I)] = 0.0
    return T


def cos_table(mode, I, K, seed):
    """rows of exactly 1, 4 or 16 (K < 16: 1 or 4) non-zeros +-m, m one power of two per row.  random: a random such row per item,
    [100, 320) one and the same direction at different magnitudes; else four directions of the most non-zeros, level l of
    bias_pattern(mode) the top direction with a quarter of its signs flipped 3 - l times: cosines 1, 1/2, 0, -1/2 with the top level."""
    rng = np.random.default_rng(seed)
    counts = (1, 4, 16) if K >= 16 else (1, 4)

    def direction(c):
        v = np.zeros(K)
        v[rng.choice(K, c, replace=False)] = rng.choice([-1.0, 1.0], c)
        return v
    if mode == "random":
        T = np.stack([direction(int(rng.choice(counts))) for _ in range(I)])
        T[100:320] = T[100]
    else:
        c = counts[-1]
        top = direction(c)
        at = np.flatnonzero(top)
        dirs = []
        for level in range(4):
            v = top.copy()
            v[at[:(3 - level) * c // 4]] *= -1.0
            dirs.append(v)
        T = np.stack(dirs)[bias_pattern(mode, I)]
    T = T * 2.0 ** rng.integers(-3, 4, I)[:, None]
    T[zero_rows(I)] = 0.0
    return T


def table(metric, mode, I, K, seed):
    return dot_table(mode, I, K, seed) if metric == "dot" else cos_table(mode, I, K, seed)


def exact_scores_of(T, queries, metric):
    """the scores of every (query, item), exact; the condition that makes them the library's fp32 bits is asserted on the operand"""
    assert_exact_products(operand(T, metric), 1.0 if metric == "dot" else 0.25, queries)
    return scores(T, queries, metric)


def draw_queries(rng, I, n):
    """zero rows, both ends of the identical block and of the plateaus, both lane halves, the last tile; then random ones, with repeats"""
    fixed = np.r_[zero_rows(I), 0, 4, 39, 40, 100, 101, 319, 320, I - 41, I - 40, I - 2, 7, 100, I - 1]
    return np.r_[fixed, rng.integers(0, I, n - fixed.size)].astype(np.uint32)


def set_tables(model, tables):
    for name, T in tables.items():
        model.set(getattr(cdae_amd, "P_" + name), T)


# ---- 1. exact order on exact grids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,I,asymmetric", [(8, 977, False), (61, 1023, True), (200, 961, False), (250, 992, True), (300, 977, False),
                                            (300, 961, True)])
def test_every_place_of_every_query(built, K, I, asymmetric):
    U, Q = 40, 301
    model = cdae_model(make_data(U, I, seed=K), K, asymmetric)
    p = int_model("random", U, I, K, asymmetric, seed=K)
    for name in ("b", "Wu", "bp"):                       # non-zero biases and user nodes: they take no part
        model.set(getattr(cdae_amd, "P_" + name.upper()), p[name])
    rng = np.random.default_rng(3000 + K)
    queries = draw_queries(rng, I, Q)
    own = [np.array([q], dtype=np.uint32) for q in queries]
    allows = allow_lists(rng, I)
    excls = {name: excl_rows(rng, I, own, allow) for name, allow in allows.items()}         # empty; the query; all of allow; outside allow; random
    ecsr = {name: csr(rows) for name, rows in excls.items()}
    seen_short = seen_zero_query = False
    for metric in ("dot", "cosine"):
        for mode in MODES:
            tables = {"W": table(metric, mode, I, K, seed=K + I)}
            if asymmetric:
                tables["V"] = table(metric, mode, I, K, seed=K + I + 1)
                assert not np.array_equal(tables["V"], tables["W"])
            set_tables(model, tables)
            for which in ("output", "input"):
                if which == "input" and mode not in ("random", "last"):
                    continue
                T = tables[TABLE_OF[which](asymmetric)]
                S = exact_scores_of(T, queries, metric)
                seen_zero_query |= bool((~S.any(axis=1)).any())
                for name, allow in allows.items():
                    if (mode != "random" or which == "input") and name not in ("none", "tiles", "half0", "third", "n17", "n33"):
                        continue                         # (every list on the dense table; the plateau tables take the lists that cut them)
                    for exclude_self in (True, False):
                        want = lists_of(S, queries, exclude_self, excls[name], allow, max(TOPKS))
                        seen_short |= bool(((want[0] != SENTINEL).sum(axis=1) < max(TOPKS)).any())
                        for topk in TOPKS:
                            got = model.similar_items(queries, topk, metric, which, exclude_self, exclude=ecsr[name], allow=allow, with_scores=True)
                            same(got, (want[0][:, :topk], want[1][:, :topk]),
                                 f"{metric} {mode} {which} allow {name} exclude_self {exclude_self} topk {topk}")
                if mode == "random":                     # without scores, without an excl CSR
                    want = lists_of(S, queries, True, None, allows["third"], 17)
                    for topk in (16, 17):
                        np.testing.assert_array_equal(model.similar_items(queries, topk, metric, which, allow=allows["third"]), want[0][:, :topk])
    assert seen_short and seen_zero_query


# ---- 2. float models: bit for bit against what the library already pins ---------------------------------------------------------------
I_F = 977


def float_model(K, T, **kw):
    """a symmetric linear CDAE with b = 0, Wu = 0, b' = 0 and the fp32 table T as W: the hidden row of the one-item row {q} is W[q]"""
    U = 40
    model = cdae_model(make_data(U, I_F, seed=K), K, False, **kw)
    model.set(cdae_amd.P_W, T); model.set(cdae_amd.P_B, np.zeros(K)); model.set(cdae_amd.P_WU, np.zeros((U, K))); model.set(cdae_amd.P_BP, np.zeros(I_F))
    return model


def float_table(K, seed=0):
    rng = np.random.default_rng(100 + K + seed)
    T = (rng.normal(0, 0.3, (I_F, K)) * rng.lognormal(0, 1, (I_F, 1))).astype(np.float32)
    T[[5, 500]] = 0.0
    return T


@pytest.mark.parametrize("K", [200, 300])
def test_the_dot_product_is_recommend_rows_of_one_item_rows(built, K):
    T = float_table(K)
    model = float_model(K, T)
    rng = np.random.default_rng(K)
    queries = np.r_[5, 500, rng.integers(0, I_F, 299)].astype(np.uint32)
    ptr, col = csr([np.array([q], dtype=np.uint32) for q in queries])
    for topk in (10, 24):                                # K = 200: 10 on the matrix cores
        want = model.recommend_rows(ptr, col, None, topk, with_scores=True)
        same(model.similar_items(queries, topk, "dot", "output", True, with_scores=True), want, f"topk {topk}")
        same(model.similar_items(queries, topk, "dot", "input", True, with_scores=True), want, f"topk {topk}, the input table of a tied model")
        both = model.recommend_rows_filtered(ptr, col, None, topk, exclude_rated=False, with_scores=True)
        same(model.similar_items(queries, topk, "dot", "output", False, with_scores=True), both, f"topk {topk}, the query a candidate")
    assert np.unique(want[1]).size > 1000 and np.isfinite(want[1]).all()


@pytest.mark.parametrize("K", [200, 300])
def test_the_cosine_is_the_dot_product_of_the_normalised_table(built, K):
    T = float_table(K)
    N = normalise(T)
    assert not N[[5, 500]].any() and np.isfinite(N).all()
    model, unit = float_model(K, T), float_model(K, N)
    rng = np.random.default_rng(K + 1)
    queries = np.r_[5, 500, rng.integers(0, I_F, 299)].astype(np.uint32)
    allow = np.sort(rng.choice(I_F, 600, replace=False)).astype(np.uint32)
    for topk in (10, 24):
        for al in (None, allow):
            for exclude_self in (True, False):
                want = unit.similar_items(queries, topk, "dot", "output", exclude_self, allow=al, with_scores=True)
                same(model.similar_items(queries, topk, "cosine", "output", exclude_self, allow=al, with_scores=True), want, f"topk {topk}")
    assert np.unique(want[1]).size > 1000
    zero = model.similar_items(np.array([5], np.uint32), 10, "cosine", with_scores=True)          # a zero query: +0.0 everywhere, never NaN
    np.testing.assert_array_equal(zero[0][0], [0, 1, 2, 3, 4, 6, 7, 8, 9, 10])
    np.testing.assert_array_equal(bits(zero[1]), np.zeros((1, 10), np.uint32))


@pytest.mark.parametrize("K", [200, 300])
def test_the_score_is_symmetric_bit_for_bit(built, K):
    model = float_model(K, float_table(K, seed=1))
    rng = np.random.default_rng(K + 2)
    sample = np.sort(rng.choice(I_F, 64, replace=False)).astype(np.uint32)
    for metric in ("dot", "cosine"):
        # general path: every pair in one call
        ids, sc = model.similar_items(sample, 64, metric, exclude_self=False, allow=sample, with_scores=True)
        G = np.empty((64, 64), np.float32)
        for r in range(64):
            assert np.array_equal(np.sort(ids[r]), sample)
            G[r, np.searchsorted(sample, ids[r])] = sc[r]
        np.testing.assert_array_equal(bits(G), bits(G.T), err_msg=f"{metric}, general path")
        if K <= 256:                                     # matrix cores: sixteen allowed items at a time, all sixteen places
            M = np.empty((64, 64), np.float32)
            for g in range(4):
                part = sample[16 * g:16 * g + 16]
                ids, sc = model.similar_items(sample, 16, metric, exclude_self=False, allow=part, with_scores=True)
                for r in range(64):
                    assert np.array_equal(np.sort(ids[r]), part)
                    M[r, np.searchsorted(sample, ids[r])] = sc[r]
            np.testing.assert_array_equal(bits(M), bits(M.T), err_msg=f"{metric}, matrix cores")
            assert np.unique(M).size > 1000


# ---- 3. position independence and chunking --------------------------------------------------------------------------------------------
def test_a_querys_bits_do_not_depend_on_the_call(built):
    I, K, Q = 977, 8, EVAL_CHUNK + 5
    rng = np.random.default_rng(55)
    T = rng.normal(0, 0.5, (I, K)).astype(np.float32)
    model = cdae_model(make_data(40, I, seed=3), K, False)
    model.set(cdae_amd.P_W, T)
    queries = rng.integers(0, I, Q).astype(np.uint32)
    excl = [np.sort(rng.choice(I, int(rng.integers(0, 6)), replace=False)).astype(np.uint32) for _ in range(Q)]
    eptr, ecol = csr(excl)
    small = np.r_[np.arange(150), np.arange(Q - 150, Q)]              # queries of both chunks of the big call

    def call(rows, topk, metric, allow):
        return model.similar_items(queries[rows], topk, metric, exclude=csr([excl[r] for r in rows]), allow=allow, with_scores=True)
    for metric in ("dot", "cosine"):
        for allow in (None, np.setdiff1d(np.arange(I), np.arange(2, I, 5)).astype(np.uint32)):
            for topk in (16, 17):                        # matrix cores (two launch groups), general path
                big = model.similar_items(queries, topk, metric, exclude=(eptr, ecol), allow=allow, with_scores=True)
                assert np.unique(bits(big[1][:300])).size > 500
                same(call(small, topk, metric, allow), (big[0][small], big[1][small]), f"{metric} topk {topk}: the small call")
                back = call(small[::-1], topk, metric, allow)
                same((back[0][::-1], back[1][::-1]), (big[0][small], big[1][small]), f"{metric} topk {topk}: reversed")
                for r in (0, 77, EVAL_CHUNK - 1, EVAL_CHUNK, Q - 1):
                    same(call(np.array([r]), topk, metric, allow), (big[0][r:r + 1], big[1][r:r + 1]), f"{metric} topk {topk}: query {r} alone")


# ---- 4. item spaces beyond RATED_LDS_WORDS * 32 ---------------------------------------------------------------------------------------
def test_more_than_65536_items(built):
    """70 001 items: 2 188 words per row, filter_bits_kernel's global-memory form (the allow list of 66 003 items has 2 063 words: rows
    start off a 16-byte boundary); the general path keeps its scores in the global workspace for both"""
    I, K, Q = 70_001, 8, 40
    model = cdae_model(make_data(40, I, seed=K, which=("tiles", "lowest")), K, False)
    rng = np.random.default_rng(6)
    queries = draw_queries(rng, I, Q)
    own = [np.array([q], dtype=np.uint32) for q in queries]
    ids = np.arange(I, dtype=np.uint32)
    big = np.setdiff1d(ids, np.r_[rng.choice(I, 3990, replace=False), np.arange(64, 72)]).astype(np.uint32)
    allows = {"none": None, "66k": big}
    assert (I + 31) // 32 > 2048 and (big.size + 31) // 32 > 2048 and ((big.size + 31) // 32) % 4 != 0 and big.size * 4 + 64 > 160 * 1024
    for metric in ("dot", "cosine"):
        for mode in ("random", "last"):
            T = table(metric, mode, I, K, seed=K + 1)
            model.set(cdae_amd.P_W, T)
            S = exact_scores_of(T, queries, metric)
            for name, allow in allows.items():
                excl = excl_rows(rng, I, own, allow)
                for exclude_self in (True, False):
                    want = lists_of(S, queries, exclude_self, excl, allow, 17)
                    for topk in (10, 17):
                        got = model.similar_items(queries, topk, metric, "output", exclude_self, exclude=csr(excl), allow=allow, with_scores=True)
                        same(got, (want[0][:, :topk], want[1][:, :topk]), f"{metric} {mode} allow {name} exclude_self {exclude_self} topk {topk}")


# ---- 5. handles -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairwise", [False, True])
def test_an_imf_or_bpr_handle_serves_its_item_factors(built, pairwise):
    I, K, Q = 977, 61, 301
    d = make_data(40, I, seed=K)
    m = cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, pairwise=pairwise, lt=cdae_amd.LOG if pairwise else cdae_amd.SQUARE, batch_users=8))
    m.reset(d, seed=1)
    rng = np.random.default_rng(K)
    queries = draw_queries(rng, I, Q)
    allow = allow_lists(rng, I)["third"]
    m.set(cdae_amd.P_BP, rng.integers(-4, 5, I))         # the item bias takes no part
    for metric in ("dot", "cosine"):
        T = table(metric, "random", I, K, seed=K)
        m.set(cdae_amd.P_W, T)
        S = exact_scores_of(T, queries, metric)
        for al in (None, allow):
            want = lists_of(S, queries, True, None, al, 17)
            for topk in (10, 17):
                for which in ("output", "input"):            # both name iv_
                    same(m.similar_items(queries, topk, metric, which, allow=al, with_scores=True), (want[0][:, :topk], want[1][:, :topk]),
                         f"{metric} {which} topk {topk}")
    np.testing.assert_array_equal(m.recommend_all(10).shape, (40, 10))
    m.close()


@pytest.mark.parametrize("K", [200, 300])
def test_an_asymmetric_model_has_two_tables(built, K):
    U = 40
    W, V = float_table(K), float_table(K, seed=7)
    model = cdae_model(make_data(U, I_F, seed=K), K, True)
    model.set(cdae_amd.P_W, W); model.set(cdae_amd.P_V, V)
    tied_w, tied_v = float_model(K, W), float_model(K, V)
    queries = np.arange(0, I_F, 3, dtype=np.uint32)
    for metric in ("dot", "cosine"):
        for topk in (10, 24):
            out = model.similar_items(queries, topk, metric, "output", with_scores=True)
            inp = model.similar_items(queries, topk, metric, "input", with_scores=True)
            same(out, tied_v.similar_items(queries, topk, metric, with_scores=True), f"{metric} output topk {topk}")
            same(inp, tied_w.similar_items(queries, topk, metric, with_scores=True), f"{metric} input topk {topk}")
            assert (out[0] != inp[0]).mean() > 0.9


def test_a_full_output_handle_is_served_from_its_fp32_rows(built):
    I, K, Q = 977, 50, 301
    d = make_data(40, I, seed=K)
    cfg = dict(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=32)
    model, plain = cdae_amd.CDAE(cdae_amd.CDAEConfig(full_output=True, **cfg)), cdae_amd.CDAE(cdae_amd.CDAEConfig(**cfg))
    model.reset(d, seed=1); plain.reset(d, seed=1)
    model.train_one_iteration(3, 0)                      # (its bf16 images exist and are of no concern)
    rng = np.random.default_rng(K)
    queries = draw_queries(rng, I, Q)
    F = float_table(K)
    model.set(cdae_amd.P_W, F); plain.set(cdae_amd.P_W, F)
    for metric in ("dot", "cosine"):
        for topk in (10, 17):
            same(model.similar_items(queries, topk, metric, with_scores=True), plain.similar_items(queries, topk, metric, with_scores=True),
                 f"float {metric} topk {topk}")
        T = table(metric, "random", I, K, seed=K)
        model.set(cdae_amd.P_W, T)
        want = lists_of(exact_scores_of(T, queries, metric), queries, True, None, None, 17)
        for topk in (10, 17):
            same(model.similar_items(queries, topk, metric, with_scores=True), (want[0][:, :topk], want[1][:, :topk]), f"{metric} topk {topk}")
        model.set(cdae_amd.P_W, F)


# ---- 6. refusals and state ------------------------------------------------------------------------------------------------------------
def _has(model, which):
    try:
        return model.get(which).size > 0
    except cdae_amd.CDAEError:
        return False


def test_refusals_leave_the_handle_and_its_parameters_as_they_were(built):
    """(the data set, configuration and seeds of test_gpu_parity's two-epoch bit-identity tests: training there is reproducible bit
    for bit, so "an epoch after the refusals gives the bits it would have given" can be asserted against a twin handle)"""
    U, I, K, Q = 1200, 500, 40, 301
    d = synth.generate(U, I, 60_000, seed=9)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64)
    model = cdae_amd.CDAE(cfg)
    model.reset(d, seed=5)
    model.train_one_iteration(5, 0)
    rng = np.random.default_rng(7)
    queries = rng.integers(0, I, Q).astype(np.uint32)
    own = [np.array([q], dtype=np.uint32) for q in queries]
    ptr, col = csr(own)
    allow = np.arange(0, I, 3, dtype=np.uint32)
    excl = excl_rows(rng, I, own, allow)
    eptr, ecol = csr(excl)
    big = int(np.argmax(np.diff(eptr) >= 2))             # an excl row with at least two items
    a = int(eptr[big])

    params = [w for w in range(12) if _has(model, w)]
    before = {w: model.get(w).copy() for w in params}
    plain = {topk: model.recommend_rows(ptr, col, None, topk, with_scores=True) for topk in (10, 17)}
    good = {(topk, metric): model.similar_items(queries, topk, metric, exclude=(eptr, ecol), allow=allow, with_scores=True)
            for topk in (10, 17) for metric in ("dot", "cosine")}
    for w in params:                                     # a call changes no parameter
        np.testing.assert_array_equal(bits(model.get(w)), bits(before[w]))

    def ecol_with(f):
        c = ecol.copy(); f(c); return (eptr, c)

    def allow_with(f):
        c = allow.copy(); f(c); return c

    def swap(c, i):
        c[i], c[i + 1] = c[i + 1], c[i]
    bad_ptr = eptr.copy(); bad_ptr[5] = bad_ptr[6] + 1
    bad = [(dict(items=np.where(np.arange(Q) == 9, I, queries).astype(np.uint32)), rf"query_items\[9\] = {I}"),
           (dict(allow=allow_with(lambda c: swap(c, 20))), r"position 21"), (dict(allow=allow_with(lambda c: c.__setitem__(9, c[8]))), r"position 9"),
           (dict(allow=allow_with(lambda c: c.__setitem__(c.size - 1, I))), rf"allow_items\[{allow.size - 1}\]"),
           (dict(allow=np.empty(0, np.uint32)), "n_allow = 0"),
           (dict(exclude=ecol_with(lambda c: swap(c, a))), f"excl row {big}"), (dict(exclude=ecol_with(lambda c: c.__setitem__(a + 1, c[a]))), f"excl row {big}"),
           (dict(exclude=ecol_with(lambda c: c.__setitem__(a, I))), f"excl row {big}"), (dict(exclude=(bad_ptr, ecol)), "excl row_ptr decreases at row 5"),
           (dict(topk=0), "topk"), (dict(topk=I + 1), "topk")]
    twin = cdae_amd.CDAE(cfg)                            # an epoch after the refusals must be the epoch without them
    twin.reset(d, seed=5)
    twin.train_one_iteration(5, 0)
    for w in params:
        np.testing.assert_array_equal(bits(twin.get(w)), bits(before[w]), err_msg=f"parameter {w}: the twin")

    def still_right(word):
        for topk in (10, 17):
            same(model.recommend_rows(ptr, col, None, topk, with_scores=True), plain[topk], f"after {word}")
            for metric in ("dot", "cosine"):
                same(model.similar_items(queries, topk, metric, exclude=(eptr, ecol), allow=allow, with_scores=True), good[(topk, metric)], f"after {word}")
    for kw, word in bad:
        args = dict(items=queries, topk=10, exclude=(eptr, ecol), allow=allow)
        args.update(kw)
        with pytest.raises(cdae_amd.CDAEError, match=word):
            model.similar_items(**args)
        still_right(word)
    out = np.empty((Q, 10), np.uint32)
    for table_id, metric_id, word in ((2, 0, b"unknown table 2"), (0, 2, b"unknown metric 2")):
        rc = model.lib.cdae_hip_similar_items(model.h, Q, queries.ctypes.data, table_id, metric_id, 1, None, None, None, 0, 10, out.ctypes.data, None)
        assert rc != 0 and word in model.lib.cdae_hip_last_error()
        still_right(word.decode())
    rc = model.lib.cdae_hip_similar_items(model.h, Q, queries.ctypes.data, 0, 0, 1, None, None, None, 0, 10, None, None)
    assert rc != 0 and b"out_ids" in model.lib.cdae_hip_last_error()
    with pytest.raises(ValueError):
        model.similar_items(queries, 10, metric="jaccard")
    # topk above the allow list's size is no error: the surplus places hold the sentinel
    ids = model.similar_items(queries, 16, allow=allow[:5])
    assert (ids[:, 5:] == SENTINEL).all() and (ids[:, 0] != SENTINEL).all()
    model.train_one_iteration(5, 1); twin.train_one_iteration(5, 1)
    for w in params:
        np.testing.assert_array_equal(bits(model.get(w)), bits(twin.get(w)), err_msg=f"parameter {w} after an epoch")
    twin.close()
    # no queries: success, nothing touched
    assert model.similar_items(np.empty(0, np.uint32), 10).shape == (0, 10)
    assert model.lib.cdae_hip_similar_items(model.h, 0, None, 0, 1, 1, None, None, None, 0, 10, None, None) == 0
    # an item shard; a handle without interactions
    mm = cdae_amd.MultiCDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, linear=True, batch_users=32), devices=[0, 0], item_rows=True)
    mm.reset(d, seed=1)
    shard = C.c_void_p()
    assert mm.lib.cdae_hip_multi_shard(mm.h, 0, C.byref(shard), None, None) == 0
    rc = mm.lib.cdae_hip_similar_items(shard, Q, queries.ctypes.data, 0, 0, 1, None, None, None, 0, 10, out.ctypes.data, None)
    assert rc != 0 and b"item shard" in mm.lib.cdae_hip_last_error()
    np.testing.assert_array_equal(mm.recommend_all(10).shape, (U, 10))           # (still usable)
    mm.close()
    fresh = cdae_amd.CDAE(model.cfg)
    with pytest.raises(cdae_amd.CDAEError, match="set_interactions"):
        fresh.similar_items(queries, 10)
    fresh.close()
    model.close()


# ---- 7. recorded, not asserted --------------------------------------------------------------------------------------------------------
def test_timing_of_an_item_table_is_recorded(built):
    """The full item-to-item table of a 20 000-item catalogue, K = 200: every item a query, top-10 by cosine, in one call (the matrix
    cores).  Median of five whole calls after a warm one, a synchronisation around each; handed to helpers.record_measured as
    similar_items.  There is no earlier code path to compare against, so no ratio is fixed."""
    U, I, K, topk = 512, 20_000, 200, 10
    d = synth.generate(U, I, U * 30, seed=4, min_items=5)
    model = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64))
    model.reset(d, seed=3)
    model.train_one_iteration(3, 0)
    queries = np.arange(I, dtype=np.uint32)
    got = model.similar_items(queries, topk)
    times = []
    for _ in range(5):
        model.synchronize(); t0 = time.perf_counter(); got = model.similar_items(queries, topk); model.synchronize(); times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    record_measured("similar_items", queries=I, items=I, num_dim=K, topk=topk, cosine_table_s=t)
    print(f"similar_items: {I} x {I} cosine top-{topk}, K = {K}: {1e3 * t:.3f} ms per call, {I / t:.0f} queries / s")
    assert (got != SENTINEL).all() and (got != queries[:, None]).all()
