"""-m gpu: the sampled training step (the step bench.py times) against oracle/cdae_oracle.cpp at every decode tier and dispatch seam.

launch_decode (cdae_hip.hip) picks the K <= 256 decode by nv = K / 64 and nt = 0 / 1 / 2 / 4 for a tail of 0 / < 16 / < 32 / more:
sixteen (NV, NT) tiers, each instantiated for CE / SQUARE x AdaGrad / SGD, each once as decode_gather_kernel (the fused launch) and
once as decode_hybrid_kernel (two launches); above 256 the decode is decode_rows_kernel<8>.  With NT > 0 the output bias b' rides in
the last tail slot of the row image, element 64 NV + 16 NT - 1 >= K, and is taken out again before the row is stored; with NT == 0 it
is a scalar on another code path.  The other tests train at K = 1, 16, 24, 40, 50, 64, 72, 100, 130, 200, 256, 300 and 512: seven tiers
and every seam were never trained.  Here:

  (1) every high edge of a tier (K = 15 .. 256: the bias slot is the only spare slot of the row image; at 63 and 255 the last element of
      the padded row), 257, 511 and 512 with all four loss / optimiser pairs, every low edge with two of them, on D400, B = 150;
  (2) in the same cases, the tables as they lie on the device: columns [:K] the bits `get` returns, columns [K:] exactly zero — top-k
      and scoring contract over the padded stride;
  (3) the step's other switches (asymmetric, linear_function, no user factor + tanh, num_neg 1 and 12, two corruptions, no corruption)
      rotated over K = 95, 128, 159, 191, 192, 223, 255;
  (4) item rows of hundreds of examples per batch (ring wrap at 128 examples, parked g falling back to per-chunk stores) at NT = 1, 2,
      0, 4;
  (5) the sequential schedule (batch_users = 1) against the oracle's literal restatement.

Training is not bit-for-bit against a CPU yardstick (rows move during a batch, in an order: tests/test_gpu_fold_in_exact.py), so the
yardstick is the fp64 block schedule at the project's bound — 2e-4 of the parameter's range after two epochs (max_param_err;
test_batched_schedule_matches_oracle, test_wide_rows), 3e-4 for (4) (test_item_rows_with_thousands_of_examples_per_batch) — plus the
two invariants that ARE exact: the fused launch and the two separate launches (set_decode_fused) leave the same bits in every
parameter, and the pad columns are zero.  An off-by-one in the dispatch or a bias left in its slot is a gross error in one column or
one bias, not rounding noise.  With CDAE_RECORD_MEASURED every case appends its worst error as step_tier_K<k>_B<b>_<variant>
(profiles/step_tiers_measured.txt holds a run).

What the file found: with num_neg = 12 on D400 (56 000 duplicate negatives among a batch's 86 000 examples) neither launch shape
reproduced its own bits from run to run — the correction rows are handed out from 16 stripes of 4096, the sort's 30 workgroups
overflowed some while others had room, and those examples took the decode's atomics fallback.  Handles whose sort has at most 32
workgroups now use one stripe (cdae_hip.hip); the neg12 cases below fail without that.

D400: 400 users x 200 items.  Items 0 .. 79 are rated with probability 0.5, 80 .. 196 with 0.02, 197 .. 199 by nobody (empty rows; the
last four-row wavefront is partial), three users rate 150 items each (rows longer than one unit).  At B = 150 the 80 popular rows are
hot rows, 64 of them late rows, and the launch is fused (tests/plan_ref.py decode_split: popularity x B / U >= 48); asserted on the
handle below.
"""
import numpy as np
import pytest

import cdae_amd
from cdae_amd import CROSS_ENTROPY, P_UU, P_V, P_W, P_WU, SQUARE, synth
from helpers import PARAMS, make_pair, max_param_err, record_measured
from test_gpu_als import device_table
from test_gpu_parity import few_items_many_users

pytestmark = pytest.mark.gpu

BOUND, BOUND_LONG = 2e-4, 3e-4
SEED = 11                                   # make_pair's default: the twin handle starts from the same parameters
COMPARED = (0, 1, 4, 5, 6, 7, 8, 9)         # W, Wu, b, b' and their accumulators, bit for bit between the two launch shapes
B400 = 150

HIGH_EDGES = [15, 31, 63, 64, 79, 95, 127, 128, 143, 159, 191, 192, 207, 223, 255, 256]
ABOVE_256 = [257, 511, 512]
LOW_EDGES = [1, 16, 32, 65, 80, 96, 129, 144, 160, 193, 208, 224]
# SQUARE with plain SGD at 0.002, not CE's 0.01: a SQUARE step is a contraction only while learn_rate x 2 (sum z^2 + 1) < 2, and sum z^2
# grows with K (z in (0, 1)).  At 0.01 the fp64 oracle ALONE runs to 1e164 on D400 at K = 511 and 512 (|W| reaches 7 at 257), and
# below that it sits close enough to the edge that two runs of it started half an fp32 ulp apart end 1.8e-4 of W's range apart at
# K = 65: nothing a 2e-4 bound can be held against.  At 0.002 the same probe gives at most 1.2e-6 over every K of the lists, and W
# still moves by 0.9 .. 1.3 in the two epochs.
PAIRS = {"ce_adagrad": dict(loss=CROSS_ENTROPY), "ce_sgd": dict(loss=CROSS_ENTROPY, using_adagrad=False, learn_rate=0.01),
         "sq_adagrad": dict(loss=SQUARE), "sq_sgd": dict(loss=SQUARE, using_adagrad=False, learn_rate=0.002)}
SWITCHES = [("asym_sq", dict(asymmetric=True, loss=SQUARE)), ("linfun", dict(linear_function=True)),
            ("nouf_tanh", dict(user_factor=False, tanh=True)), ("neg1", dict(num_neg=1)), ("neg12", dict(num_neg=12)),
            ("nc2", dict(num_corruptions=2)), ("nocorrupt", dict(corruption_ratio=0.0, scaled=False))]
SWITCH_KS = [95, 128, 159, 191, 192, 223, 255]
# K number i takes switches i and i + 3 (mod 7): every K two switches, every switch two K
SWITCH_CASES = [(K, *SWITCHES[(i + s) % 7]) for i, K in enumerate(SWITCH_KS) for s in (0, 3)]


def tier_of(K):
    """(NV, NT) as launch_decode picks them, restated"""
    tail = K % 64
    return K // 64, 0 if tail == 0 else 1 if tail < 16 else 2 if tail < 32 else 4


def test_the_case_lists_cover_every_tier_and_seam():
    tiers = {(nv, nt) for nv in range(4) for nt in (1, 2, 4)} | {(nv, 0) for nv in (1, 2, 3, 4)}
    assert len(tiers) == 16 and {tier_of(K) for K in HIGH_EDGES} == tiers                # all four pairs in every tier
    assert {tier_of(K) for K in LOW_EDGES} == {t for t in tiers if t[1]}                 # an NT = 0 tier is one K: its high edge
    for K in HIGH_EDGES + LOW_EDGES:                                                   # the row image: K elements, and b' where NT > 0
        nv, nt = tier_of(K)
        assert 64 * nv + 16 * nt >= K + (nt > 0)
    assert all(K == 256 or tier_of(K) != tier_of(K + 1) for K in HIGH_EDGES)             # each one the last K of its tier,
    assert {K + 1 for K in HIGH_EDGES} <= set(HIGH_EDGES + LOW_EDGES + ABOVE_256)         # the next K trained as well
    assert sorted(K for K in HIGH_EDGES if tier_of(K)[1] and 64 * tier_of(K)[0] + 16 * tier_of(K)[1] == K + 1) == \
        [15, 31, 63, 79, 95, 127, 143, 159, 191, 207, 223, 255]                          # b' in the only spare slot
    for K in SWITCH_KS:
        assert sum(1 for c in SWITCH_CASES if c[0] == K) == 2
    assert len({c[1] for c in SWITCH_CASES}) == 7


def make_d400():
    rng = np.random.default_rng(400)
    U, I = 400, 200
    R = rng.random((U, I)) < np.r_[np.full(80, 0.5), np.full(117, 0.02), np.zeros(3)]
    for u in (7, 199, 393):                                                            # one long row in each batch of 150
        R[u] = False
        R[u, rng.choice(197, 150, replace=False)] = True
    ptr = np.r_[0, np.cumsum(R.sum(axis=1))].astype(np.int64)
    col = np.nonzero(R)[1].astype(np.uint32)                                           # row-major: ascending inside a row
    return synth.Interactions(U, I, ptr, col, np.zeros(U + 1, np.int64), np.empty(0, np.uint32))


@pytest.fixture(scope="module")
def d400(built):
    d = make_d400()
    pop = np.bincount(d.train_col, minlength=200)
    lens = np.diff(d.train_ptr)
    assert (d.num_users, d.num_items) == (400, 200) and not pop[197:].any() and pop[:197].all() and lens.min() >= 1
    assert sorted(np.flatnonzero(lens == 150).tolist()) == [7, 199, 393] and (np.delete(lens, [7, 199, 393]) < 64).all()
    m, _ = make_pair(d, K=16, B=B400)
    plan, batch = m.decode_plan, m.batch_users
    m.close()
    assert batch == B400                                                                # batches of 150, 150, 100
    assert plan["late_rows"] == 64, plan
    assert plan["hot_rows"] > plan["late_rows"], plan                                   # hot rows that are not late
    assert plan["hot_rows"] < 197, plan                                                 # cold four-row groups, the last one partial
    assert plan["fused"], plan
    return d


@pytest.fixture(scope="module")
def long_rows(built):
    return few_items_many_users()


@pytest.fixture(scope="module")
def tiny(built):
    return synth.generate_shape("tiny", seed=5)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def errors_by_row(m, o):
    """for a failing case: per parameter the worst relative error, the median row's, and the rows that carry the worst — a wrong
    column or a stale row shows as a few rows off by 1e-2 or more, rounding as a smooth spread"""
    out = {}
    for which in PARAMS:
        ref = o.get(which)
        if not ref.size:
            continue
        got = m.get(which).astype(np.float64)
        rows = got.shape[0]
        err = np.abs(got.ravel() - ref).reshape(rows, -1).max(axis=1) / (1e-3 + np.abs(ref).max())
        out[which] = (float(err.max()), float(np.median(err)), np.argsort(err)[::-1][:4].tolist())
    return out


def assert_clean_pads(m, data, K):
    """the weight tables as they lie on the device: [:K] what `get` returns, [K:] zero (the accumulators' pads hold 1 by design)"""
    cfg = m.cfg
    tables = [(P_W, data.num_items)]
    if cfg.user_factor:
        tables.append((P_WU, data.num_users))
    if cfg.asymmetric:
        tables.append((P_V, data.num_items))
    if cfg.linear_function:
        tables.append((P_UU, data.num_users))
    for which, rows in tables:
        host = m.get(which)
        T = device_table(m, which, rows)
        assert T.shape[1] in (64, 128, 256, 512) and T.shape[1] >= K, T.shape
        np.testing.assert_array_equal(bits(T[:, :K]), bits(host), err_msg=f"parameter {which}")
        dirty = np.argwhere(T[:, K:] != 0)
        assert not dirty.size, (which, K, "pad not zero at (row, column - K)", dirty[:8].tolist(), T[:, K:][tuple(dirty[0])])


def train(m, seed, epochs):
    for ep in range(epochs):
        st = m.train_one_iteration(seed=seed, epoch=ep)
        assert st.users == m.num_users * m.cfg.num_corruptions
    return {w: m.get(w) for w in COMPARED}


def run_case(data, K, B, variant, tag, *, epochs=2, seed=4, bound=BOUND, literal=False, expect_fused=None):
    """expect_fused True: the premise that the handle takes the fused launch is asserted; None: both launch shapes where it does"""
    m, o = make_pair(data, K=K, B=B, seed=SEED, **variant)
    assert m.batch_users == B
    plan = m.decode_plan
    if K > 256:
        assert plan["late_rows"] == 0 and not plan["fused"], plan                      # one launch shape: decode_rows_kernel
    elif expect_fused:
        assert plan["fused"] and plan["late_rows"] > 0, plan
    fused = train(m, seed, epochs)
    if plan["fused"]:
        twin = cdae_amd.CDAE(m.cfg)
        twin.reset(data, seed=SEED)
        twin.set_decode_fused(False)
        assert not twin.decode_plan["fused"] and twin.decode_plan["late_rows"] == plan["late_rows"]
        apart = train(twin, seed, epochs)
        for w in COMPARED:
            np.testing.assert_array_equal(bits(fused[w]), bits(apart[w]), err_msg=f"parameter {w}: fused launch vs separate launches")
        if K % 64:
            assert_clean_pads(twin, data, K)
        twin.close()
    for ep in range(epochs):
        if literal:
            o.train_literal(seed, ep)
        else:
            o.train_batched(seed, ep, B)
    err, which = max_param_err(m, o)
    name = f"step_tier_K{K}_B{B}_{tag}"
    print(f"\n{name}: {err:.3g} (parameter {which}) tier {tier_of(K) if K <= 256 else 'rows'} plan {plan}")
    record_measured(name, err=err)
    for w in PARAMS:                                         # (max_param_err is blind to NaN: a comparison with NaN is False)
        if o.get(w).size:
            assert np.isfinite(o.get(w)).all(), ("the yardstick itself diverges at these hyper-parameters", w)
            assert np.isfinite(m.get(w)).all(), w
    if K % 64:
        assert_clean_pads(m, data, K)
    assert err < bound, (err, which, errors_by_row(m, o))
    m.close()


# ---- (1) + (2): every tier, every instantiation, both launch shapes, the pads -----------------------------------------------------------
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("K", HIGH_EDGES + ABOVE_256)
def test_high_edge_of_every_tier_in_all_four_pairs(d400, K, pair):
    run_case(d400, K, B400, PAIRS[pair], pair, expect_fused=True)


@pytest.mark.parametrize("pair", ["ce_adagrad", "sq_sgd"])
@pytest.mark.parametrize("K", LOW_EDGES)
def test_low_edge_of_every_tier(d400, K, pair):
    run_case(d400, K, B400, PAIRS[pair], pair, expect_fused=True)


# ---- (3): the other switches of the step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,tag,variant", SWITCH_CASES, ids=[f"{K}-{t}" for K, t, _ in SWITCH_CASES])
def test_switches_of_the_step_over_the_untrained_tiers(d400, K, tag, variant):
    """asym_sq: the decoder is V, the input rows are W; linfun: the per-user gate Uu; neg12 on 200 items: many duplicate negatives, i.e.
    correction rows and runs on late rows; nc2: two corruptions per user"""
    run_case(d400, K, B400, variant, tag, expect_fused=True)


# ---- (4): long chains ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [15, 95, 192, 255])
def test_long_chains_at_every_tail_form(long_rows, K):
    """60 items, 1500 users per batch: a row holds hundreds to thousands of examples of one batch — the ring of two 64-example chunks
    wraps at 128, the popular rows outgrow the LDS room of their parked g — at NT = 1, 2, 0, 4"""
    assert [tier_of(k)[1] for k in (15, 95, 192, 255)] == [1, 2, 0, 4]
    run_case(long_rows, K, 1500, dict(num_neg=3), "long_neg3", epochs=1, bound=BOUND_LONG)


def make_long_cold():
    """2000 users x 60 items: items 0 .. 23 as popular as few_items_many_users' (4 .. 13 of them per user), items 24 .. 59 rated by 40
    users each — at B = 1500 below the hot-row threshold, yet every one of them is drawn as a negative some 700 times per batch"""
    rng = np.random.default_rng(12)
    U, I, POPULAR = 2000, 60, 24
    p = 1.0 / np.arange(1, POPULAR + 1) ** 0.8
    p /= p.sum()
    R = np.zeros((U, I), bool)
    for u in range(U):
        R[u, rng.choice(POPULAR, size=int(rng.integers(4, 14)), replace=False, p=p)] = True
    for i in range(POPULAR, I):
        R[rng.choice(U, size=40, replace=False), i] = True
    ptr = np.r_[0, np.cumsum(R.sum(axis=1))].astype(np.int64)
    return synth.Interactions(U, I, ptr, np.nonzero(R)[1].astype(np.uint32), np.zeros(U + 1, np.int64), np.empty(0, np.uint32))


@pytest.fixture(scope="module")
def long_cold(built):
    return make_long_cold()


@pytest.mark.parametrize("K", [15, 95, 192, 255])
def test_long_chains_in_the_four_row_role(long_cold, K):
    """In few_items_many_users every row is a hot row at B = 1500 (one row per wavefront: decode_row64, which knows no NT) — a mutation of
    decode_rows16's scalar-bias path at K = 192 passed the four cases above.  Here 36 rows stay in four-row wavefronts with chains of
    some 700 examples per batch: eleven 64-example chunks through the ring of two, g written out per chunk, at NT = 1, 2, 0, 4."""
    d, B, num_neg = long_cold, 1500, 3
    pop = np.bincount(d.train_col, minlength=d.num_items)
    share = B / d.num_users
    assert (pop[24:] * share < 48).all() and (pop[:24] * share >= 48).all()                  # tests/plan_ref.py decode_split
    assert share * d.train_ptr[-1] * num_neg / d.num_items > 8 * 64                          # negatives per row and full batch
    m, _ = make_pair(d, K=16, B=B, num_neg=num_neg)
    plan = m.decode_plan
    m.close()
    assert plan["hot_rows"] == 24 and plan["late_rows"] == 24, plan
    run_case(d, K, B, dict(num_neg=num_neg), "longcold_neg3", epochs=1, bound=BOUND_LONG)


# ---- (5): the sequential schedule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [15, 95, 192, 255, 257])
def test_sequential_schedule_against_the_literal_restatement(tiny, K):
    run_case(tiny, K, 1, dict(), "literal", seed=7, literal=True)
