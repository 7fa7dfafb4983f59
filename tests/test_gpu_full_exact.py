"""-m gpu: the full-output decode against the bf16-faithful oracle (Oracle.train_full(..., bf16=True)), one block at a time.

The other full-output tests compare the device with the fp64 oracle within a few per cent of each parameter's range, or one device
path with another bit for bit; neither sees a fault that moves a few elements a little, or one that every path shares (the loss
epilogue's masking, the positive fix-up, the b' sums, the padding of Kp / Ip / Bp).  The faithful oracle rounds z, D and g to bf16
exactly where the device does (oracle/cdae_oracle.cpp train_users_full), so what is left between the two is fp32 arithmetic.  On the
unfused plans (K > 256, CDAE_FULL_UNFUSED) full_positive_fixup_kernel recomputes a positive's y from the fp32 z and decoder rows
rather than their bf16 images; those cases run the oracle with unrounded_positives=True.  An item-rows shard takes the plan of a
single handle of the same K: the fused kernel at K <= 256 (no fix-up), the unfused products above.

Tier A — exact known-answer step.  SQUARE, SGD, linear hidden layer, lambda = 0, learn rate 2^-4, scale 1 or 2, every parameter an
integer multiple of 2^-4 (asymmetric values, most of them small).  Then z is on the 2^-4 grid, y = z . D + b' on 2^-8, g = 2 (y - t)
on 2^-7 (bf16 rounding of an on-grid value stays on the grid), hg and dD on 2^-11, b' sums on 2^-7 and every stepped value on 2^-15.
Each case asserts, from the operands themselves, that every contraction's sum of |terms| stays below 2^24 units of its grid, so that
every partial sum the device forms — in any order, any MFMA grouping, any split — is exact in fp32, and that every value after the
step is an fp32 value.  The device must then equal the faithful oracle BIT FOR BIT in every parameter.  The cases of the unfused
plans also assert that the block holds positives whose loss gradient differs between one bf16 rounding (bf16(2 y - 2)) and two
(bf16(bf16(2 y) - 2)), the defect full_positive_fixup_kernel used to have: b' of the positive items is 1 + a few grid steps, so
that y of a positive is 1 + an odd multiple of 2^-8 for many of them.

Tier B — realistic values.  Counter-stream initialisation, one block of training, then b' of the block's positive items raised so
that > 90 % of the positives sit at p > 0.99 (CE), or > 35 % at y within 1/8 of 1 (SQUARE), accumulators zeroed; then one block against
the faithful oracle, comparing the decoder rows V (asymmetric: V takes dD alone) and b'.  Bound, element by element, for the
difference of one SGD / AdaGrad step (from zero accumulators u -> u / (beta + |u|) is 1/beta-Lipschitz, so an error e in the
summed gradient moves the parameter by at most lr e / beta; SGD: lr e):
  * fp32 term: the device sums nb products g z (exact in fp32: bf16 x bf16) in fp32 — at most nb 2^-24 sum_u |g z| — and rounds
    the step (<= 2^-23 |p| for the update, 2^-22 |p| with the AdaGrad division);
  * flip term: where the device's value and the oracle's exact one straddle a bf16 rounding boundary, the two roundings differ by
    one bf16 ulp (two, allowed, at a binade edge).  A flip is allowed wherever it is possible: for z where the fp32 z (within
    2^-20 |z| of the fp64 one) can round either way; for g where the exact g, moved by the largest fp32 error of y (K 2^-24 sum
    |z D| + 2^-24 |y| for adding b' + the possible z flips, times the loss' slope: 2 for SQUARE, 1/4 for CE) and by the device's exp / rcp
    (2^-21 |g| + 2^-22), can.  (An unfused plan's positive: y from K fp32 products of the fp32 z and V, K 2^-24 sum |z V| +
    2^-20 sum |z V| for the fp32 z against the fp64 one + 2^-24 |y|.)  It adds lr / beta (sum_u 2 ulp(g) |z| [g may flip] + sum_u |g| 2 ulp(z) [z may flip]).
The double rounding's error on a well-fit positive is an ABSOLUTE 2^-9 (CE) or 2^-8 (SQUARE), tens to hundreds of ulps of its g.
The share of elements beyond the fp32 term alone must stay below 2 %.  (CE caveat: the negatives of a raised item sit at p ~ 1
too, where one ulp of g is 2^-8; the allowance for their possible flips can exceed the error of a few positives, so the CE cases
guard the bound, and the SQUARE cases and tier A are the ones that tell one rounding from two.)
"""
import numpy as np
import pytest
import torch

import cdae_amd
from cdae_amd import binding as PLAN
from cdae_amd import synth
import oracle as orc
from oracle import binding as ob

pytestmark = pytest.mark.gpu

E = 4                                    # parameters on the 2^-E grid
LR = 2.0 ** -4
SEED = 5


def bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64).astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def bf16_ulp(x):
    a = np.maximum(np.abs(bf16(x)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def make_data(U, I, max_pos, rng):
    """U users, each rating 1 .. max_pos distinct items (every user at least one)"""
    rows = [np.sort(rng.choice(I, size=int(rng.integers(1, min(I, max_pos) + 1)), replace=False)) for _ in range(U)]
    ptr = np.zeros(U + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([r.size for r in rows])
    col = np.concatenate(rows).astype(np.uint32)
    return synth.Interactions(U, I, ptr, col, np.zeros(U + 1, dtype=np.int64), np.zeros(0, dtype=np.uint32))


def targets(data, nb, I):
    T = np.zeros((nb, I))
    for u in range(nb):
        T[u, data.train_col[data.train_ptr[u]:data.train_ptr[u + 1]]] = 1.0
    return T


def new_model(cfg, shards):
    if shards:
        m = cdae_amd.MultiCDAE(cfg, devices=[0] * shards, item_rows=True)
    else:
        m = cdae_amd.CDAE(cfg)
    return m


def oracle_of(model, data, cfg_kw):
    o = orc.Oracle(orc.OracleConfig(**cfg_kw), data.num_users, data.num_items, data.train_ptr, data.train_col)
    o.init_params(1)                                       # (sizes the parameters; every value is then the device's)
    for which in range(ob.P_COUNT):
        if o.get(which).size:
            try:
                o.set(which, model.get(which).astype(np.float64))
            except cdae_amd.CDAEError:                     # (not allocated in this configuration: V of a tied model)
                pass
    return o


def assert_plan(model, want_plan, shards, data, min_largest_shard=0):
    if shards:
        cuts = model.shards()
        assert len(cuts) == shards and cuts[0][0] == 0 and cuts[-1][1] == data.num_items, cuts
        assert max(b - a for a, b in cuts) >= min_largest_shard, cuts
    else:
        assert model.full_output_plan == want_plan, (model.full_output_plan, want_plan)


# ---- Tier A ------------------------------------------------------------------------------------------------------------------------
def grid(rng, shape, choices):
    return rng.choice(np.asarray(choices, dtype=np.float64), size=shape) * 2.0 ** -E


def tier_a(data, K, B, nb, *, asym, scale2, want_plan, shards=0, double_rounding=False, dense=0.3, min_largest_shard=0):
    """one block of nb users on the exact grid: premise, then bit equality with the faithful oracle.
    shards: MultiCDAE(item_rows=True) over that many logical shards; of want_plan only the FUSED bit then matters (every shard
    decodes with the fused kernel, or none does: the choice depends on K alone)"""
    rng = np.random.default_rng(K * 7919 + data.num_items * 31 + nb)
    U, I = data.num_users, data.num_items
    flags = dict(using_adagrad=False, asymmetric=asym, user_factor=True, linear=True, scaled=scale2, tanh=False, linear_function=False)
    hyper = dict(lambda_=0.0, learn_rate=LR, corruption_ratio=0.5 if scale2 else 0.0, beta=1.0, num_neg=5, num_corruptions=1)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.SQUARE, batch_users=B, full_output=True, **flags, **hyper)
    model = new_model(cfg, shards)
    model.reset(data, seed=3)
    assert_plan(model, want_plan, shards, data, min_largest_shard)
    sparse = [-2, -1] + [0] * int(6 * (1 - dense) / max(dense, 1e-3)) + [1, 3]      # asymmetric values, mostly 0
    params = {cdae_amd.P_W: grid(rng, (I, K), sparse), cdae_amd.P_WU: grid(rng, (U, K), [-1, 0, 0, 2]),
              cdae_amd.P_B: grid(rng, K, [-1, 0, 1, 3])}
    if asym:
        params[cdae_amd.P_V] = grid(rng, (I, K), sparse)
    T = targets(data, nb, I)
    pos_items = T.any(axis=0)
    bp = np.zeros(I)
    bp[pos_items] = 1.0 + rng.integers(-3, 4, int(pos_items.sum())) * 2.0 ** -E
    params[cdae_amd.P_BP] = bp
    for which, a in params.items():
        model.set(which, a.astype(np.float32))
        np.testing.assert_array_equal(model.get(which).astype(np.float64).ravel(), a.ravel())      # on the grid, fp32-exact
    o = oracle_of(model, data, dict(num_dim=K, loss_type=ob.LOSS_SQUARE, **flags, **hyper))
    # premise: the exact grid (module docstring)
    Z = o.encode(SEED, 0, 1, np.arange(nb, dtype=np.uint32))
    D = params[cdae_amd.P_V if asym else cdae_amd.P_W]
    Zr, Dr = bf16(Z), bf16(D)
    on = lambda x, e: np.array_equal(np.round(x * 2.0 ** e), x * 2.0 ** e)
    Y = Zr @ Dr.T + bp
    G = bf16(2.0 * (Y - T))
    units = {"y": (np.abs(Zr) @ np.abs(Dr).T + np.abs(bp), 8), "hg": (np.abs(G) @ np.abs(Dr), 11),
             "dD": (np.abs(G).T @ np.abs(Zr), 11), "db'": (np.abs(G).sum(axis=0), 7)}
    assert on(Z, E) and on(Zr, E) and on(Y, 2 * E) and on(G, 2 * E - 1)
    for name, (s, e) in units.items():
        assert s.max() * 2.0 ** e < 2.0 ** 24, (name, s.max() * 2.0 ** e)
    if not asym:          # tied: some decoder rows also take the block's input gradient (has_in in the rows-fused step)
        assert sum(o.draw_inputs(SEED, 0, u).size for u in range(nb)) > 0
    if double_rounding:   # positives where bf16(bf16(2y) - 2) != bf16(2y - 2)
        twice = bf16(bf16(2.0 * Y) - 2.0)
        n_diff = int(((twice != G) & (T == 1)).sum())
        assert n_diff > 0, "no positive tells one rounding from two"
    model.train_users(SEED, 0, 0, nb)
    o.train_full(SEED, 0, B, 0, nb, bf16=True, unrounded_positives=not want_plan & FUSED)
    for which in range(ob.P_COUNT):
        ref = o.get(which)
        if not ref.size or (which in (ob.P_V, ob.P_V_AG) and not asym):
            continue
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), ("oracle value off the fp32 grid", which)
        got = model.get(which).astype(np.float64).ravel()
        if not np.array_equal(got, ref):
            bad = np.flatnonzero(got != ref)
            raise AssertionError(f"param {which}: {bad.size} of {ref.size} elements differ, e.g. at {bad[:6]}: "
                                 f"device {got[bad[:6]]} oracle {ref[bad[:6]]}")


FUSED = PLAN.PLAN_FUSED_DECODE
TN = PLAN.PLAN_GEMM2_TN
ROWS = PLAN.PLAN_ROWS_FUSED

# (K, I, users, B, nb, asym, scale2, env, plan)
CASES_FUSED = [
    (1, 33, 40, 31, 31, True, True, {}, FUSED),
    (16, 2, 40, 33, 33, False, False, {}, FUSED),           # (one item: every user would rate all of it, which reset() refuses)
    (17, 31, 40, 128, 1, True, True, {}, FUSED),
    (63, 129, 140, 128, 128, False, True, {"CDAE_FULL_ONE_STREAM_MAX": "0"}, FUSED),
    (64, 4097, 60, 128, 33, True, False, {}, FUSED),
    (65, 129, 140, 256, 129, False, True, {}, FUSED),
    (129, 33, 40, 31, 31, False, True, {"CDAE_FULL_ONE_STREAM_MAX": "0"}, FUSED),
    (256, 4097, 140, 256, 129, True, True, {"CDAE_FULL_ONE_STREAM_MAX": "0"}, FUSED),
    (256, 129, 140, 128, 128, False, False, {}, FUSED),
    (64, 65537, 4, 48, 2, True, True, {}, FUSED),           # >= 32768 items at Kp <= 256: full_rows_wave_kernel, the row-major image only
]
CASES_UNFUSED = [
    (40, 4097, 60, 128, 33, False, True, {"CDAE_FULL_UNFUSED": "1"}, 0),
    (200, 129, 60, 48, 48, True, True, {"CDAE_FULL_UNFUSED": "1", "CDAE_FULL_ONE_STREAM_MAX": "0"}, 0),
    (300, 1000, 60, 48, 48, False, True, {}, 0),                                   # Kp = 512, Bp = 128: NT GEMM 2
    (257, 1500, 260, 256, 200, False, True, {}, TN),                               # TN + duo
    (300, 2000, 260, 256, 1, True, True, {}, TN),                                  # a block of one user
    (512, 3000, 140, 129, 129, True, False, {}, TN),
    (300, 32768, 260, 256, 3, False, True, {"CDAE_FULL_ROWS_KH": "2"}, TN | ROWS),  # rows fused, tied rows with kept inputs
    (260, 40000, 260, 129, 2, False, True, {"CDAE_FULL_ROWS_KH": "1"}, TN | ROWS),  # ... GEMM 2's last split ragged (Ip 40192, 192 per split)
    (300, 65537, 4, 48, 2, True, True, {}, ROWS),                                  # NT GEMM 2 over a rows-fused item space
]


def _run(devlib, monkeypatch, case, double_rounding, **kw):
    K, I, users, B, nb, asym, scale2, env, plan = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    data = make_data(users, I, 24 if I > 64 else max(1, I // 2), np.random.default_rng(I + users))
    tier_a(data, K, B, nb, asym=asym, scale2=scale2, want_plan=plan, double_rounding=double_rounding,
           dense=0.3 if I * K < 2_000_000 else 0.1, **kw)


@pytest.mark.parametrize("case", CASES_FUSED, ids=lambda c: f"K{c[0]}-I{c[1]}-B{c[3]}-nb{c[4]}-{'asym' if c[5] else 'tied'}"
                         + ("-2stream" if c[7] else ""))
def test_exact_step_fused_decode(devlib, monkeypatch, case):
    _run(devlib, monkeypatch, case, double_rounding=False)


@pytest.mark.parametrize("case", CASES_UNFUSED, ids=lambda c: f"K{c[0]}-I{c[1]}-B{c[3]}-nb{c[4]}-{'asym' if c[5] else 'tied'}-plan{c[8]}"
                         + ("-unfused" if "CDAE_FULL_UNFUSED" in c[7] else "") + ("-kh" + c[7]["CDAE_FULL_ROWS_KH"] if "CDAE_FULL_ROWS_KH" in c[7] else ""))
def test_exact_step_unfused_and_k512(devlib, monkeypatch, case):
    _run(devlib, monkeypatch, case, double_rounding=True)


def test_exact_step_item_rows_eight_shards(built):
    """Kp = 512 on MultiCDAE(item_rows=True): each of 8 shards runs the K > 256 products over its own item rows (fs_phase1)"""
    data = make_data(260, 3000, 24, np.random.default_rng(8))
    tier_a(data, 300, 256, 40, asym=False, scale2=True, want_plan=0, shards=8, double_rounding=True)


# Item-rows shards run the launch sequences of the single handle (cdae_hip.hip: launch_full_fused, full_products_k512, full_tail) over
# their own item rows.  Each case is a tuple of CASES_FUSED / CASES_UNFUSED: make_data and tier_a seed from its values alone, so data,
# parameters and the exact-grid premise are the ones that case already runs on one handle.  (case, shards, items the largest shard must hold)
CASES_ITEM_ROWS = [
    (CASES_FUSED[5], 2, 0),          # K 65 (Kp = 128), 129 items, tied: the fused kernel on two shards
    (CASES_FUSED[7], 3, 0),          # K 256, 4097 items, asymmetric: the fused kernel on three shards
    (CASES_UNFUSED[5], 3, 0),        # K 512, 3000 items, asymmetric: the K > 256 products on three shards
    # K 300 (Kp = 512), 65537 items on two shards: one of them holds >= 32768 items, whichever way the cut falls.  Its Ip is a multiple
    # of 256, so rows_fused_path holds (Ip % FR_ITEMS == 0) and it runs gemm3_rows_fused_kernel; the other shard, below 32768 items,
    # runs GEMM 3 + full_rows_kernel.
    (CASES_UNFUSED[8], 2, 32768),
    (CASES_FUSED[9], 2, 32768),      # K 64, 65537 items: the shard of >= 32768 items runs full_rows_wave_kernel, the other full_rows_kernel
]


@pytest.mark.parametrize("case,shards,largest", CASES_ITEM_ROWS,
                         ids=[f"K{c[0]}-I{c[1]}-B{c[3]}-nb{c[4]}-{'asym' if c[5] else 'tied'}-shards{s}" for c, s, _ in CASES_ITEM_ROWS])
def test_exact_step_item_rows_shards(built, monkeypatch, case, shards, largest):
    """the shared full-output launches on MultiCDAE(item_rows=True): fused and K > 256 plans, tied and asymmetric, each of the three
    row steps.  (The shipped library: the developer switches in the tuples do not apply to a shard.)"""
    _run(None, monkeypatch, case[:7] + ({}, case[8]), double_rounding=not case[8] & FUSED, shards=shards, min_largest_shard=largest)


# ---- Tier B ------------------------------------------------------------------------------------------------------------------------
CASES_B = [
    # (loss, K, B, adagrad, extra flags, env, plan)
    (cdae_amd.CROSS_ENTROPY, 300, 256, True, dict(), {}, TN),
    (cdae_amd.SQUARE, 300, 48, False, dict(tanh=True), {}, 0),
    (cdae_amd.CROSS_ENTROPY, 40, 48, True, dict(user_factor=False), {"CDAE_FULL_UNFUSED": "1"}, 0),
    (cdae_amd.CROSS_ENTROPY, 40, 48, False, dict(linear_function=True), {}, FUSED),
    (cdae_amd.SQUARE, 512, 129, True, dict(), {}, TN),
]


@pytest.mark.parametrize("case", CASES_B, ids=lambda c: f"{'CE' if c[0] == cdae_amd.CROSS_ENTROPY else 'SQ'}-K{c[1]}-B{c[2]}-"
                         + ("ada" if c[3] else "sgd") + "".join("-" + k for k in c[4]) + ("-unfused" if c[5] else ""))
def test_realistic_block_within_derived_bound(devlib, monkeypatch, case):
    loss, K, B, ada, extra, env, plan = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ce = loss == cdae_amd.CROSS_ENTROPY
    data = synth.generate(2 * B, 1500, 2 * B * 20, seed=K + B, min_items=4)
    flags = dict(using_adagrad=ada, asymmetric=True, user_factor=True, linear=False, scaled=True, tanh=False, linear_function=False)
    flags.update(extra)
    hyper = dict(lambda_=0.01, learn_rate=0.05 if ada else 0.01, corruption_ratio=0.5, beta=1.0, num_neg=5, num_corruptions=1)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=loss, batch_users=B, full_output=True, **flags, **hyper)
    model = cdae_amd.CDAE(cfg)
    model.reset(data, seed=11)
    assert model.full_output_plan == plan
    model.train_users(SEED, 0, B, 2 * B)                   # a block of training from the counter-stream init
    I, nb = data.num_items, B
    T = targets(data, nb, I)
    o = oracle_of(model, data, dict(num_dim=K, loss_type=loss, **flags, **hyper))
    # well-fit positives: raise b' of the block's positive items until y sits where the double rounding was coarse
    Z = o.encode(SEED, 1, 1, np.arange(nb, dtype=np.uint32))
    V = model.get(cdae_amd.P_V).astype(np.float64)
    bp = model.get(cdae_amd.P_BP).astype(np.float64)
    Y0 = bf16(Z) @ bf16(V).T
    pos = T == 1
    want = 6.0 if ce else 1.0 + 2.0 ** -5                  # CE: p = sigmoid(6) = 0.9975; SQUARE: y just above 1
    for j in np.flatnonzero(pos.any(axis=0)):
        bp[j] = want - np.median(Y0[pos[:, j], j])
    model.set(cdae_amd.P_BP, bp.astype(np.float32))
    for w in (cdae_amd.P_W_AG, cdae_amd.P_V_AG, cdae_amd.P_WU_AG, cdae_amd.P_B_AG, cdae_amd.P_BP_AG):
        model.set(w, np.zeros_like(model.get(w)))
    if flags["linear_function"]:
        model.set(cdae_amd.P_UU_AG, np.zeros_like(model.get(cdae_amd.P_UU_AG)))
    o = oracle_of(model, data, dict(num_dim=K, loss_type=loss, **flags, **hyper))
    Zr, Vr = bf16(Z), bf16(model.get(cdae_amd.P_V).astype(np.float64))
    bp = model.get(cdae_amd.P_BP).astype(np.float64)
    unfused = plan != FUSED                                # the fix-up's positives: y from the fp32 z and V, not their bf16 images
    Y = Zr @ Vr.T + bp
    if unfused:
        Y = np.where(pos, Z @ model.get(cdae_amd.P_V).astype(np.float64).T + bp, Y)
    if ce:
        share = float(np.mean(1.0 / (1.0 + np.exp(-Y[pos])) > 0.99))
    else:
        share = float(np.mean(np.abs(Y[pos] - 1.0) < 0.125))
    assert share > (0.9 if ce else 0.35), share            # premise: the stated share of positives is well fit
    # where can a bf16 rounding flip?  z: the device's fp32 z is within dz of the fp64 one; y: fp32 sums of K products (+ the flipped z)
    Zf = Z
    dz = 2.0 ** -20 * np.abs(Zf) + 2.0 ** -40
    zflip = bf16(Zf - dz) != bf16(Zf + dz)
    dy = K * 2.0 ** -24 * (np.abs(Zr) @ np.abs(Vr).T) + 2.0 ** -24 * np.abs(Y) + (zflip * 2 * bf16_ulp(Zr)) @ np.abs(Vr).T
    if unfused:                                            # fp32 sum of K fp32 products, and the fp32 z itself (within 2^-20 |z|)
        dy = np.where(pos, (K * 2.0 ** -24 * np.abs(Zf) + 2.0 ** -20 * np.abs(Zf)) @ np.abs(Vr).T + 2.0 ** -24 * np.abs(Y), dy)
    gpre = 2.0 * (Y - T) if not ce else 1.0 / (1.0 + np.exp(-Y)) - T
    dg = (2.0 if not ce else 0.25) * dy + 2.0 ** -21 * np.abs(gpre) + 2.0 ** -22        # + the device's rcp / exp (a few ulp)
    gflip = bf16(gpre - dg) != bf16(gpre + dg)
    G = bf16(gpre)
    V0, bp0 = model.get(cdae_amd.P_V).astype(np.float64), bp.copy()
    model.train_users(SEED, 1, 0, nb)
    o.train_full(SEED, 1, B, 0, nb, bf16=True, unrounded_positives=unfused)
    lr, lip = hyper["learn_rate"], (1.0 / hyper["beta"] if ada else 1.0)
    g32 = nb * 2.0 ** -24
    gf, zf_ = gflip * 2 * bf16_ulp(G), zflip * 2 * bf16_ulp(Zr)
    print(f"\npositives well fit: {share:.3f}; g flips possible {gflip.mean():.2e}, z flips {zflip.mean():.2e}")
    cases = [("V", cdae_amd.P_V, V0, np.abs(G).T @ np.abs(Zr), gf.T @ np.abs(Zr) + np.abs(G).T @ zf_),
             ("b'", cdae_amd.P_BP, bp0, np.abs(G).sum(axis=0), gf.sum(axis=0))]
    for name, which, p0, mag, flips in cases:
        ref = o.get(which).reshape(p0.shape)
        got = model.get(which).astype(np.float64).reshape(p0.shape)
        step_round = (2.0 ** -22 if ada else 2.0 ** -23) * np.abs(ref) + 2.0 ** -20 * np.abs(ref - p0)
        fp32_term = lr * lip * g32 * mag + step_round
        bound = fp32_term + lr * lip * flips
        diff = np.abs(got - ref)
        beyond = float(np.mean(diff > fp32_term))
        print(f"\n{name}: max |diff| {diff.max():.3e}, max diff/bound {np.max(diff / bound):.3f}, beyond fp32 term {beyond:.4f}")
        assert np.all(diff <= bound), (name, int((diff > bound).sum()), float(np.max(diff / bound)))
        assert beyond < 0.02, (name, beyond)
