"""-m gpu: every loss and activation path of the device at SATURATED magnitudes, against tests/golden/saturation_kat.npz (numpy
closed forms of the reference's branches: CE at a score of +-18, sigmoid at a pre-activation of +-18, tanh at +-9, LOG at +-18,
HINGE at z = 1) and against the oracle from identical fp32 parameters.

The device does not copy the reference's branches everywhere: its CE gradient is branch-free (cdae_kernels.hpp loss_grad; the same
expression is written out again in the row decode's fast_group_spec chain, the full-output GEMM epilogues, gemm1_loss_duo_kernel,
the fused full-output kernel and mf_loss_grad), on the argument that fp32 reaches the same limits, __expf overflowing to +inf and
rcp(inf) = 0 past +-88.  The rest of the suite starts from the counter-stream initialisation (scale ~1e-2) and never leaves the
middle of these functions; every test here asserts its own premise — the launch it means to reach, and the share of the actual
pre-activations or scores beyond each threshold — so that it cannot pass without touching the region.

Comparisons are element by element, |gpu - ref| <= atol + rtol |ref| (a range that includes +-100 would hide the small entries),
and every parameter is finite after every step.

Known-answer tolerance (tests a-c): the grid points are fp32 values, so y and b' are exact and only the transcendental chain rounds.
__expf is exp2(x log2 e): the rounding of x log2 e (|x| <= 18.01 where the result is not saturated) costs at most
18.01 * 1.4427 * 2^-24 * ln 2 = 1.1e-6 relative, v_exp / v_rcp add 1 ulp each, so sigmoid and tanh in (0, 1) carry < 1.3e-6
relative error: rtol 4e-6.  Near 1 the fp32 form rounds 1 - tiny to 1 (the reference's fp64 keeps 1 - 1.5e-8 at x = 18), and
1 - t or 1 - r cancels: an absolute 2^-24 from that rounding plus 2^-24 from a 1-ulp rcp of a value near 1 — atol 2^-23.  The same
bound holds for the gradient rcp(1 + e^-y) - t (one more exact subtraction) and for -V / lr, since a power-of-two learn rate makes
V = -lr g exact.
"""
import os

import numpy as np
import pytest

import cdae_amd
from cdae_amd import binding as PLAN
from cdae_amd import synth
from oracle import binding as ob
from helpers import PARAMS, make_pair, record_measured, sync_oracle_from_gpu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = np.load(os.path.join(HERE, "golden", "saturation_kat.npz"))
GRID = KAT["grid"]
ATOL, RTOL = 2.0 ** -23, 4e-6
LR = 2.0 ** -3                      # power of two: V = -lr * g and b' - lr * g round exactly
FLOOR = 1e-2                        # trajectory comparisons: |gpu - ref| <= bound * (FLOOR + |ref|)


def assert_close(got, ref, what, atol=ATOL, rtol=RTOL):
    got = np.asarray(got, dtype=np.float64).ravel()
    ref = np.asarray(ref, dtype=np.float64).ravel()
    assert np.isfinite(got).all(), (what, "non-finite", np.flatnonzero(~np.isfinite(got))[:8])
    bad = np.abs(got - ref) > atol + rtol * np.abs(ref)
    if bad.any():
        i = np.flatnonzero(bad)
        raise AssertionError(f"{what}: {i.size} entries off, e.g. at {i[:6]}: got {got[i[:6]]} want {ref[i[:6]]}")


def one_user(n_pos, n_items):
    ptr = np.array([0, n_pos], dtype=np.int64)
    col = np.arange(n_pos, dtype=np.uint32)
    return synth.Interactions(1, n_items, ptr, col, np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.uint32))


def set_both(model, o, which, arr):
    model.set(which, np.asarray(arr, dtype=np.float32))
    o.set(which, model.get(which).astype(np.float64))


def all_finite(model, o):
    for w in PARAMS:
        if o.get(w).size:
            assert np.isfinite(model.get(w)).all(), w


def share_beyond(x, t):
    return float(np.mean(np.abs(np.asarray(x)) > t))


# ---- (a) activations -------------------------------------------------------------------------------------------------------------
ACTS = {"sigmoid": dict(), "tanh": dict(tanh=True), "linear": dict(linear=True)}


def _act_ref(act, b):
    return b.astype(np.float64) if act == "linear" else np.resize(KAT[act], b.size)


@pytest.mark.parametrize("act", list(ACTS))
def test_hidden_values_of_the_grid(built, act):
    """get_hidden_values (mode 0; encode_partial + encode_finish_kernel) of a user whose W and Wu are zero and whose b is the grid
    (128 units: the 53 grid points, then again)."""
    K = 128
    model, o = make_pair(one_user(3, 4), K=K, B=1, **ACTS[act])
    b = np.resize(GRID, K).astype(np.float32)
    set_both(model, o, cdae_amd.P_W, np.zeros((4, K)))
    set_both(model, o, cdae_amd.P_WU, np.zeros((1, K)))
    set_both(model, o, cdae_amd.P_B, b)
    assert share_beyond(b, 18) > 0.4 and share_beyond(b, 88.5) > 0.1 and (b < -44.5).any()
    z = model.get_hidden_values([0], mode=0)[0]
    assert_close(z, _act_ref(act, b), f"hidden {act}")
    assert_close(z, o.encode(0, 0, 0, [0])[0], f"hidden {act} vs oracle")


def _training_encode_observed(act):
    """The TRAINING encode, observed through the decoder: one user, no negatives, CE, plain SGD with a power-of-two learn rate, lambda 0,
    V = 0 and every b' = -1000, so that every positive's score is -1000 and its gradient rcp(1 + e^1000) - 1 = -1 exactly; the V row
    of each positive is then lr * z after the step, bit for bit."""
    K, P = 128, 16
    model, o = make_pair(one_user(P, P + 4), K=K, B=1, asymmetric=True, using_adagrad=False, learn_rate=LR, lambda_=0.0, num_neg=0,
                         **ACTS[act])
    b = np.resize(GRID, K).astype(np.float32)
    model.set(cdae_amd.P_W, np.zeros((P + 4, K)))
    model.set(cdae_amd.P_WU, np.zeros((1, K)))
    model.set(cdae_amd.P_B, b)
    model.set(cdae_amd.P_V, np.zeros((P + 4, K)))
    model.set(cdae_amd.P_BP, np.full(P + 4, -1000.0))
    st = model.train_one_iteration(seed=3, epoch=0)
    assert st.users == 1
    V = model.get(cdae_amd.P_V).astype(np.float64)
    assert_close(V[:P] / LR, np.broadcast_to(_act_ref(act, b), (P, K)), f"training encode {act}")
    assert not V[P:].any()
    assert np.isfinite(model.get(cdae_amd.P_B)).all() and np.isfinite(model.get(cdae_amd.P_W)).all()


@pytest.mark.parametrize("act", list(ACTS))
def test_training_encode_of_the_grid(built, act):
    """the shipped one-launch encode (encode_users_kernel: a batch of one user is far below ENCODE_USERS_MAX)"""
    _training_encode_observed(act)


@pytest.mark.parametrize("act", list(ACTS))
def test_training_encode_of_the_grid_in_two_launches(built, monkeypatch, devlib, act):
    """CDAE_ENCODE_TWO_LAUNCHES (developer build): the training encode as encode_partial_kernel + encode_finish_kernel"""
    monkeypatch.setenv("CDAE_ENCODE_TWO_LAUNCHES", "1")
    assert cdae_amd.binding._default_path == cdae_amd.DEV_LIB_PATH
    _training_encode_observed(act)


# ---- (b) the loss gradient of every grid point through one explicit step -----------------------------------------------------------
STEP_VARIANTS = {"asym_sgd": dict(asymmetric=True, using_adagrad=False), "asym_ada": dict(asymmetric=True, using_adagrad=True),
                 "tied_sgd": dict(asymmetric=False, using_adagrad=False), "tied_ada": dict(asymmetric=False, using_adagrad=True)}


@pytest.mark.parametrize("K", [40, 300])
@pytest.mark.parametrize("loss", [cdae_amd.CROSS_ENTROPY, cdae_amd.SQUARE], ids=["ce", "sq"])
@pytest.mark.parametrize("variant", list(STEP_VARIANTS))
def test_loss_gradient_of_the_grid(built, K, loss, variant):
    """One train_one_user_corruption: the user's 53 positives carry the grid as truth-1 scores, 53 explicit negatives as truth-0
    scores.  W = Wu = 0 and b = +1000 saturate z to exactly 1, the decoder is 0 and b' is the grid, so y = b' exactly.  With plain
    SGD (lambda 0, lr = 1/8) the decoder row of item i is -lr g_i after the step: compared with the fixture's gradient columns
    (tolerance in the module docstring; derived, not measured).  Every variant — AdaGrad, tied weights — is also compared with
    Oracle.step_user from the same fp32 parameters.  K = 40 takes the hybrid row / gather decode, K = 300 decode_rows_kernel
    (launch_decode: K > 256).  One example per row: the rows' single-example step, not the chained fast_group_spec of rows with many
    examples, which test_sampled_training_from_saturated_parameters reaches."""
    flags = STEP_VARIANTS[variant]
    n = GRID.size
    I = 2 * n
    d = synth.Interactions(1, I, np.array([0, n], dtype=np.int64), np.arange(n, dtype=np.uint32), np.zeros(2, dtype=np.int64),
                           np.zeros(0, dtype=np.uint32))
    model, o = make_pair(d, K=K, B=1, loss=loss, learn_rate=LR, lambda_=0.0, **flags)
    if K > 256:
        assert model.decode_plan["hot_rows"] == 0               # the row kernel: no hybrid split is reported
    dec = cdae_amd.P_V if flags["asymmetric"] else cdae_amd.P_W
    model.set(cdae_amd.P_W, np.zeros((I, K)))
    if flags["asymmetric"]:
        model.set(cdae_amd.P_V, np.zeros((I, K)))
    model.set(cdae_amd.P_WU, np.zeros((1, K)))
    model.set(cdae_amd.P_B, np.full(K, 1000.0))
    bp = np.concatenate([GRID, GRID]).astype(np.float32)
    model.set(cdae_amd.P_BP, bp)
    sync_oracle_from_gpu(model, o)
    assert share_beyond(bp, 18) > 0.4 and share_beyond(bp, 88.5) > 0.14      # 22 and 8 of the 53 grid points
    inputs = np.arange(0, n, 2, dtype=np.uint32)
    negs = np.arange(n, I, dtype=np.uint32)
    model.train_one_user_corruption(0, inputs, negs)
    _, y, g, _ = o.step_user(0, inputs, negs)
    np.testing.assert_array_equal(y, bp.astype(np.float64))     # the oracle's premise: y is the grid
    all_finite(model, o)
    key = "ce" if loss == cdae_amd.CROSS_ENTROPY else "sq"
    want = np.concatenate([KAT[f"{key}_grad_t1"], KAT[f"{key}_grad_t0"]])
    assert_close(g, want, "oracle gradient", atol=1e-12, rtol=1e-12)
    D = model.get(dec).astype(np.float64)
    if not flags["using_adagrad"]:
        assert_close(-D / LR, np.broadcast_to(want[:, None], (I, K)), f"-{'V' if flags['asymmetric'] else 'W'}/lr")
    for w in PARAMS:
        if o.get(w).size:
            assert_close(model.get(w), o.get(w), f"parameter {w} vs oracle")
    record_measured(f"saturation_step_{variant}_{key}_K{K}", err=np.abs(-D[:, 0] / LR - want).max())


# ---- (c) data_loss ---------------------------------------------------------------------------------------------------------------
def test_data_loss_of_the_grid(built):
    """z saturated to 1, V = 0, every b' = +1000: each positive contributes (1 - 1) y + e^-1000 = 0 exactly, on the device and in the
    reference.  Setting one positive's b' to a grid point at a time makes data_loss evaluate(grid point, 1) alone."""
    n, K = 8, 32
    model, o = make_pair(one_user(n, n + 8), K=K, B=1, asymmetric=True)
    model.set(cdae_amd.P_W, np.zeros((n + 8, K)))
    model.set(cdae_amd.P_V, np.zeros((n + 8, K)))
    model.set(cdae_amd.P_WU, np.zeros((1, K)))
    model.set(cdae_amd.P_B, np.full(K, 1000.0))
    bp = np.full(n + 8, 1000.0, dtype=np.float32)
    model.set(cdae_amd.P_BP, bp)
    sync_oracle_from_gpu(model, o)
    assert model.data_loss(5, 0) == 0.0 and o.data_loss(5, 0) == 0.0
    got, ref = [], []
    for x in GRID:
        p = bp.copy()
        p[3] = x
        model.set(cdae_amd.P_BP, p)
        o.set(cdae_amd.P_BP, p.astype(np.float64))
        got.append(model.data_loss(5, 0))
        ref.append(o.data_loss(5, 0))
    assert_close(got, KAT["ce_eval_t1"], "data_loss")
    assert_close(ref, KAT["ce_eval_t1"], "oracle data_loss", atol=1e-12, rtol=1e-12)


# ---- (d) sampled training from saturated parameters ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(built):
    return synth.generate_shape("tiny", seed=5)


@pytest.fixture(scope="module")
def small(built):
    return synth.generate(1200, 500, 60_000, seed=9)


def saturate(model, o, data, *, seed, b_half=40.0, bp_half=120.0, v_sd=30.0, full=False):
    """Identical fp32 parameters on both sides: hidden biases uniform in +-b_half, decoder entries N(0, (v_sd / sqrt K)^2), b' uniform
    in +-bp_half.  Returns the pre-activations and scores of the first step as it will actually see them (the oracle's draws of the
    kept inputs and of the negatives; every unrated item in full-output mode)."""
    cfg = model.cfg
    K, U, I = cfg.num_dim, data.num_users, data.num_items
    rng = np.random.default_rng(seed)
    set_both(model, o, cdae_amd.P_B, rng.uniform(-b_half, b_half, K))
    dec = cdae_amd.P_V if cfg.asymmetric else cdae_amd.P_W
    set_both(model, o, dec, rng.normal(0.0, v_sd / np.sqrt(K), (I, K)))
    set_both(model, o, cdae_amd.P_BP, rng.uniform(-bp_half, bp_half, I))
    W = model.get(cdae_amd.P_W).astype(np.float64)
    D = model.get(dec).astype(np.float64)
    Wu = model.get(cdae_amd.P_WU).astype(np.float64)
    b, bp = model.get(cdae_amd.P_B).astype(np.float64), model.get(cdae_amd.P_BP).astype(np.float64)
    scale = 1.0 / (1.0 - cfg.corruption_ratio) if cfg.scaled else 1.0
    H, Y = [], []
    for u in range(U):
        row = data.train_col[data.train_ptr[u]:data.train_ptr[u + 1]]
        kept = row if full else o.draw_inputs(4, 0, u)
        h = scale * W[kept].sum(axis=0) + Wu[u] + b
        z = h if cfg.linear else (np.tanh(h) if cfg.tanh else 1.0 / (1.0 + np.exp(-np.clip(h, -50, 50))))
        items = np.arange(I) if full else np.concatenate([row, o.draw_negatives(4, 0, u)])
        H.append(h)
        Y.append(D[items] @ z + bp[items])
    return np.concatenate(H), np.concatenate(Y)


def rel_errs(model, o):
    """which -> max |gpu - oracle| / (FLOOR + |oracle|), every parameter finite"""
    out = {}
    for w in PARAMS:
        ref = o.get(w)
        if ref.size:
            got = model.get(w).astype(np.float64).ravel()
            assert np.isfinite(got).all(), w
            out[w] = float((np.abs(got - ref) / (FLOOR + np.abs(ref))).max())
    return out


# fp32 against fp64, two epochs: the bound is <= 1.3 x the largest element-wise error measured over the parameters (recorded as
# saturation_sampled_<name>: 2.2e-4, 2.2e-4, 2.1e-4, 3.8e-3, 5.5e-3, 1.3e-4, each on a user-side accumulator or decoder entry —
# the hidden gradient of the unsaturated units is a sum with cancellation, and tanh / linear keep more units unsaturated)
SAMPLED = {
    # name: (make_pair keywords, K, B, launch, bound)
    "ce_ada_fused": (dict(), 40, 300, "fused", 2.9e-4),
    "ce_ada_unfused": (dict(), 40, 300, "unfused", 2.9e-4),
    "sq_sgd": (dict(loss=cdae_amd.SQUARE, using_adagrad=False, learn_rate=2.0 ** -12, asymmetric=True), 40, 64, "hybrid", 2.6e-4),
    "tanh": (dict(tanh=True), 40, 1, "hybrid", 4.9e-3),
    "linear": (dict(linear=True, learn_rate=0.01), 40, 64, "hybrid", 7.1e-3),
    "ce_ada_rows_K300": (dict(asymmetric=True), 300, 64, "rows", 1.7e-4),
}
LOSS_BOUND = 1.1e-5          # relative, per epoch: <= 1.3 x the 9.1e-6 measured (SQUARE + SGD, epoch 1; the CE cases <= 2.6e-7)


@pytest.mark.parametrize("name", list(SAMPLED))
def test_sampled_training_from_saturated_parameters(tiny, name):
    """Two epochs of the sampled schedule from saturated parameters against the oracle's literal (B = 1) or block schedule:
    parameters element by element and the per-epoch data_loss."""
    kw, K, B, launch, bound = SAMPLED[name]
    model, o = make_pair(tiny, K=K, B=B, **kw)
    plan = model.decode_plan
    if launch == "unfused":
        model.set_decode_fused(False)
    if launch in ("fused", "unfused"):
        assert plan["fused"] and plan["late_rows"] > 0, plan
        assert model.decode_plan["fused"] == (launch == "fused")
    elif launch == "rows":
        assert K > 256 and plan["hot_rows"] == 0, plan
    else:
        assert K <= 256 and not plan["fused"], plan
    b_half = 20.0 if kw.get("tanh") else 40.0
    H, Y = saturate(model, o, tiny, seed=17, b_half=b_half)
    assert share_beyond(H, 9.0 if kw.get("tanh") else 18.0) > 0.4, share_beyond(H, 18.0)
    assert share_beyond(Y, 18.0) > 0.6 and share_beyond(Y, 88.5) > 0.1, (share_beyond(Y, 18.0), share_beyond(Y, 88.5))
    for ep in range(2):
        model.train_one_iteration(seed=4, epoch=ep)
        if B == 1:
            o.train_literal(4, ep)
        else:
            o.train_batched(4, ep, B)
        lg, lo = model.data_loss(6, ep), o.data_loss(6, ep)
        record_measured(f"saturation_sampled_{name}_loss", ep=ep, err=abs(lg - lo) / abs(lo))
        assert np.isfinite(lg) and abs(lg - lo) <= LOSS_BOUND * abs(lo), (ep, lg, lo)
    errs = rel_errs(model, o)
    record_measured(f"saturation_sampled_{name}", **{f"p{w}": e for w, e in errs.items()})
    worst = max(errs, key=errs.get)
    assert errs[worst] < bound, (worst, errs)


def test_fused_and_unfused_decode_agree_bit_for_bit_when_saturated(tiny):
    """decode_gather_kernel against the separate decode + gather launches (set_decode_fused(False)) from saturated parameters:
    every parameter bit-identical after two epochs, as at ordinary magnitudes
    (test_gpu_parity.py::test_fused_decode_gather_launch_changes_no_bit)."""
    outs = []
    for allow in (True, False):
        model, o = make_pair(tiny, K=40, B=300)
        assert model.decode_plan["fused"] and model.decode_plan["late_rows"] > 0, model.decode_plan
        model.set_decode_fused(allow)
        saturate(model, o, tiny, seed=17)
        for ep in range(2):
            model.train_one_iteration(seed=4, epoch=ep)
        outs.append({w: model.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)})
        model.close()
    for w in outs[0]:
        assert np.isfinite(outs[0][w]).all(), w
        assert np.array_equal(outs[0][w], outs[1][w]), (w, np.abs(outs[0][w] - outs[1][w]).max())


# ---- (e) full-output decode from saturated parameters ----------------------------------------------------------------------------
# bf16 operands: every bound is <= 1.3 x the element-wise error measured for that parameter (recorded as saturation_full_<name>).
# The score side (b', b'_ag: P_BP, P_BP_AG) stays within 0.3 - 6 %; the hidden side does not: z and D are rounded to bf16 (2^-9) before
# y = D z, which moves the unsaturated scores' g by up to ~0.03, and the hidden gradient sum_j g_j D_j cancels — the user-side AdaGrad
# accumulators (P_WU_AG) of small entries differ by up to 100 % of (1e-2 + |ref|).
FULL = {
    # name: (K, B, data set, developer switch, plan bits that must be set / clear, per-parameter bounds)
    "fused_B48": (24, 48, "tiny", None, (PLAN.PLAN_FUSED_DECODE, 0),
                  {0: 0.052, 1: 0.034, 4: 0.43, 5: 1.3, 6: 4e-4, 7: 7.3e-3, 8: 4.1e-3, 9: 0.014}),
    "fused_B300": (24, 300, "tiny", None, (PLAN.PLAN_FUSED_DECODE, 0),
                   {0: 0.23, 1: 0.15, 4: 0.10, 5: 0.74, 6: 5e-4, 7: 7.3e-3, 8: 0.058, 9: 0.052}),
    "three_gemm_B48": (24, 48, "tiny", "CDAE_FULL_UNFUSED", (0, PLAN.PLAN_FUSED_DECODE),
                       {0: 0.049, 1: 0.035, 4: 0.43, 5: 1.3, 6: 3.7e-4, 7: 7.6e-3, 8: 3e-3, 9: 0.014}),
    "duo_K300_B256": (300, 256, "small", None, (PLAN.PLAN_GEMM2_TN, PLAN.PLAN_FUSED_DECODE),
                      {0: 0.26, 1: 0.22, 4: 0.30, 5: 1.1, 6: 0.099, 7: 7.4e-3, 8: 7.9e-3, 9: 0.033}),
}


def _full_run(data, K, B):
    model, o = make_pair(data, K=K, B=B, full_output=True)
    _, Y = saturate(model, o, data, seed=23, full=True)
    return model, o, Y


@pytest.mark.parametrize("name", list(FULL))
def test_full_output_from_saturated_parameters(request, monkeypatch, name):
    """Full-output decode (bf16 MFMA operands, fp32 epilogues) from saturated parameters against Oracle.train_full, two epochs: the
    fused kernel (K <= 256), the three tiled GEMMs (CDAE_FULL_UNFUSED, developer build) and the K > 256 path whose GEMM 1 is
    gemm1_loss_duo_kernel and GEMM 2 gemm_tn_bf16_kernel (whole 256-user blocks; the fused rows step needs >= 32768 items and is
    left to tests/test_gpu_accuracy.py)."""
    K, B, dname, switch, (must, must_not), bounds = FULL[name]
    data = request.getfixturevalue(dname)
    if switch:
        request.getfixturevalue("devlib")
        monkeypatch.setenv(switch, "1")
    model, o, Y = _full_run(data, K, B)
    plan = model.full_output_plan
    assert (plan & must) == must and not (plan & must_not), plan
    assert share_beyond(Y, 18.0) > 0.6 and share_beyond(Y, 88.5) > 0.1, (share_beyond(Y, 18.0), share_beyond(Y, 88.5))
    for ep in range(2):
        model.train_one_iteration(seed=4, epoch=ep)
        o.train_full(4, ep, B)
    errs = rel_errs(model, o)
    record_measured(f"saturation_full_{name}", **{f"p{w}": e for w, e in errs.items()})
    assert set(errs) == set(bounds)
    for w in errs:
        assert errs[w] < bounds[w], (w, errs[w], bounds[w])


def test_duo_and_tiled_gemm1_agree_bit_for_bit_when_saturated(small, monkeypatch, devlib):
    """gemm1_loss_duo_kernel against the tiled GEMM 1 (CDAE_GEMM1_TILED) at K = 300, B = 256 from saturated parameters: the same loss
    epilogue on the same products — every parameter bit-identical after an epoch."""
    outs = []
    for tiled in (False, True):
        if tiled:
            monkeypatch.setenv("CDAE_GEMM1_TILED", "1")
        model, _, Y = _full_run(small, 300, 256)
        assert model.full_output_plan & PLAN.PLAN_GEMM2_TN
        assert share_beyond(Y, 88.5) > 0.1
        model.train_one_iteration(seed=4, epoch=0)
        outs.append({w: model.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)})
        model.close()
    for w in outs[0]:
        assert np.isfinite(outs[0][w]).all(), w
        assert np.array_equal(outs[0][w], outs[1][w]), (w, np.abs(outs[0][w] - outs[1][w]).max())


# ---- (f) IMF / BPR ---------------------------------------------------------------------------------------------------------------
def _mf_data():
    """53 users: user u's first (smallest) item is item u, then four of the items 53 .. 99"""
    rng = np.random.default_rng(3)
    n = GRID.size
    rows = [np.r_[u, np.sort(rng.choice(np.arange(n, n + 47), 4, replace=False))].astype(np.uint32) for u in range(n)]
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    return synth.Interactions(n, n + 47, ptr, np.concatenate(rows), np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.uint32))


MF_CASES = [(False, cdae_amd.SQUARE), (False, cdae_amd.CROSS_ENTROPY), (False, cdae_amd.LOG), (False, cdae_amd.HINGE),
            (True, cdae_amd.LOG), (True, cdae_amd.HINGE)]
MF_BOUND = 1e-3


@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("pairwise,loss", MF_CASES, ids=lambda v: str(v))
def test_mf_from_grid_scores(built, pairwise, loss, B):
    """Every user vector is e_0 and item i < 53 carries grid[i] in coordinate 0 (biases 0), so each user's first instance scores its
    positive item u at exactly grid[u] — HINGE at exactly z = 1 included.  Two epochs of the sequential schedule (B = 1) against
    MfOracle.train_literal, of the block schedule (B = 64: one block) against train_batched."""
    from test_gpu_mf import PAIRS, by_position, make
    d = _mf_data()
    K = 16
    m, o = make(d, K=K, B=B, loss=loss, pairwise=pairwise)
    np.testing.assert_array_equal(m.user_order(), np.arange(d.num_users))
    rng = np.random.default_rng(5)
    uv = np.zeros((d.num_users, K)); uv[:, 0] = 1.0
    iv = rng.normal(0.0, 0.1, (d.num_items, K)); iv[:, 0] = 0.0; iv[:GRID.size, 0] = GRID
    for po, pg, val in ((ob.MF_UV, cdae_amd.P_WU, uv), (ob.MF_IV, cdae_amd.P_W, iv), (ob.MF_UB, cdae_amd.P_UB, np.zeros(d.num_users)),
                        (ob.MF_IB, cdae_amd.P_BP, np.zeros(d.num_items))):
        m.set(pg, val)
        o.set(po, by_position(m, pg))
    first = np.array([o.predict(u, int(d.train_col[d.train_ptr[u]])) for u in range(d.num_users)])
    np.testing.assert_array_equal(first, GRID)
    assert share_beyond(first, 18) > 0.4 and share_beyond(first, 88.5) > 0.14 and (first == 1.0).any()
    for ep in range(2):
        m.train_one_iteration(seed=7, epoch=ep)
        if B == 1:
            o.train_literal(7, ep)
        else:
            o.train_batched(7, ep, B)
    errs = {}
    for po, pg in PAIRS:
        ref = o.get(po)
        got = by_position(m, pg).ravel()
        assert np.isfinite(got).all(), pg
        errs[pg] = float((np.abs(got - ref) / (FLOOR + np.abs(ref))).max())
    record_measured(f"saturation_mf_pair{int(pairwise)}_loss{loss}_B{B}", **{f"p{w}": e for w, e in errs.items()})
    worst = max(errs, key=errs.get)
    assert errs[worst] < MF_BOUND, (worst, errs)


# ---- (g) fold-in of user nodes (fold_in_rows_kernel: its own uses of activate, act_deriv and loss_grad) ----------------------------
FOLD_K, FOLD_LAMBDA = 128, 2.0 ** -6
FOLD_LENS = (1, 3, 42, 43, 64, 129, 200)            # both roles at num_neg = 5 (a wavefront up to 42 items, a workgroup beyond)
FOLD_UIDS = (1, cdae_amd.NO_USER, 1, 0, 1, cdae_amd.NO_USER, 1)


FOLD_NAMES = ("wu", "wu_ag", "uu", "uu_ag")


def _fold_errs(got, want):
    return {n: float((np.abs(g - w) / (FLOOR + np.abs(w))).max()) for n, g, w in zip(FOLD_NAMES, got, want)}


def _fold_model(I, tables, Wu, **kw):
    """a handle over len(Wu) users that holds the given tables (no training), CROSS_ENTROPY, lr = 1/8, lambda = 2^-6"""
    from test_gpu_rows import csr
    U = Wu.shape[0]
    model = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=FOLD_K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=U, learn_rate=LR,
                                              lambda_=FOLD_LAMBDA, **kw))
    model.set_interactions(U, I, *csr([np.arange(3 * u, 3 * u + 3, dtype=np.uint32) for u in range(U)]))
    model.init_params(0)
    for which, arr in tables.items():
        model.set(which, arr)
    model.set(cdae_amd.P_WU, Wu)
    return model


def _fold_rows(I, seed):
    from test_gpu_rows import csr
    rng = np.random.default_rng(seed)
    return csr([np.sort(rng.choice(I, n, replace=False)).astype(np.uint32) for n in FOLD_LENS]) + (np.array(FOLD_UIDS, np.uint32),)


def _fold_yardstick(model, ptr, col, uids, n_epochs, frozen_delta=False):
    """tests/fold_in_ref.py from the handle's fp32 parameters -> (want, z of every row's first step)"""
    import fold_in_ref as ref
    from test_gpu_fold_in import SEED, oracle_config, start_nodes
    import oracle as orc
    cfg = model.cfg
    o = orc.Oracle(oracle_config(cfg), ptr.size - 1, model.num_items, ptr, col)
    P = dict(W=model.get(cdae_amd.P_W).astype(np.float64), b=model.get(cdae_amd.P_B).astype(np.float64),
             bp=model.get(cdae_amd.P_BP).astype(np.float64), V=model.get(cdae_amd.P_V).astype(np.float64) if cfg.asymmetric else None)
    start = [a.astype(np.float64) for a in start_nodes(model, uids)]
    z0 = np.stack([ref.step(o.cfg, P, col[ptr[r]:ptr[r + 1]], o.draw_inputs(SEED, 0, r, 0), o.draw_negatives(SEED, 0, r, 0),
                            tuple(a[r] for a in start))[1] for r in range(ptr.size - 1)])
    return ref.fold_in(o, P, start, SEED, 0, n_epochs), start, z0, o, P


@pytest.mark.parametrize("adagrad", [True, False], ids=["ada", "sgd"])
@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_fold_in_from_saturated_hidden_units(built, act, adagrad):
    """b carries the grid in units 0 .. 63 and user 1's Wu row carries it in units 64 .. 127; W = 0 (asymmetric: the decoder V is
    not), so S = 0 and h = b + wu is the grid point itself, exactly, on the device and in the yardstick.  Two epochs against the fp64
    yardstick under the bound test_sampled_training_from_saturated_parameters holds this activation and optimiser to.  Then ONE step:
    where z is exactly 0, 1 or -1 (|h| > 18, or > 9 for tanh: act'(z) = 0, delta = 0) the node moves by the lambda wu term alone —
    an equality: a unit whose wu is 0 keeps wu = 0 and wu_ag = 1e-4 bit for bit, and under plain SGD with power-of-two lr and lambda
    every saturated unit is wu - lr lambda wu, which fp64 forms exactly and fmaf rounds once."""
    from test_gpu_fold_in import SEED, fold_all
    I = 977
    rng = np.random.default_rng(41)
    half = np.resize(GRID, 64)
    b = np.r_[half, np.zeros(64)]
    Wu = np.stack([np.zeros(FOLD_K), np.r_[np.zeros(64), half], rng.normal(0, 0.1, FOLD_K)])
    tables = {cdae_amd.P_W: np.zeros((I, FOLD_K)), cdae_amd.P_V: rng.normal(0, 0.05, (I, FOLD_K)), cdae_amd.P_B: b,
              cdae_amd.P_BP: rng.uniform(-1, 1, I)}
    model = _fold_model(I, tables, Wu, asymmetric=True, using_adagrad=adagrad, tanh=(act == "tanh"))
    ptr, col, uids = _fold_rows(I, 43)
    thr = 9.0 if act == "tanh" else 18.0
    bound = SAMPLED["tanh"][4] if act == "tanh" else SAMPLED["ce_ada_fused" if adagrad else "sq_sgd"][4]
    want, start, z0, o, P = _fold_yardstick(model, ptr, col, uids, 2)
    h0 = b[None, :] + start[0]
    sat = np.abs(h0) > thr
    np.testing.assert_array_equal(np.isin(z0, (0.0, 1.0, -1.0)) & (h0 != 0), sat)          # the premise: exactly saturated there
    assert share_beyond(h0[uids == 1], thr) > 0.4 and share_beyond(h0, 88.5) > 0.05 and (np.abs(h0) == 1000).any()
    got = fold_all(model, ptr, col, uids, n_epochs=2)
    record_measured(f"saturation_fold_in_hidden_{act}_{'ada' if adagrad else 'sgd'}", **_fold_errs(got, want))
    for name, g, w in zip(FOLD_NAMES, got, want):
        assert_close(g, w, f"fold-in {act} {name}", atol=bound * FLOOR, rtol=bound)
    assert np.abs(want[0] - start[0])[~sat].max() > 1e-3             # (the unsaturated units took real steps)
    # one step: delta = 0 where z is saturated
    one = fold_all(model, ptr, col, uids, n_epochs=1)
    still = sat & (start[0] == 0)
    assert still.any() and (one[0][still] == 0).all() and (one[1][still] == np.float32(1e-4)).all()
    if not adagrad:
        lam_only = (start[0] - LR * (FOLD_LAMBDA * start[0])).astype(np.float32)
        assert (start[0][sat] != 0).any()
        np.testing.assert_array_equal(one[0][sat], lam_only[sat])
    model.close()


def test_fold_in_from_saturated_scores(built):
    """b' carries the grid (977 items: the 53 points again and again) and W ~ N(0, 0.02^2), so every example's y = W[j].z + b'[j] sits
    within a fraction of its grid point: the kernel's branch-free CROSS_ENTROPY gradient beyond |y| > 18 and past the fp32 overflow of
    e^-y, against the yardstick's clamped branches.  Two epochs of AdaGrad, both roles, under the sigmoid / AdaGrad bound of
    test_sampled_training_from_saturated_parameters."""
    from test_gpu_fold_in import SEED, fold_all
    I = 977
    rng = np.random.default_rng(47)
    tables = {cdae_amd.P_W: rng.normal(0, 0.02, (I, FOLD_K)), cdae_amd.P_B: rng.normal(0, 0.3, FOLD_K), cdae_amd.P_BP: np.resize(GRID, I)}
    Wu = rng.normal(0, 0.3, (3, FOLD_K))
    model = _fold_model(I, tables, Wu)
    ptr, col, uids = _fold_rows(I, 49)
    bound = SAMPLED["ce_ada_fused"][4]
    want, start, z0, o, P = _fold_yardstick(model, ptr, col, uids, 2)
    examples = [np.r_[col[ptr[r]:ptr[r + 1]], o.draw_negatives(SEED, 0, r, 0)] for r in range(ptr.size - 1)]
    y0 = np.concatenate([P["W"][E] @ z0[r] + P["bp"][E] for r, E in enumerate(examples)])        # the scores of every row's first step
    assert share_beyond(y0, 18.0) > 0.4 and share_beyond(y0, 88.5) > 0.1 and share_beyond(y0, 500) > 0.02
    got = fold_all(model, ptr, col, uids, n_epochs=2)
    record_measured("saturation_fold_in_scores", **_fold_errs(got, want))
    for name, g, w in zip(FOLD_NAMES, got, want):
        assert_close(g, w, f"fold-in scores {name}", atol=bound * FLOOR, rtol=bound)
    assert np.abs(want[0] - start[0]).max() > 1e-3
    model.close()
