"""-m gpu: the IMF / BPR kernels (cdae_mf_kernels.hpp) against oracle/mf_oracle.cpp at every K tier and beyond the default
hyper-parameters — what tests/test_gpu_mf.py leaves out.

compute_batch_mf instantiates mf_user_kernel<NI, PAIR, IN_PLACE> and mf_item_kernel<NI> for NI = 1, 2, 4, 8 (K <= 64, 65 .. 128,
129 .. 256, 257 .. 512: one wavefront holds a row, NI floats per lane).  test_gpu_mf.py runs the in-place loop at K = 24 only (NI = 1)
and the block schedule with the default hyper-parameters only.  Here:

  * the sequential schedule (batch_users = 1: IN_PLACE, PF = 4 register sets of rows, accumulators and biases, BPR both items, twice)
    at both edges of every tier, on D40 — a data set whose users repeat item rows at every distance around the 8-instance conflict
    window and across the 64-instance chunk boundary (tests/mf_conflict_ref.py; the premise is asserted for the seed and the epochs
    trained) — and on "tiny", whose 300 users are two launch windows of the sequential default;
  * the block schedule at B = 33 (a partial last block, activity-grouped order) with plain SGD, without bias terms, with num_neg = 1
    (BPR never carries its positive) and num_neg = 12 (BPR's private copy of a positive lives across more pairs than one prefetch
    group and across chunk boundaries), at K = 24, 200 and 300 (NI = 1, 4, 8);
  * D40 as ONE block of 8 users: every item row takes hundreds of contributions in phase I.

Bound: fp32 storage and 1-ulp hardware rcp / sqrt / exp against fp64, 2e-4 of the parameter's range after two epochs — the bound of
test_gpu_mf.py, which its block cases hold at K = 300.  HINGE is left to the K = 24 cases there: its branch at exactly z = 1 can
legitimately differ between fp32 and fp64.  With CDAE_RECORD_MEASURED every case appends its worst error as
mf_tier_<model>_K<k>_B<b>_<variant> (profiles/mf_tiers_measured.txt).
"""
import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth
from helpers import record_measured
import mf_conflict_ref as cr
from test_gpu_mf import PAIRS, by_position, make, max_err

pytestmark = pytest.mark.gpu

BOUND = 2e-4
MODELS = {"imf": dict(pairwise=False, loss=cdae_amd.SQUARE), "bpr": dict(pairwise=True, loss=cdae_amd.LOG)}
SGD, NO_BIAS = dict(using_adagrad=False, learn_rate=0.02), dict(using_bias_term=False)
D40_SEED, D40_EPOCHS = 5, 2


@pytest.fixture(scope="module")
def tiny(built):
    return synth.generate_shape("tiny", seed=5)


@pytest.fixture(scope="module")
def d40(built):
    """D40, with the premise of every in-place case on it: the repeats reach the window, its edges and a chunk boundary in every
    epoch that is trained"""
    d = cr.d40()
    for pairwise, num_neg in cr.D40_SETTINGS:
        for ep in range(D40_EPOCHS):
            cr.assert_reaches_the_window(d, pairwise, num_neg, D40_SEED, ep)
    return d


def errors_by_row(m, o):
    """for a failing case: per parameter the worst relative error and the rows that carry it — a stale or wrong row shows as a few
    rows off by 1e-2 or more, rounding as a smooth spread"""
    out = {}
    for po, pg in PAIRS:
        ref = o.get(po)
        got = by_position(m, pg)
        err = np.abs(got.ravel() - ref).reshape(got.shape[0], -1).max(axis=1) / (1e-3 + np.abs(ref).max())
        worst = np.argsort(err)[::-1][:4]
        out[pg] = (float(err.max()), float(np.median(err)), worst.tolist())
    return out


def run(data, name, model, K, B, seed, variant, tag, epochs=2):
    kw = dict(MODELS[model])
    kw.update(variant)
    m, o = make(data, K=K, B=B, **kw)
    assert m.batch_users == B
    for ep in range(epochs):
        st = m.train_one_iteration(seed=seed, epoch=ep)
        assert st.users == data.num_users
        if B == 1:
            o.train_literal(seed, ep)
        else:
            o.train_batched(seed, ep, B)
    err, which = max_err(m, o)
    print(f"\nmf_tier_{model}_K{K}_B{B}_{name}_{tag}: {err:.3g} (parameter {which})")
    record_measured(f"mf_tier_{model}_K{K}_B{B}_{name}_{tag}", err=err)
    for _, pg in PAIRS:
        assert np.isfinite(m.get(pg)).all(), pg
    assert err < BOUND, (err, which, errors_by_row(m, o))
    m.close()


# ---- the sequential schedule (IN_PLACE) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 64, 65, 128, 129, 256, 257, 512])
@pytest.mark.parametrize("model", list(MODELS))
def test_sequential_schedule_at_every_tier_edge(d40, model, K):
    """both edges of NI = 1, 2, 4, 8 at the default hyper-parameters; K = 1 and the odd sizes leave padding lanes in the row"""
    run(d40, "d40", model, K, 1, D40_SEED, dict(), "default", epochs=D40_EPOCHS)


SEQ_K200 = [("imf", "default", dict()), ("bpr", "default", dict()),
            ("imf", "sgd", SGD), ("bpr", "sgd", SGD),
            ("imf", "nobias", NO_BIAS), ("bpr", "nobias", NO_BIAS),
            ("imf", "neg1", dict(num_neg=1)), ("bpr", "neg1", dict(num_neg=1)),
            ("imf", "ce", dict(loss=cdae_amd.CROSS_ENTROPY)), ("bpr", "square", dict(loss=cdae_amd.SQUARE)),
            ("bpr", "neg12", dict(num_neg=12))]


@pytest.mark.parametrize("model,tag,variant", SEQ_K200, ids=[f"{m}-{t}" for m, t, _ in SEQ_K200])
def test_sequential_schedule_variants_at_the_benchmark_dimension(d40, model, tag, variant):
    """K = 200 (NI = 4): plain SGD, no bias terms, a single negative, the other loss of each model, and BPR with 12 pairs per positive
    (420 pairs for the longest row: seven chunks, a positive's pairs across two of them)"""
    run(d40, "d40", model, 200, 1, D40_SEED, variant, tag, epochs=D40_EPOCHS)


@pytest.mark.parametrize("K", [128, 200, 512])
@pytest.mark.parametrize("model", list(MODELS))
def test_sequential_schedule_over_two_launch_windows(tiny, model, K):
    """300 users: the sequential default walks 256 users per launch, so the second launch starts from what the first one left"""
    assert tiny.num_users == 300
    run(tiny, "tiny", model, K, 1, 7, dict(), "default")


# ---- the block schedule -----------------------------------------------------------------------------------------------------------
BLOCK_VARIANTS = {"default": dict(), "sgd": SGD, "nobias": NO_BIAS, "neg1": dict(num_neg=1), "neg12": dict(num_neg=12)}


@pytest.mark.parametrize("tag", list(BLOCK_VARIANTS))
@pytest.mark.parametrize("K", [24, 200, 300])
@pytest.mark.parametrize("model", list(MODELS))
def test_block_schedule_beyond_the_defaults(tiny, model, K, tag):
    """B = 33 on 300 users: nine full blocks in activity-grouped order and a last block of three.  sgd: the plain-SGD instantiations of
    both kernels; nobias: phase U, BPR's carried positive and phase I without bias steps; neg1: no pair is ever carried; neg12: the
    carried copy outlives a prefetch group of 8 pairs and, every 64 pairs, a chunk."""
    run(tiny, "tiny", model, K, 33, 3, BLOCK_VARIANTS[tag], tag)


def test_block_schedule_orders_the_users_of_these_cases(tiny):
    m, _ = make(tiny, K=8, B=33)
    order = m.user_order()
    assert not np.array_equal(order, np.arange(tiny.num_users))
    lens = np.diff(tiny.train_ptr)[order]
    assert lens[-3:].max() <= lens[:-3].min()                 # the short last block holds the three least active users


@pytest.mark.parametrize("model", list(MODELS))
def test_one_block_of_eight_users_on_forty_items(d40, model):
    """D40 as one block: 141 positives x 6 instances (IMF) or 2 x 5 examples (BPR) on 40 item rows — a row's phase-I chain holds on
    average 21 (35) contributions per epoch, from up to eight users: more than one prefetch group of mf_item_kernel"""
    per_row = d40.nnz_train * (10 if model == "bpr" else 6) / d40.num_items
    assert per_row > 16
    run(d40, "d40", model, 200, 8, D40_SEED, dict(), "default", epochs=D40_EPOCHS)
