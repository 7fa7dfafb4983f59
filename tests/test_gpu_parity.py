"""-m gpu: the HIP path, called through the C ABI, against the CPU oracle on identical inputs.

Tolerances: the reference computes in fp64 (src/base/mat.hpp:12,19-22); the HIP path stores and
computes in fp32 with hardware rcp/sqrt/exp (1 ulp).  Integer work (masks, negatives, top-k ids) is
bit-exact.  fp tolerances are written next to each assert.
"""
import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth
import oracle as orc
from oracle import binding as ob
from helpers import assert_valid_topk, make_pair, max_param_err, record_measured

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny(built):
    return synth.generate_shape("tiny", seed=5)


@pytest.fixture(scope="module")
def small(built):
    return synth.generate(1200, 500, 60_000, seed=9)


def test_init_params_match_counter_stream(tiny):
    model, o = make_pair(tiny, K=10)
    o.init_params(11)     # oracle's own init (fp64) vs the device init kernel (fp32 of the same fp64 value)
    for which in (0, 4):
        ref = o.get(which).astype(np.float32)
        np.testing.assert_array_equal(model.get(which).ravel(), ref)
    assert np.all(model.get(1) == np.float32(1e-4)) and np.all(model.get(8) == 0)


@pytest.mark.parametrize("K", [1, 10, 50, 64, 65, 128, 129, 200, 256, 257, 512])
@pytest.mark.parametrize("mode", [0, 1])
def test_encode_matches_oracle(tiny, K, mode):
    model, o = make_pair(tiny, K=K)
    uids = np.arange(tiny.num_users, dtype=np.uint32)[::-1].copy()      # any order, all users
    z_gpu = model.get_hidden_values(uids, seed=3, epoch=2, mode=mode)
    z_ref = o.encode(3, 2, mode, uids)
    # sigmoid outputs in (0,1): absolute tolerance 2e-6 (fp32 sum of <= ~100 rows + 1-ulp exp/rcp)
    assert np.abs(z_gpu - z_ref).max() < 2e-6


@pytest.mark.parametrize("variant", [
    dict(), dict(loss=cdae_amd.SQUARE), dict(asymmetric=True), dict(using_adagrad=False, learn_rate=0.01),
    dict(tanh=True), dict(linear=True, learn_rate=0.02), dict(user_factor=False), dict(scaled=False),
    dict(corruption_ratio=0.0, scaled=False), dict(corruption_ratio=1.0, scaled=False), dict(num_neg=1),
    dict(num_corruptions=2), dict(beta=0.0),
])
def test_sequential_schedule_tracks_reference_literal(tiny, variant):
    """batch_users = 1 is the reference's schedule: compare with the LITERAL restatement of cdae.hpp:136-358."""
    model, o = make_pair(tiny, K=24, B=1, **variant)
    for ep in range(2):
        model.train_one_iteration(seed=7, epoch=ep)
        o.train_literal(7, ep)
    err, which = max_param_err(model, o)
    # two epochs x 300 users of fp32 AdaGrad steps vs fp64: relative 2e-4 of the parameter's range
    assert err < 2e-4, (err, which)


@pytest.mark.parametrize("B", [7, 64, 300])
@pytest.mark.parametrize("variant", [dict(), dict(loss=cdae_amd.SQUARE, asymmetric=True)])
def test_batched_schedule_matches_oracle(tiny, B, variant):
    model, o = make_pair(tiny, K=40, B=B, **variant)
    for ep in range(2):
        model.train_one_iteration(seed=1, epoch=ep)
        o.train_batched(1, ep, B)
    err, which = max_param_err(model, o)
    assert err < 2e-4, (err, which)


@pytest.mark.parametrize("variant", [dict(), dict(asymmetric=True, loss=cdae_amd.SQUARE), dict(using_adagrad=False, learn_rate=0.01),
                                     dict(user_factor=False, tanh=True)])
@pytest.mark.parametrize("B,K", [(1, 24), (64, 40), (300, 200)])
def test_linear_function_gate_matches_oracle(tiny, B, K, variant):
    """linear_function (cdae.hpp:29, 382-384, 295-299, 339-340, 351-357): the per-user gate Uu on the input sum, its own
    AdaGrad step, and Uu[u] (.) delta in the input rows.  B = 1 against the LITERAL restatement, B > 1 against the block
    schedule; encode, loss and top-k go through the gate as well."""
    model, o = make_pair(tiny, K=K, B=B, linear_function=True, **variant)
    assert (model.get(cdae_amd.P_UU) == 1).all() and (model.get(cdae_amd.P_UU_AG) == np.float32(1e-4)).all()   # cdae.hpp:131-132
    for ep in range(2):
        model.train_one_iteration(seed=7, epoch=ep)
        if B == 1:
            o.train_literal(7, ep)
        else:
            o.train_batched(7, ep, B)
    assert np.abs(o.get(ob.P_UU) - 1.).max() > 1e-2          # the gate trained
    err, which = max_param_err(model, o)
    assert err < 2e-4, (err, which)
    uids = np.arange(tiny.num_users, dtype=np.uint32)
    for mode in (0, 1):      # activations in [-1, 1] from parameters that themselves agree to 2e-4 of their range
        assert np.abs(model.get_hidden_values(uids, seed=3, epoch=2, mode=mode) - o.encode(3, 2, mode, uids)).max() < 3e-4
    lg, lo = model.data_loss(5, 0), o.data_loss(5, 0)
    assert abs(lg - lo) < 3e-4 * abs(lo)
    rec_g = model.recommend_all(10)
    rec_o, sc_o = o.recommend(10, with_scores=True)
    clear = np.abs(np.diff(sc_o, axis=1)).min(axis=1) > 1e-3
    np.testing.assert_array_equal(rec_g[clear], rec_o[clear])
    assert_valid_topk(model, tiny, rec_g, 10, K, eps="derived")      # every user, the near-ties included


def test_linear_function_full_output(tiny):
    model, o = make_pair(tiny, K=24, B=48, full_output=True, linear_function=True)
    for ep in range(2):
        model.train_one_iteration(seed=4, epoch=ep)
        o.train_full(4, ep, 48)
    err, which = max_param_err(model, o)
    record_measured("linear_function_full_output", err=err, which=which)
    assert err < 4.5e-3, (err, which)                          # bf16 operands; measured 3.3e-3 (profiles/r06_measured_bf16_guards.txt; the bound was 2e-2 through round 5)


def test_loss_and_recommend_match_oracle(small):
    model, o = make_pair(small, K=50, B=256)
    for ep in range(3):
        model.train_one_iteration(seed=2, epoch=ep)
        o.train_batched(2, ep, 256)
    lg, lo = model.data_loss(5, 0), o.data_loss(5, 0)
    assert abs(lg - lo) < 2e-4 * abs(lo)                      # sum over ~48k positives, fp32 vs fp64
    pg, po = model.penalty_loss(), o.penalty_loss()
    assert abs(pg - po) < 2e-4 * abs(po)
    rec_g = model.recommend_all(10)
    rec_o, sc_o = o.recommend(10, with_scores=True)
    # ids must agree wherever the oracle's neighbouring scores are separated by more than fp32 noise
    gap = np.abs(np.diff(sc_o, axis=1)).min(axis=1)
    clear = gap > 1e-4
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(rec_g[clear], rec_o[clear])
    assert_valid_topk(model, small, rec_g, 10, 50, eps="derived")    # every user, the near-ties included
    m_g = orc.eval_topn(rec_g, small.test_ptr, small.test_col)
    m_o = orc.eval_topn(rec_o, small.test_ptr, small.test_col)
    assert np.abs(m_g - m_o).max() < 2e-3                     # a near-tie may swap one id


def test_user_range_and_offset_equal_full_run(tiny):
    """A shard with a global-id offset draws the same random streams as the full run."""
    full, _ = make_pair(tiny, K=16, B=50)
    full.train_users(seed=4, epoch=0, u_begin=100, u_end=200)
    shard_data = tiny.user_range(100, 200)
    cfg = full.cfg
    shard = cdae_amd.CDAE(cfg)
    shard.set_interactions(shard_data.num_users, shard_data.num_items, shard_data.train_ptr, shard_data.train_col,
                           user_id_offset=100)
    shard.init_params(11)
    for which in (0, 1, 6, 7, 8, 9):
        shard.set(which, make_pair(tiny, K=16, B=50)[0].get(which))
    wu = make_pair(tiny, K=16, B=50)[0]
    shard.set(4, wu.get(4)[100:200]); shard.set(5, wu.get(5)[100:200])
    shard.train_one_iteration(seed=4, epoch=0)
    for which in (0, 8, 6):
        np.testing.assert_allclose(shard.get(which), full.get(which), rtol=0, atol=1e-6)
    np.testing.assert_allclose(shard.get(4), full.get(4)[100:200], rtol=0, atol=1e-6)


def test_errors_are_reported_not_swallowed(tiny):
    with pytest.raises(cdae_amd.CDAEError, match="LOGISTIC aborts"):
        cdae_amd.CDAE(cdae_amd.CDAEConfig(lt=cdae_amd.LOGISTIC))
    m = cdae_amd.CDAE(cdae_amd.CDAEConfig(lt=cdae_amd.SQUARE))
    with pytest.raises(cdae_amd.CDAEError, match="set_interactions"):
        m.train_one_iteration(0, 0)
    ptr = np.array([0, 2, 2], dtype=np.int64)       # user 1 has no item: the reference CHECK-fails (cdae.hpp:139)
    with pytest.raises(cdae_amd.CDAEError, match="no training item"):
        m.set_interactions(2, 5, ptr, np.array([0, 1], dtype=np.uint32))
    ptr = np.array([0, 2], dtype=np.int64)
    with pytest.raises(cdae_amd.CDAEError, match="ascending"):
        m.set_interactions(1, 5, ptr, np.array([3, 1], dtype=np.uint32))


@pytest.mark.parametrize("rule", [0, 1])
def test_delta_exchange_kernel_matches_numpy_restatement(tiny, rule):
    """cdae_hip_delta_begin / _compute / _apply with a hand-made "all-reduce": one process emulating two identical ranks (the
    all-reduced buffer is 2 x this rank's).  rule 0: sum; rule 1: item rows divided by the ranks that touched them, b by the world."""
    import torch
    from cdae_amd.distributed import wrap_device_floats
    model, _ = make_pair(tiny, K=20, B=64)
    shared_ids = (0, 1, 8, 9, 6, 7)
    model.delta_begin()
    buf = wrap_device_floats(*model.delta_device_ptr())
    stream = torch.cuda.ExternalStream(model.stream_handle(), device=buf.device)     # the stream the library's delta calls run on
    before = {w: model.get(w).astype(np.float64) for w in shared_ids}
    model.train_users(seed=2, epoch=0, u_begin=0, u_end=64)
    after = {w: model.get(w).astype(np.float64) for w in shared_ids}
    model.delta_compute()
    model.synchronize()
    with torch.cuda.stream(stream):
        buf.mul_(2.0)                                  # "all-reduce" of two identical ranks
    model.delta_apply(2, rule)
    touched = (np.abs(after[1] - before[1]).sum(1) + np.abs(after[9] - before[9])) > 0
    for w in shared_ids:
        d = after[w] - before[w]
        if rule == 0:
            want = before[w] + 2 * d
        elif w in (6, 7):
            want = before[w] + 2 * d / 2
        else:
            wgt = np.where(touched, 0.5, 1.0)
            want = before[w] + 2 * d * (wgt[:, None] if d.ndim == 2 else wgt)
        np.testing.assert_allclose(model.get(w), want, rtol=0, atol=2e-6)


def test_training_is_bit_deterministic_and_handles_reload(tiny, small):
    """Two fresh handles, and a handle that held another data set before, produce bit-identical parameters: no atomics are
    left on the default path (duplicate corrections are summed in example order)."""
    cfg = cdae_amd.CDAEConfig(num_dim=40, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=96)

    def run(model, data):
        model.set_interactions(data.num_users, data.num_items, data.train_ptr, data.train_col)
        model.init_params(3)
        model.train_one_iteration(1, 0)
        return {w: model.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)}

    first = run(cdae_amd.CDAE(cfg), tiny)
    second = run(cdae_amd.CDAE(cfg), tiny)
    reused = cdae_amd.CDAE(cfg)
    run(reused, small)
    third = run(reused, tiny)
    for w in first:
        assert np.array_equal(first[w], second[w]) and np.array_equal(first[w], third[w]), w


@pytest.mark.parametrize("env", [dict(CDAE_PREP_THREAD="0"), dict(CDAE_PREP2="off"), dict(CDAE_PREP2="own"), dict(CDAE_EVENT_SYSTEM_FENCE="1"),
                                 dict(CDAE_ENCODE_TWO_LAUNCHES="1"), dict(CDAE_SORT_TILE="1"), dict(CDAE_SORT_LIBRARY="1"), dict(CDAE_SORT_SCAN="1"), dict(CDAE_PREP2="aux"),
                                 dict(CDAE_HOST_PACE_US="0"), dict(CDAE_HOST_PACE_US="5")],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_scheduling_switches_do_not_change_a_single_bit(small, monkeypatch, devlib, env):
    """The prep worker thread, the second prep lane, device-scope events, the one-launch encode, the tile counting sort and host pacing
    (round 6: the caller's thread looks for the prepared lists itself, so that the main stream carries no wait for them; 0 = the device
    always waits, 5 us = it mostly does) change WHEN work is issued and by which kernel — never the arithmetic or its order: parameters
    after two epochs are bit-identical to the default configuration's."""
    cfg = cdae_amd.CDAEConfig(num_dim=40, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64)

    def run():
        m = cdae_amd.CDAE(cfg)
        m.reset(small, seed=5)
        for ep in range(2):
            m.train_one_iteration(5, ep)
        out = {w: m.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)}
        m.close()
        return out

    base = run()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    other = run()
    for w in base:
        assert np.array_equal(base[w], other[w]), (env, w)


@pytest.mark.parametrize("K,B,kw", [(40, 300, dict()), (200, 300, dict(loss=cdae_amd.SQUARE, asymmetric=True)), (50, 128, dict(using_adagrad=False, learn_rate=0.01)),
                                    (64, 300, dict(user_factor=False, tanh=True))])
def test_fused_decode_gather_launch_changes_no_bit(tiny, monkeypatch, devlib, K, B, kw):
    """Round 6: decode and hidden-gradient gather as ONE launch (decode_gather_kernel: the gather wavefronts wait, example by
    example, for the g of rows still being decoded; g, D0 and the correction rows written through, sc1) against the SEPARATE
    launches (CDAE_DECODE_UNFUSED): the same roles, the same sums in the same order — every parameter bit-identical after two
    epochs.  The 120-item space makes duplicate negatives (correction rows, runs on late rows) the common case."""
    monkeypatch.setenv("CDAE_DECODE_HOT_POS", "6")       # enough popular ("hot") rows at these sizes: late rows + the fused launch
    monkeypatch.setenv("CDAE_DECODE_LATE_POS", "6")

    def run(expect_fused):
        m, _ = make_pair(tiny, K=K, B=B, **kw)
        plan = m.decode_plan
        assert plan["late_rows"] > 0 and plan["hot_rows"] >= plan["late_rows"] and plan["fused"] == expect_fused, plan
        for ep in range(2):
            m.train_one_iteration(seed=4, epoch=ep)
        out = {w: m.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)}
        m.close()
        return out, plan

    fused, plan = run(True)
    monkeypatch.setenv("CDAE_DECODE_UNFUSED", "1")
    apart, _ = run(False)
    for w in fused:
        assert np.array_equal(fused[w], apart[w]), (w, plan, np.abs(fused[w] - apart[w]).max())
    assert np.isfinite(fused[0]).all()


def test_set_decode_fused_switches_the_launch_and_no_bit(tiny):
    """cdae_hip_set_decode_fused (ABI 12, shipped library): a handle that may train side by side with another one on the same device takes the
    two separate launches — the same bits.  The logical shards of cdae_hip_multi_* get it from the library (tests/test_gpu_multi.py)."""
    outs = []
    for allow in (True, False):
        m, _ = make_pair(tiny, K=40, B=300)
        assert m.decode_plan["fused"], m.decode_plan                      # 300 users per batch: tiny's popular rows are hot rows
        m.set_decode_fused(allow)
        assert m.decode_plan["fused"] == allow
        for ep in range(2):
            m.train_one_iteration(seed=4, epoch=ep)
        outs.append({w: m.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)})
        m.close()
    for w in outs[0]:
        assert np.array_equal(outs[0][w], outs[1][w]), w


@pytest.mark.parametrize("B", [64, 300])
def test_late_rows_track_the_oracle_and_round_fives_arithmetic(tiny, monkeypatch, devlib, B):
    """The late rows' terms of the hidden gradient are added by hidden_finish_kernel from Ghot (one entry per user and row, one
    correction row per duplicate run) instead of being gathered: against the oracle's block schedule at the usual 2e-4, and against
    round 5's arithmetic (CDAE_NO_LATE_ROWS: every example gathered) — a different order of the same fp32 additions, 2e-5."""
    monkeypatch.setenv("CDAE_DECODE_HOT_POS", "4")
    monkeypatch.setenv("CDAE_DECODE_LATE_POS", "4")
    m, o = make_pair(tiny, K=40, B=B)
    assert m.decode_plan["late_rows"] > 0, m.decode_plan
    for ep in range(2):
        m.train_one_iteration(seed=1, epoch=ep)
        o.train_batched(1, ep, B)
    err, which = max_param_err(m, o)
    assert err < 2e-4, (err, which)
    monkeypatch.setenv("CDAE_NO_LATE_ROWS", "1")
    m5, _ = make_pair(tiny, K=40, B=B)
    assert m5.decode_plan["late_rows"] == 0 and not m5.decode_plan["fused"] and m5.decode_plan["hot_rows"] <= m.decode_plan["hot_rows"]
    for ep in range(2):
        m5.train_one_iteration(seed=1, epoch=ep)
    for w in (0, 1, 4, 5, 6, 7, 8, 9):
        a, b = m.get(w).astype(np.float64), m5.get(w).astype(np.float64)
        assert np.abs(a - b).max() <= 2e-5 * (1e-3 + np.abs(b).max()), w


def test_the_shipped_library_reads_no_developer_switch(small, monkeypatch):
    """The SHIPPED library (no `devlib` here) under every developer switch that changes results or kernels in the developer build —
    CDAE_DEBUG_SKIP_ROLES / _SKIP_PREP give WRONG results there by design — trains the same bits as without them."""
    cfg = cdae_amd.CDAEConfig(num_dim=40, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64)

    def run(full_output=False):
        m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=40, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64, full_output=full_output))
        assert m.lib is cdae_amd.load_library(cdae_amd.LIB_PATH)
        m.reset(small, seed=5)
        for ep in range(2):
            m.train_one_iteration(5, ep)
        out = {w: m.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)}
        m.close()
        return out

    base, base_full = run(), run(True)
    for k, v in dict(CDAE_DEBUG_SKIP_ROLES="63", CDAE_DEBUG_SKIP_PREP="1", CDAE_SORT_TILE="1", CDAE_DUP_CAP="2", CDAE_DECODE_ONE_ROW_PER_WAVE="1",
                     CDAE_FULL_UNFUSED="1", CDAE_FULL_B_SUMMED="1", CDAE_PREP2="off", CDAE_PREP_THREAD="0", CDAE_UNIT_POS="16",
                     CDAE_DECODE_HOT_POS="1", CDAE_ENCODE_TWO_LAUNCHES="1", CDAE_FULL_ONE_STREAM_MAX="0", CDAE_DECODE_UNFUSED="1", CDAE_NO_LATE_ROWS="1").items():
        monkeypatch.setenv(k, v)
    other, other_full = run(), run(True)
    for w in base:
        assert np.array_equal(base[w], other[w]) and np.array_equal(base_full[w], other_full[w]), w
    del cfg


def test_duplicate_correction_overflow_falls_back_to_atomics(tiny, monkeypatch, devlib):
    """CDAE_DUP_CAP bounds the duplicate-negative correction buffer; examples beyond it take the atomic path and the
    result is the same trajectory (up to the order of a few fp32 additions)."""
    monkeypatch.setenv("CDAE_DUP_CAP", "2")
    small_cap, o = make_pair(tiny, K=24, B=64, num_neg=20)          # many negatives per user -> many duplicates
    monkeypatch.delenv("CDAE_DUP_CAP")
    roomy, _ = make_pair(tiny, K=24, B=64, num_neg=20)
    for ep in range(2):
        small_cap.train_one_iteration(seed=8, epoch=ep)
        roomy.train_one_iteration(seed=8, epoch=ep)
        o.train_batched(8, ep, 64)
    err, which = max_param_err(small_cap, o)
    assert err < 2e-4, (err, which)
    for which in (0, 1, 4, 5, 6, 7, 8, 9):
        np.testing.assert_allclose(small_cap.get(which), roomy.get(which), rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("K", [1, 20, 50, 200])
def test_pipelined_exchange_kernels(tiny, K):
    """cdae_hip_delta_stage / _merge / _merge_stage with a fake peer: the "all-reduced" buffer is a multiple of the rank's
    own staged delta (so the row pads stay zero, as with real peers); the peer part must land on the live parameters one
    period late while the rank's own later steps are kept, and must never be re-sent."""
    import torch
    from cdae_amd.distributed import wrap_device_floats
    model, _ = make_pair(tiny, K=K, B=64)
    shared_ids = (0, 1, 8, 9, 6, 7)

    class ex:                                            # the receive buffer of the library's exchange, on the library's stream
        pass
    model.delta_begin(); model.delta_stage(); model.synchronize()
    ex.recv = wrap_device_floats(*model.delta_recv_device_ptr())
    ex.stream = torch.cuda.ExternalStream(model.stream_handle(), device=ex.recv.device)

    def snap():
        return {w: model.get(w).astype(np.float64) for w in shared_ids}

    def staged_sum():
        model.synchronize()
        with torch.cuda.stream(ex.stream):
            return float(ex.recv.double().sum())

    def close(a, b):
        return abs(a - b) < 1e-3 * max(1.0, abs(b))

    x0 = snap()
    model.train_users(seed=2, epoch=0, u_begin=0, u_end=64)
    x1 = snap()
    model.delta_stage()                                  # send = recv = d1 = x1 - x0 ; base = x1
    assert ex.recv.is_cuda and ex.recv.numel() == model.delta_recv_device_ptr()[1]
    assert close(staged_sum(), sum(float((x1[w] - x0[w]).sum()) for w in shared_ids))
    with torch.cuda.stream(ex.stream):
        ex.recv.mul_(3.0)                                # "all-reduce": two peers with the same delta -> their part is 2 d1
    model.train_users(seed=2, epoch=0, u_begin=64, u_end=128)      # training goes on while the "all-reduce" runs
    x2 = snap()
    model.delta_merge()                                  # x += recv - send
    model.synchronize()
    x3 = snap()
    for w in shared_ids:
        np.testing.assert_allclose(x3[w], x2[w] + 2.0 * (x1[w] - x0[w]), rtol=1e-6, atol=5e-6)
    model.delta_stage()                                  # stages d2 = x2 - x1 only: the peers' part is not re-sent
    assert close(staged_sum(), sum(float((x2[w] - x1[w]).sum()) for w in shared_ids))
    with torch.cuda.stream(ex.stream):
        ex.recv.mul_(0.5)                                # peers' part of this period: -0.5 d2
    model.train_users(seed=2, epoch=0, u_begin=128, u_end=192)
    x4 = snap()
    model.delta_merge_stage()                            # fused boundary: merge the above, stage d3 = x4 - x3
    model.synchronize()
    for w in shared_ids:
        np.testing.assert_allclose(model.get(w).astype(np.float64), x4[w] - 0.5 * (x2[w] - x1[w]), rtol=1e-6, atol=5e-6)
    assert close(staged_sum(), sum(float((x4[w] - x3[w]).sum()) for w in shared_ids))


def test_async_enqueue_and_prefetch_equal_synchronous_training(tiny):
    """enqueue_users / prefetch_users only change WHEN work is queued, never the result.  (Equality up to the
    order of the few fp32 atomics that carry duplicate-negative corrections: a few fp32 ulps.)"""
    a, _ = make_pair(tiny, K=32, B=40)
    b, _ = make_pair(tiny, K=32, B=40)
    a.train_one_iteration(seed=9, epoch=0)
    a.train_users(seed=9, epoch=1, u_begin=0, u_end=120)
    # same work, queued batch by batch with the next batch prefetched, one synchronisation at the end
    bounds = [(0, s, min(tiny.num_users, s + 40)) for s in range(0, tiny.num_users, 40)] + [(1, 0, 40), (1, 40, 80), (1, 80, 120)]
    for i, (ep, u0, u1) in enumerate(bounds):
        b.enqueue_users(9, ep, u0, u1)
        if i + 1 < len(bounds):
            b.prefetch_users(9, *bounds[i + 1])
    st = b.collect_stats()
    assert st.users == tiny.num_users + 120 and st.batches == len(bounds)
    for which in (0, 1, 4, 5, 6, 7, 8, 9):
        np.testing.assert_allclose(a.get(which), b.get(which), rtol=5e-6, atol=1e-6)
    # a prefetch that is never consumed (different range next) must not corrupt anything
    b.prefetch_users(9, 2, 0, 40)
    b.train_users(9, 2, 40, 80)
    a.train_users(9, 2, 40, 80)
    np.testing.assert_allclose(a.get(0), b.get(0), rtol=5e-6, atol=1e-6)


def test_two_batches_of_prefetch_carry_over_and_stale_drops(tiny):
    """With the second prep lane the library looks two batches ahead, and prefetch_users prepares both leading batches of a
    range.  Whether the caller then trains them in one call, one batch per call (the second prepared batch carries over), or
    walks away from them (stale: dropped), the parameters equal those of plain synchronous training of the same batches."""
    a, _ = make_pair(tiny, K=32, B=40)
    b, _ = make_pair(tiny, K=32, B=40)
    U = tiny.num_users
    a.train_users(seed=5, epoch=0, u_begin=0, u_end=U)
    a.train_users(seed=5, epoch=1, u_begin=0, u_end=160)
    a.train_users(seed=5, epoch=2, u_begin=80, u_end=160)
    # epoch 0: two-batch prefetches consumed by one-batch calls
    starts = list(range(0, U, 40))
    b.prefetch_users(5, 0, 0, min(U, 80))
    for s0 in starts:
        b.enqueue_users(5, 0, s0, min(U, s0 + 40))
        if s0 + 40 < U:
            b.prefetch_users(5, 0, s0 + 40, min(U, s0 + 120))
    # epoch 1: a two-batch prefetch consumed by one four-batch call
    b.prefetch_users(5, 1, 0, 80)
    b.enqueue_users(5, 1, 0, 160)
    # epoch 2: prepared batches that are never trained (other range, other epoch), then a partial match
    b.prefetch_users(5, 2, 0, 80)
    b.prefetch_users(5, 3, 0, 80)
    b.prefetch_users(5, 2, 80, 160)
    b.enqueue_users(5, 2, 80, 120)
    b.prefetch_users(5, 2, 120, 160)          # already carried over: nothing new to prepare
    b.enqueue_users(5, 2, 120, 160)
    st = b.collect_stats()
    assert st.users == U + 160 + 80
    for which in (0, 1, 4, 5, 6, 7, 8, 9):
        np.testing.assert_allclose(a.get(which), b.get(which), rtol=5e-6, atol=1e-6)


@pytest.fixture(scope="module")
def ragged(built):
    """Heavy-tailed rows: 1 item, a few, > 128 (several work units), > 2048 (sampler's global-memory path)."""
    rng = np.random.default_rng(3)
    I = 9000
    sizes = [1, 2, 3, 127, 128, 129, 300, 700, 2047, 2048, 2049, 2600] + list(rng.integers(5, 60, size=52))
    rows = [np.sort(rng.choice(I, size=int(n), replace=False)).astype(np.uint32) for n in sizes]
    ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    col = np.concatenate(rows)
    empty = np.zeros(len(rows) + 1, dtype=np.int64)
    return synth.Interactions(len(rows), I, ptr, col, empty, np.zeros(0, dtype=np.uint32))


@pytest.mark.parametrize("B,K", [(1, 16), (5, 200), (64, 72)])
def test_ragged_rows_multi_unit_users_and_long_rows(ragged, B, K):
    model, o = make_pair(ragged, K=K, B=B, num_neg=2)
    uids = np.arange(ragged.num_users, dtype=np.uint32)
    for mode in (0, 1):
        assert np.abs(model.get_hidden_values(uids, seed=5, epoch=1, mode=mode) - o.encode(5, 1, mode, uids)).max() < 5e-6
    model.train_one_iteration(seed=5, epoch=0)
    o.train_batched(5, 0, B)
    err, which = max_param_err(model, o)
    assert err < 2e-4, (err, which)
    lg, lo = model.data_loss(6, 0), o.data_loss(6, 0)
    assert abs(lg - lo) < 2e-4 * abs(lo)
    rec_g = model.recommend_all(10)
    rec_o, sc_o = o.recommend(10, with_scores=True)
    clear = np.abs(np.diff(sc_o, axis=1)).min(axis=1) > 1e-4
    np.testing.assert_array_equal(rec_g[clear], rec_o[clear])


def few_items_many_users():
    """60 items, 2000 users of 4 .. 13 items each (tests/test_gpu_step_tiers.py trains on it too)"""
    rng = np.random.default_rng(11)
    I, U = 60, 2000
    p = 1.0 / np.arange(1, I + 1) ** 0.8
    p /= p.sum()
    rows = [np.sort(rng.choice(I, size=int(rng.integers(4, 14)), replace=False, p=p)).astype(np.uint32) for _ in range(U)]
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    return synth.Interactions(U, I, ptr, np.concatenate(rows), np.zeros(U + 1, np.int64), np.empty(0, np.uint32))


@pytest.mark.parametrize("K,B", [(40, 2000), (200, 1500), (64, 700)])
def test_item_rows_with_thousands_of_examples_per_batch(built, K, B):
    """Few items, many users per batch: every item row holds hundreds to thousands of examples of ONE batch — the four-rows-per-
    wavefront decode walks many 64-example chunks through its LDS ring (staging, wrap at 128, g write-out per chunk), the popular
    rows exceed the LDS room their g is parked in (1280 examples) and fall back to per-chunk stores, input rows scan many chunks."""
    d = few_items_many_users()
    model, o = make_pair(d, K=K, B=B, num_neg=3)
    for ep in range(2):
        model.train_one_iteration(seed=4, epoch=ep)
        o.train_batched(4, ep, B)
    err, which = max_param_err(model, o)
    assert err < 3e-4, (err, which)          # (thousands of sequential fp32 steps per row and batch)


@pytest.mark.parametrize("K,topk", [(8, 1), (40, 10), (100, 16), (200, 10), (256, 5), (64, 20), (300, 10)])
def test_recommend_matrix_core_path(ragged, K, topk):
    """K7 on MFMA (K <= 256, topk <= 16) and the per-user fallback (topk 20, K 300): ragged user/item counts that are no
    multiples of the 128-user / 32-item tiles."""
    model, _ = make_pair(ragged, K=K, B=32, num_neg=2)
    model.train_one_iteration(seed=5, epoch=0)
    rec = model.recommend_all(topk)
    assert rec.shape == (ragged.num_users, topk)
    assert_valid_topk(model, ragged, rec, topk, K)
    part = model.recommend_all(topk, 3, ragged.num_users - 2)            # a sub-range of users
    np.testing.assert_array_equal(part, rec[3:ragged.num_users - 2])


@pytest.mark.parametrize("K", [100, 256, 300, 512])
def test_wide_rows(tiny, K):
    """NI = 2, 4 (no pad element: separate bias path), 8."""
    model, o = make_pair(tiny, K=K, B=32)
    model.train_one_iteration(seed=3, epoch=0)
    o.train_batched(3, 0, 32)
    err, which = max_param_err(model, o)
    assert err < 2e-4, (err, which)


def test_single_user_single_item_dataset(built):
    ptr = np.array([0, 1], dtype=np.int64)
    col = np.array([2], dtype=np.uint32)
    d = synth.Interactions(1, 12, ptr, col, np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.uint32))
    model, o = make_pair(d, K=8, B=1)
    for ep in range(3):
        model.train_one_iteration(seed=1, epoch=ep)
        o.train_literal(1, ep)
    err, which = max_param_err(model, o)
    assert err < 1e-4, (err, which)
    assert model.recommend_all(10).shape == (1, 10) and 2 not in model.recommend_all(10)[0]


@pytest.mark.parametrize("variant", [dict(), dict(loss=cdae_amd.SQUARE, learn_rate=0.02), dict(asymmetric=True),
                                     dict(using_adagrad=False, learn_rate=0.002)])
@pytest.mark.parametrize("B", [1, 48, 300])
def test_full_output_mfma_decode_matches_oracle(tiny, B, variant):
    """BASELINE configs[1]/[4]: every unrated item is a negative; dense decode on bf16 MFMA with fp32 accumulation.
    The oracle computes the same block-summed schedule in fp64.  Tolerance: operands (z, D) and the loss gradient
    g are rounded to bf16 (relative 2^-9 = 2e-3 each) before the three contractions, so parameters agree to
    1.3e-2 of their range after two epochs at K = 24 (measured 5e-4 .. 1.23e-2 over the twelve cases — the largest is the hidden bias
    of the 300-user block with the default flags; the bound was 2e-2 through round 4), and the loss to 1e-2 relative."""
    model, o = make_pair(tiny, K=24, B=B, full_output=True, **variant)
    for ep in range(2):
        model.train_one_iteration(seed=4, epoch=ep)
        o.train_full(4, ep, B)
    err, which = max_param_err(model, o)
    print(f"\nfull-output K=24 B={B} {variant}: max parameter error {err:.2e} of range ({which})")
    assert err < 1.3e-2, (err, which)
    lg, lo = model.current_loss(4, 0), o.data_loss(4, 0) + o.penalty_loss()
    assert abs(lg - lo) < 1e-2 * abs(lo)


def test_more_than_65536_items(built):
    """I > 65536 leaves the 16-bit sort keys (rocPRIM onesweep) for the 32-bit ones and widens every item-indexed table;
    BASELINE configs[4] (1 M items) lives there.  Sampled schedule, loss, top-k and the full-output decode vs the oracle."""
    data = synth.generate(160, 70_000, 6_400, seed=21, min_items=12)
    assert data.num_items > 65536
    model, o = make_pair(data, K=8, B=64)
    for ep in range(2):
        model.train_one_iteration(seed=3, epoch=ep)
        o.train_batched(3, ep, 64)
    err, which = max_param_err(model, o)
    assert err < 2e-4, (err, which)
    lg, lo = model.data_loss(5, 0), o.data_loss(5, 0)
    assert abs(lg - lo) < 2e-4 * abs(lo)
    rec_g = model.recommend_all(10)
    rec_o, sc_o = o.recommend(10, with_scores=True)
    clear = np.abs(np.diff(sc_o, axis=1)).min(axis=1) > 1e-4
    assert clear.mean() > 0.5
    np.testing.assert_array_equal(rec_g[clear], rec_o[clear])
    assert_valid_topk(model, data, rec_g, 10, 8, eps="derived")      # every user, the near-ties included
    full, of = make_pair(data, K=8, B=32, full_output=True)
    full.train_one_iteration(seed=3, epoch=0)
    of.train_full(3, 0, 32)
    err, which = max_param_err(full, of)
    record_measured("more_than_65536_items_full", err=err, which=which)
    assert err < 4e-3, (err, which)                            # measured 2.8e-3 (round 6; was 2e-2)


@pytest.mark.parametrize("K,B,unfused_env", [(300, 48, False), (512, 130, False), (24, 48, True), (200, 64, True), (300, 256, False)])
def test_full_output_three_gemm_path(tiny, small, monkeypatch, devlib, K, B, unfused_env):
    """K > 256 (BASELINE configs[4]: K = 512) keeps the three separate matrix-core products — GEMM 1 with the loss epilogue,
    split-K GEMM 2, GEMM 3 — instead of the fused kernel; CDAE_FULL_UNFUSED selects them for any K.  Same oracle as
    test_full_output_mfma_decode_matches_oracle; the bf16 rounding of z and D enters y = D z through K products, so the
    tolerance on the parameters is 3e-2 of their range here (measured 2.1e-2 .. 2.5e-2 on b', the smallest-valued
    parameter, at K = 200 .. 512; the fused kernel measures the same at K = 200) against 2e-2 at K = 24.  Since the end of
    round 3 the item count is padded to a multiple of 256 whenever K > 256, so blocks that fill whole 256-user tiles (B = 130 and
    256 here) take gemm1_loss_duo_kernel and gemm_tn_bf16_kernel at these small shapes too; B = 48 keeps the tiled kernels."""
    if unfused_env:
        monkeypatch.setenv("CDAE_FULL_UNFUSED", "1")
    data = small if B >= 256 else tiny      # (with 256 of tiny's 300 users per block there are two AdaGrad steps per epoch: b' alone is 3.8e-2 off)
    model, o = make_pair(data, K=K, B=B, full_output=True)
    for ep in range(2):
        model.train_one_iteration(seed=4, epoch=ep)
        o.train_full(4, ep, B)
    err, which = max_param_err(model, o)
    record_measured(f"three_gemm_path_K{K}_B{B}", err=err, which=which)
    # measured (round 6, profiles/r06_measured_bf16_guards.txt) 2.14e-2 / 2.31e-2 / 4.1e-3 / 5.5e-3 / 1.59e-2 in the order of the cases; each bound <= 1.3 x its
    # measurement (3e-2 / 2e-2 for all of them through round 5)
    bound = {(300, 48): 2.8e-2, (512, 130): 3e-2, (24, 48): 5.5e-3, (200, 64): 7.5e-3, (300, 256): 2.1e-2}[(K, B)]
    assert err < bound, (err, which, bound)
    lg, lo = model.current_loss(4, 0), o.data_loss(4, 0) + o.penalty_loss()
    assert abs(lg - lo) < 1e-2 * abs(lo)


def _clear_rows(sc, tol=1e-4):
    return np.abs(np.diff(sc, axis=1)).min(axis=1) > tol


def test_recommend_general_path_large_item_space_and_k_above_256(built):
    """num_dim in (256, 512] and topk > 16 do not fit the matrix-core top-k kernel, and 50 000 items x 4 B do not fit the
    160 KiB LDS: the general recommend path keeps its scores in a global workspace (this combination used to
    CHECK-abort the first TOPN row of Solver::train)."""
    d = synth.generate(200, 50_000, 8_000, seed=12, min_items=20)
    model, o = make_pair(d, K=300, B=64)
    model.train_one_iteration(seed=2, epoch=0)
    o.train_batched(2, 0, 64)
    for topk in (10, 20):
        rec_g = model.recommend_all(topk)
        rec_o, sc_o = o.recommend(topk, with_scores=True)
        clear = _clear_rows(sc_o)
        assert clear.mean() > 0.8
        np.testing.assert_array_equal(rec_g[clear], rec_o[clear])
        assert_valid_topk(model, d, rec_g, topk, 300, eps="derived")   # every user, the near-ties included
    # K <= 256 with topk > 16 on the same item space: general path as well
    model2, o2 = make_pair(d, K=40, B=64)
    rec_g = model2.recommend_all(24)
    rec_o, sc_o = o2.recommend(24, with_scores=True)
    clear = _clear_rows(sc_o, 1e-5)
    np.testing.assert_array_equal(rec_g[clear], rec_o[clear])
    assert_valid_topk(model2, d, rec_g, 24, 40, eps="derived")


def test_recommend_with_a_rated_set_that_is_not_the_train_row(small):
    """recommend(uid, topk, rated_item_set) encodes FROM the given set and masks exactly it (cdae.hpp:167-179): compare with
    an oracle whose row of that user IS the foreign set."""
    model, o = make_pair(small, K=50, B=128)
    model.train_one_iteration(seed=2, epoch=0)
    rng = np.random.default_rng(0)
    for uid in (0, 17, small.num_users - 1):
        row = small.train_col[small.train_ptr[uid]:small.train_ptr[uid + 1]]
        other = np.setdiff1d(np.arange(small.num_items, dtype=np.uint32), row)
        foreign = np.sort(np.concatenate([row[::2], rng.choice(other, 7, replace=False)])).astype(np.uint32)
        ptr, col = small.train_ptr.copy(), small.train_col
        col2 = np.concatenate([col[:ptr[uid]], foreign, col[ptr[uid + 1]:]])
        ptr2 = ptr.copy()
        ptr2[uid + 1:] += foreign.size - row.size
        o2 = orc.Oracle(o.cfg, small.num_users, small.num_items, ptr2, col2)
        for which in range(12):
            if o.get(which).size:
                o2.set(which, model.get(which).astype(np.float64))
        ref, sc = o2.recommend(10, uid, uid + 1, with_scores=True)
        got = model.recommend_user(uid, rng.permutation(foreign), 10)          # any order
        assert not np.intersect1d(got, foreign).size
        if _clear_rows(sc)[0]:
            np.testing.assert_array_equal(got, ref[0])
        # clear or not: a valid top-10 under the z a handle encodes from the foreign set (a twin whose train row of that user it is)
        twin = cdae_amd.CDAE(model.cfg)
        twin.set_interactions(small.num_users, small.num_items, ptr2, col2)
        twin.init_params(0)
        for which in range(12):
            if o.get(which).size:
                twin.set(which, model.get(which))
        z = twin.get_hidden_values(np.array([uid], dtype=np.uint32), mode=0)
        assert_valid_topk(model, small, got[None, :], 10, 50, eps="derived", users=[uid], rated=[foreign], Z=z)
        # the train row itself through the explicit path == the table
        np.testing.assert_array_equal(model.recommend_user(uid, row, 10), model.recommend_all(10, uid, uid + 1)[0])
    with pytest.raises(cdae_amd.CDAEError):
        model.recommend_user(0, [1, 1, 2], 10)


def test_wide_gemm_tiles_change_no_bit(built, monkeypatch, devlib):
    """K > 256 full-output path: the 256 x 256-tile kernel (round 3; all three products when rows and columns are multiples of 256)
    against the 256 x 128 / 128 x 128 ones (CDAE_GEMM_NARROW=1).  Every output element is the same sum over k in the same order
    (64-wide slices, four MFMA steps each), whatever the tile: identical G, identical slabs, identical parameters."""
    d = synth.generate(600, 33_000, 36_000, seed=6, min_items=20)
    cfg = cdae_amd.CDAEConfig(num_dim=300, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=256, full_output=True)

    def run():
        m = cdae_amd.CDAE(cfg)
        m.reset(d, seed=4)
        m.train_one_iteration(4, 0)
        out = {w: m.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)}
        loss = m.current_loss(4, 0)
        m.close()
        return out, loss

    wide, loss_w = run()
    monkeypatch.setenv("CDAE_GEMM_NARROW", "1")
    narrow, loss_n = run()
    for w in wide:
        assert np.array_equal(wide[w], narrow[w]), w
    # (the loss pass adds the users' fp64 terms with atomics: the parameters are bit-equal, the sum of the same terms to the last digit or two)
    assert abs(loss_w - loss_n) <= 1e-12 * abs(loss_n) and np.isfinite(loss_w)


@pytest.mark.parametrize("adagrad", [True, False])
def test_fused_rows_kernel_matches_separate_launches(built, monkeypatch, devlib, adagrad):
    """K > 256 over >= 32768 items (BASELINE configs[4]'s path): GEMM 3 and the row step in one launch (gemm3_rows_fused_kernel: dD
    stays in the accumulators; the rows some user kept as an input are stepped from their dD pieces by full_rows_inputs_kernel)
    against the two separate launches (CDAE_FULL_ROWS_SEPARATE=1).  One block: every dD element is the same sum over the users in
    the same order and the row step is the same expression, so W / W_ag are IDENTICAL, rows with kept inputs included; b' sums its
    gradient (the row of G^T) in another order.  Then a whole epoch of three blocks, where b' feeds the next block's forward
    product: close.  CDAE_FULL_ROWS_KH=1 (one workgroup per item tile instead of two) must not change a bit
    against the default."""
    d = synth.generate(600, 33_000, 36_000, seed=6, min_items=20)

    def run(batch_users):
        cfg = cdae_amd.CDAEConfig(num_dim=300, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=batch_users, full_output=True,
                                  using_adagrad=adagrad, learn_rate=0.1 if adagrad else 0.01)
        m = cdae_amd.CDAE(cfg)
        m.reset(d, seed=4)
        m.train_one_iteration(4, 0)
        m.train_one_iteration(4, 1)          # second epoch: the forward product reads the bf16 images the first one's row steps left
        out = {w: m.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)}
        loss = m.current_loss(4, 0)
        m.close()
        return out, loss

    fused1, loss_f1 = run(640)               # one block per epoch
    fused3, loss_f3 = run(256)
    monkeypatch.setenv("CDAE_FULL_ROWS_KH", "1")
    kh1, loss_k1 = run(256)
    monkeypatch.delenv("CDAE_FULL_ROWS_KH")
    monkeypatch.setenv("CDAE_FULL_ROWS_SEPARATE", "1")
    sep1, loss_s1 = run(640)
    sep3, loss_s3 = run(256)
    for w in fused3:
        assert np.array_equal(fused3[w], kh1[w]), w
    assert abs(loss_f3 - loss_k1) <= 1e-12 * abs(loss_f3)
    # the kept-input rows really are exercised: some rows moved by more than the no-input step could explain
    for w in fused1:
        scale = np.abs(sep1[w]).max() + 1e-30
        err = np.abs(fused1[w] - sep1[w]).max() / scale
        assert err <= 2e-5, (w, err)
        err3 = np.abs(fused3[w] - sep3[w]).max() / (np.abs(sep3[w]).max() + 1e-30)
        assert err3 <= 2e-4, (w, err3)
    assert abs(loss_f1 - loss_s1) <= 1e-5 * abs(loss_s1) and abs(loss_f3 - loss_s3) <= 1e-4 * abs(loss_s3)


@pytest.mark.parametrize("asymmetric", [False, True])
def test_fused_rows_first_block_is_bit_identical(built, monkeypatch, devlib, asymmetric):
    """One block from fresh parameters: the decoder rows (W, or V with an asymmetric decoder — then the input rows W of the kept
    items step in the second launch) and their accumulators out of the fused launch are bit-identical to the separate launches'
    (b' differs only in the order its gradient is summed: 1e-6)."""
    d = synth.generate(500, 33_000, 30_000, seed=9, min_items=20)
    cfg = cdae_amd.CDAEConfig(num_dim=300, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=512, full_output=True, asymmetric=asymmetric)

    def run():
        m = cdae_amd.CDAE(cfg)
        m.reset(d, seed=3)
        w_init = m.get(0)
        m.train_one_iteration(4, 0)
        out = {w: m.get(w) for w in ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9) if asymmetric else (0, 1, 4, 5, 6, 7, 8, 9))}
        m.close()
        return out, w_init

    fused, w_init = run()
    monkeypatch.setenv("CDAE_FULL_ROWS_SEPARATE", "1")
    sep, _ = run()
    for w in ((0, 1, 2, 3, 4, 5, 6, 7) if asymmetric else (0, 1, 4, 5, 6, 7)):
        assert np.array_equal(fused[w], sep[w]), w
    for w in (8, 9):
        np.testing.assert_allclose(fused[w], sep[w], rtol=2e-6, atol=1e-9)
    assert np.abs(fused[0] - w_init).max() > 0      # (the rows moved at all)


def test_tn_gemm2_changes_no_bit(built, monkeypatch, devlib):
    """K > 256 full-output path: hg = G D from G^T and the row-major decoder image (gemm_tn_bf16_kernel: contraction-row-major
    operands through gfx950's transposing LDS read; GEMM 1 then writes no G and D^T is never rebuilt) against G and D^T through the
    NT kernel (CDAE_GEMM2_NT=1).  Same products, same 16-wide steps in the same order, same contraction splits: identical slabs,
    identical parameters after two epochs (the second one runs on the images the first one's row steps left)."""
    d = synth.generate(600, 33_000, 36_000, seed=6, min_items=20)
    cfg = cdae_amd.CDAEConfig(num_dim=300, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=256, full_output=True)

    def run():
        m = cdae_amd.CDAE(cfg)
        m.reset(d, seed=4)
        m.train_one_iteration(4, 0)
        m.train_one_iteration(4, 1)
        out = {w: m.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)}
        rec = m.recommend_all(10, 0, 64)
        m.close()
        return out, rec

    tn, rec_tn = run()
    monkeypatch.setenv("CDAE_GEMM2_NT", "1")
    nt, rec_nt = run()
    for w in tn:
        assert np.array_equal(tn[w], nt[w]), w
    assert np.array_equal(rec_tn, rec_nt)


@pytest.mark.parametrize("loss", ["ce", "square"])
def test_gemm1_duo_changes_no_bit(built, monkeypatch, devlib, loss):
    """K = 512 full-output path: GEMM 1 with the z rows of 256 users in registers and only D staged through LDS —
    gemm1_loss_duo_kernel (the two wavefronts of a SIMD in opposite phases, whole tiles double-buffered by LDS DMA, 16-byte G^T stores
    through v_permlane32_swap) — against the 256 x 256-tile kernel (CDAE_GEMM1_TILED=1).  Every G^T element is the same sum over k in the same order and the same loss
    expression: identical parameters after two epochs, three blocks each (the last one partly filled: users past the block's end and
    items past the last one are zero in G^T)."""
    d = synth.generate(600, 33_000, 36_000, seed=6, min_items=20)
    lt = cdae_amd.CROSS_ENTROPY if loss == "ce" else cdae_amd.SQUARE
    cfg = cdae_amd.CDAEConfig(num_dim=300, lt=lt, beta=1.0, batch_users=256, full_output=True, learn_rate=0.1 if loss == "ce" else 0.02)

    def run():
        m = cdae_amd.CDAE(cfg)
        m.reset(d, seed=4)
        m.train_one_iteration(4, 0)
        m.train_one_iteration(4, 1)
        out = {w: m.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)}
        m.close()
        return out

    duo = run()                                    # gemm1_loss_duo_kernel
    monkeypatch.setenv("CDAE_GEMM1_TILED", "1")
    tiled = run()
    for w in duo:
        assert np.isfinite(tiled[w]).all()
        assert np.array_equal(duo[w], tiled[w]), ("duo", w, float(np.abs(duo[w] - tiled[w]).max()))


@pytest.mark.parametrize("variant", [dict(loss=cdae_amd.CROSS_ENTROPY), dict(loss=cdae_amd.SQUARE, using_adagrad=False, learn_rate=0.002, user_factor=False),
                                     dict(loss=cdae_amd.CROSS_ENTROPY, asymmetric=True)])
def test_k512_path_over_a_large_item_space_matches_oracle(built, variant):
    """The K > 256 launches of a large item space — GEMM 1 with the z rows in registers, GEMM 2 through the transposing LDS read, GEMM 3
    fused with the row step (>= 32768 items), the kept-input rows behind it — against the fp64 oracle's block schedule
    (Oracle.train_full) directly, not only against the launches they replace: 33 000 items, K = 300, 300 users in blocks of 256 (the
    second block ragged), two flag sets (CE + AdaGrad + user node; SQUARE + SGD, no user node).  Tolerance as
    test_full_output_three_gemm_path: operands and g are rounded to bf16."""
    d = synth.generate(300, 33_000, 20_000, seed=21, min_items=20)
    kw = dict(variant)
    loss = kw.pop("loss")
    model, o = make_pair(d, K=300, B=256, loss=loss, full_output=True, **kw)
    assert model.full_output_plan == (cdae_amd.binding.PLAN_GEMM2_TN | cdae_amd.binding.PLAN_ROWS_FUSED)
    model.train_one_iteration(seed=4, epoch=0)
    o.train_full(4, 0, 256)
    # as test_reduced_config5_k512_131072_items: a row's first block step starts from a 1e-4 accumulator, so the bf16 rounding of a
    # near-zero summed gradient becomes step-size noise on single elements of W — max 6e-2 of the range, mean far below; every
    # other parameter within 3e-2
    for which in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9):
        ref = o.get(which)
        if not ref.size:
            continue
        diff = np.abs(model.get(which).astype(np.float64).ravel() - ref) / (1e-3 + np.abs(ref).max())
        record_measured(f"k512_large_item_space_{variant.get('asymmetric', False)}_{loss}", which=which, max=diff.max(), mean=diff.mean())
        # measured over the three variants (round 6, profiles/r06_measured_bf16_guards.txt): W / V max 5.9e-2, mean 4.4e-5; the odd ids (accumulators) up to
        # 3.1e-2, the other parameters up to 7.3e-3 — the bounds are <= 1.3 x those (7e-2 / 5e-3, 6e-2, 3e-2 through round 5)
        if which in (0, 2):
            assert diff.max() <= 7e-2 and diff.mean() <= 6e-5, (which, diff.max(), diff.mean())
        elif which in (1, 3):
            continue                                   # (accumulators: the squares of those steps)
        else:                                          # (the other accumulators hold squares: twice the relative error of what they square)
            assert diff.max() <= (4.1e-2 if which % 2 else 9.5e-3), (which, diff.max())
    lg, lo = model.current_loss(4, 0), o.data_loss(4, 0) + o.penalty_loss()
    assert abs(lg - lo) < 1e-2 * abs(lo)


@pytest.mark.parametrize("U,I,B", [(257, 32_768, 256), (700, 40_000, 512), (1030, 65_537, 1024)])
def test_k512_launches_on_edge_shapes_change_no_bit(built, monkeypatch, devlib, U, I, B):
    """The three K > 256 launches together (gemm1_loss_duo_kernel, gemm_tn_bf16_kernel, gemm3_rows_fused_kernel +
    full_rows_inputs_kernel) against the launches they replace (CDAE_GEMM1_TILED, CDAE_GEMM2_NT, CDAE_FULL_ROWS_SEPARATE) on edge
    shapes: an item count that is exactly the smallest the fused row step takes / not a multiple of anything / one past 65 536 (32-bit
    sort keys), a last block of ONE user (257 = 256 + 1), of 188 and of 6 users, one / two / four user tiles per block.  Rows and
    accumulators identical; b' within its summation order."""
    d = synth.generate(U, I, 30 * U, seed=U, min_items=20)
    cfg = cdae_amd.CDAEConfig(num_dim=257, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=B, full_output=True)

    def run():
        m = cdae_amd.CDAE(cfg)
        m.reset(d, seed=2)
        m.train_one_iteration(2, 0)
        out = {w: m.get(w) for w in (0, 1, 4, 5, 6, 7, 8, 9)}
        plan = m.full_output_plan
        m.close()
        return out, plan

    new, plan = run()
    assert plan == (cdae_amd.binding.PLAN_GEMM2_TN | cdae_amd.binding.PLAN_ROWS_FUSED)
    for k in ("CDAE_GEMM1_TILED", "CDAE_GEMM2_NT", "CDAE_FULL_ROWS_SEPARATE"):
        monkeypatch.setenv(k, "1")
    old, plan_old = run()
    assert plan_old == 0
    n_blocks = -(-U // B)
    for w in new:
        assert np.isfinite(new[w]).all(), w
        if w in (8, 9) or n_blocks > 1:       # b' sums its gradient in another order (and feeds the next block's forward product)
            scale = np.abs(old[w]).max() + 1e-30
            assert np.abs(new[w] - old[w]).max() / scale <= 2e-4, w
        else:
            assert np.array_equal(new[w], old[w]), w


@pytest.mark.parametrize("K,B,kw", [(24, 64, {}), (50, 128, dict(asymmetric=True)), (200, 96, dict(lt=cdae_amd.SQUARE, learn_rate=0.02))])
def test_full_output_one_stream_order_changes_no_bit(built, monkeypatch, devlib, K, B, kw):
    """Full-output path, small item spaces: the whole block on ONE stream with the b recurrence as the leading workgroups of the row
    launch (CDAE_FULL_ONE_STREAM_MAX users per block and below) against the two-stream order (hidden layer and recurrence on the second
    stream, joined through events).  Same kernels on the same operands in the same order per stream: identical parameters."""
    d = synth.generate_shape("small", seed=5)
    lt = kw.pop("lt", cdae_amd.CROSS_ENTROPY)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=lt, beta=1.0, batch_users=B, full_output=True, **kw)

    def run():
        m = cdae_amd.CDAE(cfg)
        m.reset(d, seed=4)
        for ep in range(2):
            m.train_one_iteration(4, ep)
        out = {w: m.get(w) for w in ((0, 1, 4, 5, 6, 7, 8, 9) + ((2, 3) if kw.get("asymmetric") else ()))}
        m.close()
        return out

    monkeypatch.setenv("CDAE_FULL_ONE_STREAM_MAX", "0")
    two = run()
    monkeypatch.setenv("CDAE_FULL_ONE_STREAM_MAX", "100000")
    one = run()
    for w in two:
        assert np.array_equal(one[w], two[w]), w
