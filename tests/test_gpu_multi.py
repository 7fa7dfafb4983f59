"""-m gpu: data parallelism behind the C ABI (cdae_hip_multi_*, cdae_hip_comm_*, cdae_hip_exchange_*; cdae_multi.hip).

One MI355X is all a test box has, so the multi-shard handle runs as LOGICAL shards of GPU 0 (device_ids all equal: same
schedule as one shard per GPU, the all-reduce is the library's fixed-order sum kernel instead of RCCL), and RCCL itself is
exercised through a one-rank communicator owned by the library.  What is asserted:
  * the multi handle == N single handles driven by hand through cdae_hip_delta_stage / _merge with a sum in between —
    bit for bit, synchronous and pipelined (the protocol of cdae_amd/distributed.py, now inside the library);
  * one shard == the plain single handle; get / set_param address global matrices; loss and top-k are the sharded sums;
  * a one-rank RCCL exchange is the identity and leaves the parameters bit-identical to a run without exchange.
"""
import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth
from cdae_amd.distributed import _DeviceBuffer

pytestmark = pytest.mark.gpu

HYPER = dict(num_neg=5, num_corruptions=1, corruption_ratio=0.5, scaled=True, learn_rate=0.1, beta=1.0, lambda_=0.01)
SHARED = [cdae_amd.P_W, cdae_amd.P_W_AG, cdae_amd.P_B, cdae_amd.P_B_AG, cdae_amd.P_BP, cdae_amd.P_BP_AG]


@pytest.fixture(scope="module")
def small(built):
    return synth.generate(1200, 500, 60_000, seed=9)


def cfg_of(K=24, B=32, **kw):
    return cdae_amd.CDAEConfig(num_dim=K, batch_users=B, **{"lt": cdae_amd.CROSS_ENTROPY, **HYPER, **kw})


def emulate(d, cfg, cuts, init_seed, seed, epochs, period):
    """N single handles + the stage / sum / merge protocol by hand (what cdae_multi.hip's local_epoch does)"""
    import torch
    dev = torch.device("cuda", 0)
    ms, sends, recvs = [], [], []
    for u0, u1 in cuts:
        sd = d.user_range(u0, u1)
        m = cdae_amd.CDAE(cfg)
        m.set_interactions(sd.num_users, sd.num_items, sd.train_ptr, sd.train_col, user_id_offset=u0)
        m.init_params(init_seed)
        m.delta_begin(); m.delta_stage(); m.synchronize()
        ps, _ = m.delta_device_ptr()
        pr, n = m.delta_recv_device_ptr()
        sends.append(torch.as_tensor(_DeviceBuffer(ps, n), device=dev))
        recvs.append(torch.as_tensor(_DeviceBuffer(pr, n), device=dev))
        ms.append(m)
    sizes = [u1 - u0 for u0, u1 in cuts]
    B = min(cfg.batch_users, min(sizes))
    steps = -(-max(sizes) // B)
    per = [-(-n // steps) for n in sizes]

    def boundary(pending, start_next):
        for m in ms:
            (m.delta_merge_stage if pending and start_next else m.delta_merge if pending else m.delta_stage)()
        if start_next:
            for m in ms:
                m.synchronize()
            total = sends[0].clone()
            for t in sends[1:]:
                total += t
            for t in recvs:
                t.copy_(total)
            torch.cuda.synchronize()

    for ep in range(epochs):
        pending, n = False, 0
        for t in range(steps):
            for r, m in enumerate(ms):
                a, b = min(sizes[r], t * per[r]), min(sizes[r], (t + 1) * per[r])
                if b > a:
                    m.enqueue_users(seed, ep, a, b)
            n += 1
            if period == 0:
                boundary(False, True); boundary(True, False)
            elif n % period == 0:
                boundary(pending, True); pending = True
        if period:
            boundary(pending, True); boundary(True, False)
        for m in ms:
            m.synchronize()
    return ms


@pytest.mark.parametrize("period", [0, 1, 3])
@pytest.mark.parametrize("shards", [2, 5])
def test_multi_handle_equals_the_hand_driven_protocol_bit_for_bit(small, shards, period):
    cfg = cfg_of()
    mm = cdae_amd.MultiCDAE(cfg, devices=[0] * shards, exchange_every=period)
    mm.reset(small, seed=11)
    cuts = mm.shards()
    assert cuts[0][0] == 0 and cuts[-1][1] == small.num_users and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    nnz = [int(small.train_ptr[b] - small.train_ptr[a]) for a, b in cuts]
    assert max(nnz) - min(nnz) < 0.1 * sum(nnz) / shards          # balanced by interactions
    st = None
    for ep in range(2):
        st = mm.train_one_iteration(3, ep)
    assert st.users == small.num_users
    ref = emulate(small, cfg, cuts, 11, 3, 2, period)
    for which in SHARED:
        got = mm.get(which)
        for r in ref:                                            # every replica ends an epoch with the same shared block
            np.testing.assert_array_equal(got, r.get(which))
    np.testing.assert_array_equal(mm.get(cdae_amd.P_WU), np.concatenate([r.get(cdae_amd.P_WU) for r in ref]))
    np.testing.assert_array_equal(mm.get(cdae_amd.P_WU_AG), np.concatenate([r.get(cdae_amd.P_WU_AG) for r in ref]))
    # the reported loss and the top-10 lists are the shards' own, put together
    loss = sum(r.data_loss(5, 0) for r in ref) + ref[0].penalty_loss() + sum(
        0.5 * HYPER["lambda_"] * float((r.get(cdae_amd.P_WU).astype(np.float64) ** 2).sum()) for r in ref[1:])
    assert abs(mm.current_loss(5, 0) - loss) <= 1e-6 * abs(loss)
    np.testing.assert_array_equal(mm.recommend_all(10), np.concatenate([r.recommend_all(10) for r in ref]))
    np.testing.assert_array_equal(mm.recommend_all(7, 100, 900), np.concatenate([r.recommend_all(7) for r in ref])[100:900])


def test_shards_that_share_a_device_do_not_take_the_fused_launch(built):
    """Round 6: the fused decode + gather launch must not run side by side with another handle's on one device (its gather wavefronts hold
    their slots while they wait); the library switches it off for logical shards — and leaves it on for a handle of its own."""
    import ctypes as C
    d = synth.generate_shape("tiny", seed=5)
    cfg = cfg_of(K=40, B=300)
    one = cdae_amd.CDAE(cfg)
    one.reset(d, seed=1)
    assert one.decode_plan["fused"] and one.decode_plan["late_rows"] > 0
    mm = cdae_amd.MultiCDAE(cfg, devices=[0, 0])
    mm.reset(d, seed=1)
    for s in range(2):
        h, f, l = C.c_void_p(), C.c_uint32(9), C.c_uint32(9)
        assert mm.lib.cdae_hip_multi_shard(mm.h, s, C.byref(h), None, None) == 0
        assert mm.lib.cdae_hip_decode_plan(h, None, C.byref(l), C.byref(f)) == 0
        assert f.value == 0
    one.close(); mm.close()


def test_one_shard_is_the_single_handle(small):
    cfg = cfg_of(B=64)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0])
    mm.reset(small, seed=11)
    one = cdae_amd.CDAE(cfg)
    one.reset(small, seed=11)
    for ep in range(2):
        mm.train_one_iteration(3, ep)
        one.train_one_iteration(3, ep)
    for which in SHARED + [cdae_amd.P_WU, cdae_amd.P_WU_AG]:
        np.testing.assert_array_equal(mm.get(which), one.get(which))


def test_sharded_init_and_random_streams_are_those_of_the_single_gpu_run(small):
    """Wu rows and the masks / negatives of a shard are keyed by GLOBAL user id: with a one-user-per-step schedule nothing but
    the exchange differs from the single run, and at epoch 0 / step 0 not even that."""
    cfg = cfg_of(B=16)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0, 0, 0])
    mm.reset(small, seed=11)
    one = cdae_amd.CDAE(cfg)
    one.reset(small, seed=11)
    for which in SHARED + [cdae_amd.P_WU, cdae_amd.P_WU_AG]:
        np.testing.assert_array_equal(mm.get(which), one.get(which))
    # set_param scatters the private rows to their shards and broadcasts the shared block
    rng = np.random.default_rng(0)
    wu = rng.normal(size=(small.num_users, cfg.num_dim)).astype(np.float32)
    w = rng.normal(size=(small.num_items, cfg.num_dim)).astype(np.float32)
    mm.set(cdae_amd.P_WU, wu); mm.set(cdae_amd.P_W, w)
    one.set(cdae_amd.P_WU, wu); one.set(cdae_amd.P_W, w)
    np.testing.assert_array_equal(mm.get(cdae_amd.P_WU), wu)
    np.testing.assert_array_equal(mm.get(cdae_amd.P_W), w)
    assert abs(mm.current_loss(5, 0) - one.current_loss(5, 0)) <= 1e-6 * abs(one.current_loss(5, 0))
    np.testing.assert_array_equal(mm.recommend_all(10), one.recommend_all(10))


def test_synchronous_collective_on_the_main_stream_changes_no_bit(small, monkeypatch, devlib):
    """Round 6: a rank that owns its device issues the SYNCHRONOUS exchange's all-reduce on its main stream (stage -> all-reduce -> merge in
    stream order, no event hand-off to the collective stream and back).  Against round 5's hand-off (CDAE_XCHG_COLLECTIVE_STREAM, developer
    build): the same buffers and kernels in the same order — bit-identical parameters."""
    def run():
        a = cdae_amd.CDAE(cfg_of(B=64))
        a.reset(small, seed=11)
        a.comm_init_rank(1, 0, cdae_amd.comm_unique_id())
        a.exchange_configure(0)
        for lo in range(0, small.num_users, 64):
            a.enqueue_users(3, 0, lo, min(small.num_users, lo + 64))
            a.exchange_step()
        a.exchange_flush()
        a.synchronize()
        out = {w: a.get(w) for w in SHARED + [cdae_amd.P_WU]}
        a.close()
        return out
    main = run()
    monkeypatch.setenv("CDAE_XCHG_COLLECTIVE_STREAM", "1")
    side = run()
    for w in main:
        assert np.array_equal(main[w], side[w]), w


@pytest.mark.parametrize("period", [0, 2])
def test_library_owned_rccl_communicator_with_one_rank(small, period):
    """ncclGetUniqueId / ncclCommInitRank / ncclAllReduce inside the library, beside the training kernels: a one-rank group
    sums nothing in, so training with the exchange on must give the parameters of training without it — to fp32 rounding:
    the merge rebuilds cur as A + (cur - A) (that form is what keeps REPLICAS bit-identical, see delta_pipe_kernel)."""
    cfg = cfg_of(B=64)
    a = cdae_amd.CDAE(cfg)
    a.reset(small, seed=11)
    uid = cdae_amd.comm_unique_id()
    assert len(uid) == 128 and any(uid)
    a.comm_init_rank(1, 0, uid)
    with pytest.raises(cdae_amd.CDAEError):
        a.comm_init_rank(1, 0, uid)                              # one communicator per handle
    t = a.exchange_time_all_reduce(3)
    assert 0.0 < t < 0.1
    a.exchange_configure(period)
    b = cdae_amd.CDAE(cfg)
    b.reset(small, seed=11)
    for lo in range(0, small.num_users, 64):
        hi = min(small.num_users, lo + 64)
        a.enqueue_users(3, 0, lo, hi)
        a.exchange_step()
        b.enqueue_users(3, 0, lo, hi)
    a.exchange_flush()
    a.synchronize(); b.synchronize()
    for which in SHARED + [cdae_amd.P_WU]:
        ref = b.get(which)
        np.testing.assert_allclose(a.get(which), ref, rtol=0, atol=2e-5 * max(1e-3, float(np.abs(ref).max())))


def test_bad_shard_layouts_are_rejected(built):
    with pytest.raises(cdae_amd.CDAEError):
        cdae_amd.MultiCDAE(cfg_of(), devices=[])
    with pytest.raises(cdae_amd.CDAEError):
        cdae_amd.MultiCDAE(cfg_of(), devices=[0, 0, 7])           # neither all distinct nor all equal
    m = cdae_amd.MultiCDAE(cfg_of(), devices=[0, 0])
    with pytest.raises(cdae_amd.CDAEError):
        m.train_one_iteration(1, 0)                              # no data yet


# ---- CDAE_LAYOUT_ITEM_ROWS: the shards cut the item rows (full-output decode; BASELINE configs[4] layout) ---------------------
def _param_range_err(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / (1e-3 + np.abs(b).max()))


@pytest.mark.parametrize("K,B,shards", [(24, 48, 2), (24, 300, 3), (200, 64, 4), (300, 64, 2), (512, 32, 3)])
def test_item_rows_layout_is_the_single_gpu_full_output_schedule(built, K, B, shards):
    """Every shard owns a range of item rows and sees every user; two [batch x K] all-reduces per batch.  Same steps in the same
    order as the single handle — only the two cross-shard sums are associated differently (fp32), and z passes through bf16 on
    its way into the products, so a last-bit difference in z can move a product by one bf16 ulp: parameters agree to 5e-3 of
    their range after two epochs (the single handle itself is 2e-2 … 3e-2 from the fp64 oracle, tests/test_gpu_parity.py)."""
    d = synth.generate_shape("tiny", seed=5)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, batch_users=B, full_output=True, **HYPER)
    one = cdae_amd.CDAE(cfg)
    one.reset(d, seed=11)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0] * shards, item_rows=True)
    mm.reset(d, seed=11)
    cuts = mm.shards()                                          # item ranges in this layout
    assert cuts[0][0] == 0 and cuts[-1][1] == d.num_items and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    for which in SHARED + [cdae_amd.P_WU, cdae_amd.P_WU_AG]:     # W rows are initialised by GLOBAL item id
        np.testing.assert_array_equal(mm.get(which), one.get(which))
    for ep in range(2):
        st = mm.train_one_iteration(3, ep)
        one.train_one_iteration(3, ep)
        assert st.users == d.num_users and st.examples == d.nnz_train
    errs = {w: _param_range_err(mm.get(w), one.get(w)) for w in SHARED + [cdae_amd.P_WU, cdae_amd.P_WU_AG]}
    print("\nitem-rows layout vs single handle:", {k: round(v, 6) for k, v in errs.items()})
    assert max(errs.values()) < 5e-3, errs
    # reported loss and top-10 of the SAME parameters: copy the single handle's into the shards
    for which in SHARED + [cdae_amd.P_WU, cdae_amd.P_WU_AG]:
        mm.set(which, one.get(which))
        np.testing.assert_array_equal(mm.get(which), one.get(which))
    la, lb = mm.current_loss(5, 0), one.current_loss(5, 0)
    assert abs(la - lb) <= 2e-5 * abs(lb), (la, lb)
    topk = 10
    rec_m, rec_o = mm.recommend_all(topk), one.recommend_all(topk)
    agree = (rec_m == rec_o).all(axis=1).mean()
    assert agree > 0.97, agree                                  # near-ties may swap (fp32 sum order of the encode)
    for u in range(d.num_users):
        rated = d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]
        assert len(set(rec_m[u].tolist())) == topk and not np.intersect1d(rec_m[u], rated).size


def test_item_rows_layout_tracks_the_oracle_block_schedule(built):
    d = synth.generate_shape("tiny", seed=5)
    import oracle as orc
    from oracle import binding as ob
    K, B = 24, 48
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, batch_users=B, full_output=True, **HYPER)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0, 0, 0], item_rows=True)
    mm.reset(d, seed=11)
    o = orc.Oracle(orc.OracleConfig(num_dim=K, loss_type=ob.LOSS_CE, **HYPER), d.num_users, d.num_items, d.train_ptr, d.train_col)
    o.init_params(11)
    for which in SHARED + [cdae_amd.P_WU, cdae_amd.P_WU_AG]:
        o.set(which, mm.get(which).astype(np.float64))
    for ep in range(2):
        mm.train_one_iteration(4, ep)
        o.train_full(4, ep, B)
    for which in SHARED + [cdae_amd.P_WU]:
        ref = o.get(which)
        from helpers import record_measured
        record_measured("item_rows_full_output_vs_oracle", which=which, err=np.abs(mm.get(which).astype(np.float64).ravel() - ref).max() / (1e-3 + np.abs(ref).max()))
        assert np.abs(mm.get(which).astype(np.float64).ravel() - ref).max() / (1e-3 + np.abs(ref).max()) < 3.4e-3      # measured <= 2.63e-3 (round 6; was 2e-2)


# ---- the SAMPLED decode in the item-rows layout: the single-GPU schedule itself, over item shards (round 3) ------------------
PRIVATE = [cdae_amd.P_WU, cdae_amd.P_WU_AG]


def _all_params(m, extra=()):
    return {w: m.get(w) for w in SHARED + PRIVATE + list(extra)}


@pytest.mark.parametrize("K,B,kw", [(24, 48, {}), (200, 64, {}), (24, 300, dict(num_corruptions=2)), (40, 37, dict(asymmetric=True)),
                                    (24, 48, dict(linear_function=True)), (24, 48, dict(user_factor=False)), (300, 16, {})])
def test_item_rows_sampled_with_one_shard_is_the_single_handle_bit_for_bit(built, K, B, kw):
    """One item shard runs the three phases (input sums -> z, decode + local hidden gradient, hidden-layer + input-row steps) on
    ALL rows: the same kernels on the same lists, every sum in the same order — so it IS the single handle, bit for bit.  What
    the phases add is only where the two per-user sums would cross shards."""
    d = synth.generate_shape("tiny", seed=5)
    cfg = cfg_of(K=K, B=B, **kw)
    one = cdae_amd.CDAE(cfg)
    one.reset(d, seed=11)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0], item_rows=True)
    mm.reset(d, seed=11)
    extra = ([cdae_amd.P_V, cdae_amd.P_V_AG] if kw.get("asymmetric") else []) + ([cdae_amd.P_UU, cdae_amd.P_UU_AG] if kw.get("linear_function") else [])
    for ep in range(2):
        st = mm.train_one_iteration(3, ep)
        ref = one.train_one_iteration(3, ep)
        assert (st.users, st.batches, st.examples) == (ref.users, ref.batches, ref.examples)
    a, b = _all_params(mm, extra), _all_params(one, extra)
    for w in a:
        np.testing.assert_array_equal(a[w], b[w], err_msg=f"parameter {w}")
    la, lb = mm.current_loss(5, 0), one.current_loss(5, 0)      # (bit-equal parameters; the loss pass adds its fp64 terms with atomics: last digits)
    assert abs(la - lb) <= 1e-12 * abs(lb)


@pytest.mark.parametrize("K,B", [(24, 48), (300, 64)])
def test_item_rows_full_output_with_one_shard_is_the_single_handle_bit_for_bit(built, K, B):
    """Full-output decode, one item shard: the products and the two-stream tail are the single handle's launches (K 24: the fused
    kernel, K 300: the K > 256 products).  The schedules differ in where hg is summed — slab_sum_kernel, then hidden_finish_kernel
    over the sum, against hidden_finish_kernel over the slabs — and in who writes the bf16 images; neither changes a bit."""
    d = synth.generate_shape("tiny", seed=5)
    cfg = cfg_of(K=K, B=B, full_output=True)
    one = cdae_amd.CDAE(cfg)
    one.reset(d, seed=11)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0], item_rows=True)
    mm.reset(d, seed=11)
    for ep in range(2):
        mm.train_one_iteration(3, ep)
        one.train_one_iteration(3, ep)
    a, b = _all_params(mm), _all_params(one)
    for w in a:
        np.testing.assert_array_equal(a[w], b[w], err_msg=f"parameter {w}")


@pytest.mark.parametrize("K,B,shards,kw", [(24, 48, 2, {}), (24, 300, 3, {}), (200, 64, 4, {}), (300, 32, 2, {}), (24, 48, 3, dict(asymmetric=True)),
                                           (24, 48, 2, dict(linear_function=True)), (24, 64, 5, dict(lt=cdae_amd.SQUARE, beta=1.0))])
def test_item_rows_sampled_layout_is_the_single_gpu_schedule(built, K, B, shards, kw):
    """N item shards: every shard samples the batch's WHOLE example list (negatives rejected against the whole rows) and keeps the
    examples of its rows; per-row chains are untouched; only the two cross-shard sums (input sums, hidden gradient) are associated
    differently in fp32.  Parameters after two epochs within 1e-4 of their range of the single handle's (measured ~1e-6), same
    reported loss, same top-10; the user node is sharded by user range and reassembles to the single handle's Wu."""
    d = synth.generate_shape("tiny", seed=5)
    cfg = cfg_of(K=K, B=B, **kw)
    one = cdae_amd.CDAE(cfg)
    one.reset(d, seed=11)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0] * shards, item_rows=True)
    mm.reset(d, seed=11)
    cuts = mm.shards()
    assert cuts[0][0] == 0 and cuts[-1][1] == d.num_items and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    extra = ([cdae_amd.P_V, cdae_amd.P_V_AG] if kw.get("asymmetric") else []) + ([cdae_amd.P_UU, cdae_amd.P_UU_AG] if kw.get("linear_function") else [])
    for w, v in _all_params(mm, extra).items():                  # rows initialised by GLOBAL item / user id
        np.testing.assert_array_equal(v, one.get(w))
    for ep in range(2):
        st = mm.train_one_iteration(3, ep)
        ref = one.train_one_iteration(3, ep)
        assert (st.users, st.batches, st.examples) == (ref.users, ref.batches, ref.examples)
    errs = {w: _param_range_err(v, one.get(w)) for w, v in _all_params(mm, extra).items()}
    print(f"\nsampled item-rows layout, {shards} shards vs single handle:", {k: float(f"{v:.2e}") for k, v in errs.items()})
    assert max(errs.values()) < 1e-4, errs
    for w in SHARED + PRIVATE + extra:                           # loss / top-10 of the SAME parameters
        mm.set(w, one.get(w))
        np.testing.assert_array_equal(mm.get(w), one.get(w))
    la, lb = mm.current_loss(5, 0), one.current_loss(5, 0)
    assert abs(la - lb) <= 2e-5 * abs(lb), (la, lb)
    rec_m, rec_o = mm.recommend_all(10), one.recommend_all(10)
    assert (rec_m == rec_o).all(axis=1).mean() > 0.97
    for u in range(d.num_users):
        rated = d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]
        assert len(set(rec_m[u].tolist())) == 10 and not np.intersect1d(rec_m[u], rated).size


@pytest.mark.parametrize("K,B,shards,kw", [(1, 1, 3, {}), (64, 7, 2, dict(num_neg=1)), (130, 1000, 8, {}), (24, 50, 3, dict(corruption_ratio=0.0, scaled=False)),
                                           (24, 50, 4, dict(corruption_ratio=1.0, scaled=False)), (33, 299, 6, dict(num_corruptions=3, tanh=True)),
                                           (16, 64, 2, dict(using_adagrad=False, learn_rate=0.02)), (20, 33, 3, dict(linear=True, user_factor=False))])
def test_item_rows_sampled_layout_edge_shapes(built, K, B, shards, kw):
    """one user per batch over three shards, a batch larger than the data set, shards of a handful of rows, no / total corruption,
    several corruptions, SGD, linear hidden layer: always the single handle's trajectory"""
    d = synth.generate_shape("tiny", seed=5)
    cfg = cfg_of(K=K, B=B, **kw)
    one = cdae_amd.CDAE(cfg)
    one.reset(d, seed=2)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0] * shards, item_rows=True)
    mm.reset(d, seed=2)
    for ep in range(2):
        st = mm.train_one_iteration(9, ep)
        ref = one.train_one_iteration(9, ep)
        assert (st.users, st.batches, st.examples) == (ref.users, ref.batches, ref.examples)
    errs = {w: _param_range_err(v, one.get(w)) for w, v in _all_params(mm).items() if v.size}
    assert max(errs.values()) < 1e-4, errs
    assert abs(mm.current_loss(5, 0) - one.current_loss(5, 0)) <= 2e-5 * abs(one.current_loss(5, 0))


def test_item_rows_sampled_with_a_user_who_rated_almost_everything_and_shards_without_examples(built):
    """the sampler's fallback walk (a user who rated all but 3 items) lands on the same negatives in every shard; a shard none of
    whose rows a batch touches only runs its per-batch clears"""
    rng = np.random.default_rng(3)
    I = 400
    rows = [np.sort(rng.choice(I, n, replace=False)).astype(np.uint32) for n in (I - 3, 30, 17, 2, 120, 5)]
    rows += [np.sort(rng.choice(40, 6, replace=False)).astype(np.uint32) for _ in range(20)]      # users who only know the first 40 items
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    d = synth.Interactions(len(rows), I, ptr, np.concatenate(rows), np.zeros(len(rows) + 1, np.int64), np.empty(0, np.uint32))
    cfg = cfg_of(K=12, B=4, num_neg=2)
    one = cdae_amd.CDAE(cfg)
    one.reset(d, seed=2)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0] * 5, item_rows=True)
    mm.reset(d, seed=2)
    for ep in range(2):
        mm.train_one_iteration(4, ep)
        one.train_one_iteration(4, ep)
    errs = {w: _param_range_err(v, one.get(w)) for w, v in _all_params(mm).items()}
    assert max(errs.values()) < 1e-4, errs


def test_item_rows_sampled_layout_tracks_the_oracle_block_schedule(built):
    import oracle as orc
    from oracle import binding as ob
    d = synth.generate_shape("tiny", seed=5)
    K, B = 24, 48
    cfg = cfg_of(K=K, B=B)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0, 0, 0], item_rows=True)
    mm.reset(d, seed=11)
    o = orc.Oracle(orc.OracleConfig(num_dim=K, loss_type=ob.LOSS_CE, **HYPER), d.num_users, d.num_items, d.train_ptr, d.train_col)
    o.init_params(11)
    for which in SHARED + PRIVATE:
        o.set(which, mm.get(which).astype(np.float64))
    for ep in range(2):
        mm.train_one_iteration(4, ep)
        o.train_batched(4, ep, B)
    for which in SHARED + PRIVATE:
        ref = o.get(which)
        err = np.abs(mm.get(which).astype(np.float64).ravel() - ref).max() / (1e-3 + np.abs(ref).max())
        assert err < 2e-4, (which, err)


def test_item_rows_layout_shards_the_user_node_by_user(built):
    """Wu / Wu_ag live on the shard that owns the user (contiguous user ranges balanced by interactions), not on
    every shard: the shard handles' own tables add up to the user count, and a shard's table is exactly its range of the global Wu."""
    import ctypes as C
    d = synth.generate_shape("tiny", seed=5)
    cfg = cfg_of(K=24, B=48)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0] * 4, item_rows=True)
    mm.reset(d, seed=11)
    mm.train_one_iteration(3, 0)
    wu = mm.get(cdae_amd.P_WU)
    lib, rows, at = mm.lib, [], 0
    for s in range(4):
        h = C.c_void_p()
        assert lib.cdae_hip_multi_shard(mm.h, s, C.byref(h), None, None) == 0
        p, n = C.c_void_p(), C.c_size_t()
        assert lib.cdae_hip_param_device_ptr(h, cdae_amd.P_WU, C.byref(p), C.byref(n)) == 0
        r = n.value // lib.cdae_hip_row_stride(h)
        out = np.empty((r, 24), np.float32)
        assert lib.cdae_hip_get_param(h, cdae_amd.P_WU, out.ctypes.data, out.size) == 0
        np.testing.assert_array_equal(out, wu[at:at + r])
        rows.append(r)
        at += r
    assert sum(rows) == d.num_users and max(rows) < d.num_users and min(rows) > 0


@pytest.mark.parametrize("K,B,shards,kw", [(24, 48, 1, {}), (24, 48, 3, {}), (200, 64, 4, {}), (24, 300, 5, dict(num_corruptions=2)), (40, 37, 2, dict(asymmetric=True))])
def test_item_rows_sampled_with_the_tile_counting_sort_changes_no_bit(built, monkeypatch, devlib, K, B, shards, kw):
    """Round 4: a sampled item shard may order its example list with the four tile kernels of cdae_sort_kernels.hpp instead of the
    library radix sort (CDAE_SORT_TILE; the kernels give an example on another shard's row — VOID — no ticket and no place).  The
    item-major order, the segment table and the duplicate marks are the same, so two epochs end on the same bits."""
    d = synth.generate_shape("small", seed=5)
    cfg = cfg_of(K=K, B=B, **kw)

    def run():
        mm = cdae_amd.MultiCDAE(cfg, devices=[0] * shards, item_rows=True)
        mm.reset(d, seed=11)
        for ep in range(2):
            mm.train_one_iteration(3, ep)
        extra = [cdae_amd.P_V, cdae_amd.P_V_AG] if kw.get("asymmetric") else []
        out = _all_params(mm, extra)
        mm.close()
        return out

    lib = run()
    monkeypatch.setenv("CDAE_SORT_TILE", "1")
    tile = run()
    for w in lib:
        np.testing.assert_array_equal(lib[w], tile[w], err_msg=f"parameter {w}")


# ---- cdae_hip_multi_set_schedule (ABI 11): relay part + combine rule of the user-sharded layout -----------------------------
def test_relayed_epochs_are_the_single_gpu_schedule_bit_for_bit(small):
    """relay_epochs >= the epochs trained: every epoch is the single-GPU schedule — users in Solver<CDAE>::train's order
    (cdae.hpp:136-146), in blocks of batch_users, the block of shared parameters handed from shard to shard.  ONE handle that holds
    everybody and is walked range by range over the same cuts takes the same blocks from the same streams: equal bits."""
    cfg = cfg_of(B=32)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0] * 3)
    mm.set_schedule(relay_epochs=2.0)
    mm.reset(small, seed=11)
    one = cdae_amd.CDAE(cfg)
    one.reset(small, seed=11)
    for ep in range(2):
        st = mm.train_one_iteration(3, ep)
        assert st.users == small.num_users
        for a, b in mm.shards():
            one.train_users(3, ep, a, b)
    for which in SHARED + [cdae_amd.P_WU, cdae_amd.P_WU_AG]:
        np.testing.assert_array_equal(mm.get(which), one.get(which))
    np.testing.assert_array_equal(mm.recommend_all(10), one.recommend_all(10))


def test_a_fraction_of_an_epoch_is_relayed_then_the_rest_is_exchanged(small):
    """relay_epochs = 1.4: epoch 0 is relayed whole, epoch 1 relays global users [0, 0.4 U) — through the cut they cross — and
    exchanges the rest in steps of sync_batch_users per shard; restated with single handles and the hand-driven protocol."""
    import torch
    cfg = cfg_of(B=32)
    shards, sync_b = 3, 8
    mm = cdae_amd.MultiCDAE(cfg, devices=[0] * shards)
    mm.set_schedule(period=0, sync_batch_users=sync_b, relay_epochs=1.4)
    mm.reset(small, seed=11)
    cuts = mm.shards()
    for ep in range(2):
        st = mm.train_one_iteration(3, ep)
        assert st.users == small.num_users
    # the same by hand
    dev = torch.device("cuda", 0)
    ms = []
    for u0, u1 in cuts:
        sd = small.user_range(u0, u1)
        m = cdae_amd.CDAE(cfg)
        m.set_interactions(sd.num_users, sd.num_items, sd.train_ptr, sd.train_col, user_id_offset=u0)
        m.init_params(11)
        ms.append(m)

    def hand_on(dst, src):
        for which in SHARED:
            dst.set(which, src.get(which))

    U = small.num_users
    for ep in range(2):
        R = U if ep == 0 else int((1.4 - ep) * U + 1e-6)
        first, last = [0] * shards, 0
        for s, (u0, u1) in enumerate(cuts):
            if u0 >= R:
                break
            if s:
                hand_on(ms[s], ms[s - 1])
            first[s] = min(R, u1) - u0
            ms[s].train_users(3, ep, 0, first[s])
            last = s
        for s in range(shards):
            if s != last:
                hand_on(ms[s], ms[last])
        if R == U:
            continue
        sends, recvs = [], []
        for m in ms:
            m.delta_begin(); m.delta_stage(); m.synchronize()
            ps, _ = m.delta_device_ptr()
            pr, n = m.delta_recv_device_ptr()
            sends.append(torch.as_tensor(_DeviceBuffer(ps, n), device=dev))
            recvs.append(torch.as_tensor(_DeviceBuffer(pr, n), device=dev))
        rest = [u1 - u0 - f for (u0, u1), f in zip(cuts, first)]
        steps = max(1, -(-max(rest) // sync_b))
        per = [-(-n // steps) for n in rest]
        for t in range(steps):
            for s, m in enumerate(ms):
                n = cuts[s][1] - cuts[s][0]
                a, b = min(n, first[s] + t * per[s]), min(n, first[s] + (t + 1) * per[s])
                if b > a:
                    m.enqueue_users(3, ep, a, b)
            for m in ms:
                m.delta_stage()
            for m in ms:
                m.synchronize()
            total = sends[0].clone()
            for x in sends[1:]:
                total += x
            for x in recvs:
                x.copy_(total)
            torch.cuda.synchronize()
            for m in ms:
                m.delta_merge()
        for m in ms:
            m.synchronize()
    for which in SHARED:
        for m in ms:
            np.testing.assert_array_equal(mm.get(which), m.get(which))
    np.testing.assert_array_equal(mm.get(cdae_amd.P_WU), np.concatenate([m.get(cdae_amd.P_WU) for m in ms]))


def test_global_accumulator_combine_is_its_statement(small):
    """CDAE_COMBINE_GLOBAL_ACC (cdae_exchange_algebra.h pipe_pair): per (parameter, accumulator) pair the replicas exchange their
    accumulator growth and their step with their own preconditioner taken back out; the merge takes one step with the accumulator that
    has seen everybody.  One synchronous step of three shards against the same formula in numpy (fp32 operations in the same order up
    to the association of the three-term sum), and the properties that make it a combine RULE: an element only one replica moved
    ends exactly where that replica put it; replicas agree bit for bit."""
    cfg = cfg_of(B=16)
    shards = 3
    mm = cdae_amd.MultiCDAE(cfg, devices=[0] * shards)
    mm.set_schedule(period=0, combine=cdae_amd.COMBINE_GLOBAL_ACC)
    mm.reset(small, seed=11)
    cuts = mm.shards()
    before = {w: mm.get(w) for w in SHARED}
    mm.train_one_iteration(3, 0)
    # the replicas of every shard agree
    hs = []
    for s in range(shards):
        hs.append({w: mm.shard_get(s, w) for w in SHARED})
    for w in SHARED:
        for s in range(1, shards):
            np.testing.assert_array_equal(hs[0][w], hs[s][w])
    # one global step by hand: three single handles, each trains ITS first step's users from the common parameters
    ms = []
    for u0, u1 in cuts:
        sd = small.user_range(u0, u1)
        m = cdae_amd.CDAE(cfg)
        m.set_interactions(sd.num_users, sd.num_items, sd.train_ptr, sd.train_col, user_id_offset=u0)
        m.init_params(11)
        ms.append(m)
    sizes = [u1 - u0 for u0, u1 in cuts]
    steps = -(-max(sizes) // 16)
    per = [-(-n // steps) for n in sizes]
    beta = np.float32(HYPER["beta"])
    cur = {w: before[w].copy() for w in SHARED}
    for t in range(steps):
        after = []
        for s, m in enumerate(ms):
            for w in SHARED:
                m.set(w, cur[w])
            a, b = min(sizes[s], t * per[s]), min(sizes[s], (t + 1) * per[s])
            if b > a:
                m.train_users(3, 0, a, b)
            after.append({w: m.get(w) for w in SHARED})
        for p, acc in ((cdae_amd.P_W, cdae_amd.P_W_AG), (cdae_amd.P_B, cdae_amd.P_B_AG), (cdae_amd.P_BP, cdae_amd.P_BP_AG)):
            da = [x[acc] - cur[acc] for x in after]
            dp = [(x[p] - cur[p]) * (beta + np.sqrt(x[acc])) for x in after]
            new_acc = cur[acc] + ((da[0] + da[1]) + da[2])
            new_p = cur[p] + ((dp[0] + dp[1]) + dp[2]) / (beta + np.sqrt(new_acc))
            movers = sum((x[p] != cur[p]).astype(np.int32) for x in after)
            only = movers == 1
            if only.any():     # an element one replica moved: that replica's value up to the rounding of (x * d) / d
                mover_val = sum(np.where(x[p] != cur[p], x[p], np.float32(0)) for x in after)
                assert np.abs(new_p[only] - mover_val[only]).max() <= 4e-7 * max(1.0, np.abs(mover_val[only]).max())
            cur[acc], cur[p] = new_acc.astype(np.float32), new_p.astype(np.float32)
    for w in SHARED:
        scale = max(1e-3, float(np.abs(cur[w]).max()))
        assert np.abs(hs[0][w] - cur[w]).max() <= 1e-4 * scale, w
    # and it is a different rule from the sum where several replicas moved an element
    ms2 = cdae_amd.MultiCDAE(cfg, devices=[0] * shards)
    ms2.reset(small, seed=11)
    ms2.train_one_iteration(3, 0)
    assert np.abs(ms2.get(cdae_amd.P_W) - hs[0][cdae_amd.P_W]).max() > 1e-4


# ---- the one-host-thread-per-GPU code paths on a one-GPU box (developer build: every shard on a ONE-RANK communicator) ---------------
def _plan(sizes, B):
    steps = max(1, -(-max(sizes) // B))
    return steps, [-(-n // steps) for n in sizes]


@pytest.mark.parametrize("period", [0, 2])
def test_thread_per_shard_loop_and_rccl_calls_with_one_rank_communicators(small, monkeypatch, devlib, period):
    """devices = [0, 0, 0] driven like three GPUs: ncclCommInitRank per shard, one host thread per shard for the epoch, every boundary
    through ncclAllReduce under the group guard, the flush — the code a real N-GPU run executes.  A one-rank all-reduce is the identity,
    so every shard must end exactly where a single handle ends that trains the same users in the same steps on its own."""
    monkeypatch.setenv("CDAE_MULTI_ONE_RANK_COMMS", "1")
    cfg = cfg_of(B=32)
    mm = cdae_amd.MultiCDAE(cfg, devices=[0, 0, 0], exchange_every=period)
    mm.reset(small, seed=11)
    cuts = mm.shards()
    for ep in range(2):
        st = mm.train_one_iteration(3, ep)
        assert st.users == small.num_users
    sizes = [b - a for a, b in cuts]
    steps, per = _plan(sizes, 32)
    for s, (u0, u1) in enumerate(cuts):
        sd = small.user_range(u0, u1)
        m = cdae_amd.CDAE(cfg)
        m.set_interactions(sd.num_users, sd.num_items, sd.train_ptr, sd.train_col, user_id_offset=u0)
        m.init_params(11)
        # the same boundaries by hand (cdae_multi.hip step_single / flush_single): a one-rank all-reduce leaves the staged delta as it is,
        # but STAGE / MERGE still run — c = A + (c - snap) after A += (c - A) is c only up to an ulp, so they belong to the expected bits
        st = {"pending": False, "n": 0, "begun": False}

        def begin_if_needed():                # cdae_multi.hip begin_if_needed: the base is taken at the FIRST boundary, behind the first step's training
            if not st["begun"]:
                m.delta_begin(); m.delta_stage()
                st["begun"] = True

        def boundary(start_next):
            if st["pending"] and start_next:
                m.delta_merge_stage()
            elif st["pending"]:
                m.delta_merge()
            elif start_next:
                m.delta_stage()
            st["pending"] = start_next

        for ep in range(2):
            for t in range(steps):
                a, b = min(sizes[s], t * per[s]), min(sizes[s], (t + 1) * per[s])
                if b > a:
                    m.enqueue_users(3, ep, a, b)
                begin_if_needed()
                st["n"] += 1
                if period == 0:
                    boundary(True); boundary(False)
                elif st["n"] % period == 0:
                    boundary(True)
            begin_if_needed()
            if period != 0 or st["pending"]:
                boundary(True); boundary(False)
            m.synchronize()
        for w in SHARED:
            got, want = mm.shard_get(s, w), m.get(w)
            print(f"shard {s} parameter {w}: bit-equal {np.array_equal(got, want)}, max |diff| {np.abs(got - want).max():.2e}")
            # the hand-driven boundaries reproduce the library's to the last ulp of the STAGE / MERGE algebra (measured <= 3.6e-7 on
            # parameters of order 1 after two epochs); what the test is for is that every call of the thread-per-shard loop executes
            np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
        m.close()
    mm.close()


@pytest.mark.parametrize("full_output", [False, True])
def test_item_rows_thread_per_shard_loop_runs_on_one_rank_communicators(small, monkeypatch, devlib, full_output):
    """the item-rows layout's one-thread-per-GPU batch loop (phases + two all-reduces per batch on each shard's own communicator):
    with one-rank communicators the sums stay local — the numbers are not the model's — but every call of the loop executes, returns
    and leaves finite parameters; evaluation (single-thread group calls) runs behind it"""
    monkeypatch.setenv("CDAE_MULTI_ONE_RANK_COMMS", "1")
    mm = cdae_amd.MultiCDAE(cfg_of(B=64, full_output=full_output), devices=[0, 0], item_rows=True)
    mm.reset(small, seed=11)
    st = mm.train_one_iteration(3, 0)
    assert st.users == small.num_users
    assert np.isfinite(mm.get(cdae_amd.P_W)).all() and np.isfinite(mm.current_loss(5, 0))
    assert mm.recommend_all(10).shape == (small.num_users, 10)
    mm.close()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("item_rows", [False, True])
def test_a_failing_shard_thread_ends_the_epoch_with_an_error_not_a_hang(small, monkeypatch, devlib, item_rows):
    """GroupGuard: shard 1's thread fails at its fourth step; it aborts the group's communicators, its peers return, the call reports
    the shard's own message, and the handle answers every later call with the abort — nothing blocks (pytest-timeout is the judge)."""
    monkeypatch.setenv("CDAE_MULTI_ONE_RANK_COMMS", "1")
    monkeypatch.setenv("CDAE_MULTI_FAIL_AT", "1:3")
    mm = cdae_amd.MultiCDAE(cfg_of(B=32), devices=[0, 0, 0], item_rows=item_rows)
    mm.reset(small, seed=11)
    with pytest.raises(cdae_amd.CDAEError, match="forced failure"):
        mm.train_one_iteration(3, 0)
    with pytest.raises(cdae_amd.CDAEError, match="aborted"):
        mm.train_one_iteration(3, 1)
    mm.close()
