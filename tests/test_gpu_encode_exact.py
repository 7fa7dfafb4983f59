"""-m gpu: the user-parallel kernel family BIT FOR BIT against tests/encode_ref.py — encode_partial_kernel + encode_finish_kernel
(cdae_hip_encode), encode_users_kernel (the one-launch training encode), data_loss_kernel and sqnorm_kernel — at every seam of the
work units: rows of 1, 7 | 8 | 9, 63 | 64 | 65, ... 1023 | 1024 | 1025, 1100 items at unit 64 and up to 2047 | 2048 | 2049 at unit
128 (tests/encode_ref.py LENGTHS64 / LENGTHS128), every row stride and both edges of each.

  tier 1  cdae_hip_encode on integer-valued models: array_equal with the integers computed from Oracle.draw_inputs' masks and with
          Oracle.encode; every call shape (in order, reversed, repeats that outweigh any batch, n = 2 B + 1, B = 1).
  tier 2  the ORDER include/cdae_hip.h documents, on real values: array_equal with its fp32 emulation.  The scale is 1 or 2 (a power
          of two), so acc * scale is exact and numpy's `acc * scale + b` rounds once, as the kernel's fused multiply-add does: the
          emulation has no double rounding to get wrong.
  tier 3  the TRAINING encode observed through the decoder, batches instead of test_gpu_saturation.py's one user: pairwise disjoint
          rows, asymmetric, CE, plain SGD, lr 2^-4, lambda 0, no negatives, V = 0, b' = -1000 — every positive's gradient is -1
          exactly, nothing but V and b' moves, and after one epoch V[i] = lr z of the owner of item i, bit for bit.  One launch at unit
          64 (rows beyond 16 units wrap the wavefronts), two launches (800 users), unit 128 with a two-launch batch and a one-launch
          tail, and two corruptions.
  tier 4  data_loss as an exact integer (SQUARE on the grid, stream-2 masks), across the 32768-user chunk seam, through three
          shards in both layouts; penalty_loss exactly, the gate Uu not counted.

tests/test_encode_reference.py proves every premise used here (magnitude sums below 2^24, |1 - y| <= 4095, >= 99 % of the positives
with 1 - y != 0, the room of the second corruption) for these very tables on the build machine.  No tolerance anywhere.
"""
import numpy as np
import pytest

import cdae_amd
import encode_ref as ref
from test_encode_reference import LOSS_TABLE, ids

pytestmark = pytest.mark.gpu

_WHICH = dict(W=cdae_amd.P_W, V=cdae_amd.P_V, Wu=cdae_amd.P_WU, b=cdae_amd.P_B, bp=cdae_amd.P_BP, Uu=cdae_amd.P_UU)


def config_of(c, batch_users=None):
    return cdae_amd.CDAEConfig(num_dim=c.K, lt=c.loss, batch_users=c.B if batch_users is None else batch_users, **c.flags, **c.hyper)


def model_of(c, batch_users=None, cls=cdae_amd.CDAE, **kw):
    """a handle (or a MultiCDAE) over the case's data set that holds the case's parameters"""
    m = cls(config_of(c, batch_users), **kw)
    m.set_interactions(c.data.num_users, c.data.num_items, c.data.train_ptr, c.data.train_col)
    m.init_params(0)
    for name, a in c.P.items():
        m.set(_WHICH[name], a)
    return m


def same_bits(got, want, msg):
    assert got.dtype == np.float32 and want.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=msg)


def encode(m, mode, uids):
    return m.get_hidden_values(uids, seed=ref.SEED, epoch=ref.EPOCH, mode=mode)


# ---- tier 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ref.INFERENCE_CASES, ids=ids(ref.INFERENCE_CASES))
def test_encode_returns_the_integers(built, t):
    c = ref.case_of(t)
    o = ref.oracle_of(c)
    m = model_of(c)
    assert m.batch_users == c.B
    for mode in (0, 1):
        for name, uids in ref.call_lists(c).items():
            Z, worst = ref.exact_encode(c, o, mode, uids)
            assert worst < 2 ** 24
            got = encode(m, mode, uids)
            same_bits(got, Z.astype(np.float32), f"mode {mode} {name}")
            if name == "order":
                np.testing.assert_array_equal(got.astype(np.float64), o.encode(ref.SEED, ref.EPOCH, mode, uids), err_msg=f"oracle, mode {mode}")
    m.close()


@pytest.mark.parametrize("K", ref.CALL_SHAPE_K)
@pytest.mark.parametrize("B", [7, 1])
def test_encode_walks_a_list_in_chunks_of_the_batch(built, K, B):
    """n = 2 B + 1 users (three chunks, the last of one user) on a handle with batch_users = 7, and batch_users = 1"""
    c = ref.case_of(("seam64", K, {}))
    o = ref.oracle_of(c)
    m = model_of(c, batch_users=B)
    lens = np.diff(c.data.train_ptr)
    heavy = np.argsort(-lens)[:10]
    uids = np.r_[heavy[:5], 2, heavy[5:], 3, 49, 5, 0].astype(np.uint32)             # long rows at both ends of a chunk and across its seam
    assert uids.size == 15 and m.batch_users == B
    for mode in (0, 1):
        same_bits(encode(m, mode, uids), ref.exact_encode(c, o, mode, uids)[0].astype(np.float32), f"mode {mode}")
    m.close()


# ---- tier 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ref.ORDER_CASES, ids=ids(ref.ORDER_CASES))
def test_encode_sums_in_the_documented_order(built, t):
    """real-valued parameters: the bits are those of the order include/cdae_hip.h documents, restated in fp32 by
    encode_ref.emulate_encode.  scale = 1 or 2: the fused multiply-add of the finish rounds once and so does its numpy form."""
    c = ref.case_of(t)
    assert c.kind == "real" and c.scale in (1.0, 2.0)
    o = ref.oracle_of(c)
    m = model_of(c)
    for name, a in c.P.items():
        same_bits(m.get(_WHICH[name]), a, name)
    for mode in (0, 1):
        for name, uids in ref.call_lists(c).items():
            same_bits(encode(m, mode, uids), ref.emulate_encode(c, o, mode, uids)[0], f"mode {mode} {name}")
    m.close()


# ---- tier 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ref.TRAINING_CASES, ids=ids(ref.TRAINING_CASES))
def test_training_encode_through_the_decoder(built, t):
    c = ref.case_of(t, training=True)
    o = ref.oracle_of(c)
    m = model_of(c)
    U, nc = c.data.num_users, c.hyper["num_corruptions"]
    assert m.batch_users == c.B
    st = m.train_one_iteration(seed=ref.SEED, epoch=ref.EPOCH)
    assert st.users == U * nc
    V = m.get(cdae_amd.P_V)
    if c.kind == "grid":
        Vq, worst = ref.exact_decoder(c, o)
        assert worst < 2 ** 24
        np.testing.assert_array_equal(V.astype(np.float64) / ref.LR, Vq)
    else:
        want, room = ref.expected_decoder(c, o)
        assert room < ref.SECOND_CORRUPTION_ROOM
        same_bits(V, want, "V = lr z")
    if nc == 1:                                            # hg = 0: nothing on the input side moved, across batches too
        for name in ("W", "Wu", "b", "Uu"):
            if name in c.P:
                same_bits(m.get(_WHICH[name]), c.P[name], name)
        assert (m.get(cdae_amd.P_BP) == np.float32(-1000.0 + ref.LR)).all()
    m.close()


# ---- tier 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ref.LOSS_CASES, ids=ids(ref.LOSS_CASES))
def test_data_loss_is_the_integer(built, t):
    c = ref.case_of(t)
    o = ref.oracle_of(c)
    r = ref.exact_data_loss(c, o)
    ref.assert_loss_premises(r)
    m = model_of(c)
    got = m.data_loss(ref.SEED, ref.EPOCH)
    assert got == o.data_loss(ref.SEED, ref.EPOCH) == r["loss"], (got, r)
    assert m.data_loss(ref.SEED, ref.EPOCH) == got                     # and again: nothing left over in the workspace
    m.close()


def test_data_loss_across_the_chunk_seam(built):
    """32768 + 70 users: the long rows are the last user of the first chunk (129 items, three units) and the first of the second
    (65 items) — the unit prefix offset by the chunk's first user, the slot relative to it, both corruptions"""
    assert ref.CHUNK_CASE in LOSS_TABLE
    c = ref.case_of(ref.CHUNK_CASE)
    o = ref.oracle_of(c)
    r = ref.exact_data_loss(c, o)
    ref.assert_loss_premises(r)
    m = model_of(c)
    got = m.data_loss(ref.SEED, ref.EPOCH)
    assert got == o.data_loss(ref.SEED, ref.EPOCH) == r["loss"], (got, r)
    uids = np.arange(ref.CHUNK - 3, ref.CHUNK + 3, dtype=np.uint32)
    for mode in (0, 1):
        same_bits(encode(m, mode, uids), ref.exact_encode(c, o, mode, uids)[0].astype(np.float32), f"mode {mode}")
    m.close()


@pytest.mark.parametrize("t", ref.PENALTY_CASES, ids=ids(ref.PENALTY_CASES))
def test_penalty_loss_is_exact_and_leaves_the_gate_out(built, t):
    """0.5 lambda (|W|^2 + |V|^2 + |Wu|^2 + |b|^2 + |b'|^2) with lambda = 2^-6 on the grid, under linear_function with Uu != 1: Uu is
    not counted (cdae.hpp:103-107); V only when asymmetric; without user_factor there is no Wu term"""
    c = ref.case_of(t)
    assert c.flags["linear_function"] and (c.P["Uu"] != 1).any()
    m = model_of(c)
    assert m.penalty_loss() == ref.oracle_of(c).penalty_loss() == ref.exact_penalty(c)
    m.close()


@pytest.mark.parametrize("item_rows", [False, True], ids=["user-shards", "item-rows"])
@pytest.mark.parametrize("t", ref.SHARDED_CASES, ids=ids(ref.SHARDED_CASES))
def test_current_loss_of_three_shards_is_the_same_integer(built, t, item_rows):
    """user-sharded: the per-shard losses added; item rows: phase 0, the all-reduce of the input sums, the finish and the loss of each
    shard's rows.  current_loss = data_loss + penalty_loss, both exact (multiples of 2^-8 far below 2^53)"""
    c = ref.case_of(t)
    o = ref.oracle_of(c)
    r = ref.exact_data_loss(c, o)
    ref.assert_loss_premises(r)
    want = r["loss"] + ref.exact_penalty(c)
    assert ref.exact_penalty(c) > 0 and want == o.data_loss(ref.SEED, ref.EPOCH) + o.penalty_loss()
    m = model_of(c, cls=cdae_amd.MultiCDAE, devices=[0] * 3, item_rows=item_rows)
    assert len(m.shards()) == 3
    assert m.current_loss(ref.SEED, ref.EPOCH) == want
    m.close()
