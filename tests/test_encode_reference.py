"""The references of tests/encode_ref.py against the fp64 oracle, and every premise tests/test_gpu_encode_exact.py relies on — on
the build machine, without a GPU, for every case table that file runs.  A premise can therefore never be what fails on the GPU.

  grid cases   the integer references equal Oracle.encode / Oracle.data_loss / Oracle.penalty_loss exactly (they are computed from
               Oracle.draw_inputs' masks, not by those functions); every sum of magnitudes is below 2^24, every |1 - y| at most 4095,
               at least 99 % of the positives have 1 - y != 0; the fp32 emulation of the documented order returns the same integers.
  real cases   the fp32 emulation of the documented order lies within its derived rounding bound of the oracle:
               (terms + 3) u / (1 - (terms + 3) u) times the sum of magnitudes, u = 2^-24.
"""
import numpy as np
import pytest

import encode_ref as ref


def ids(table):
    return [ref.case_id(t) for t in table]


@pytest.mark.parametrize("t", ref.INFERENCE_CASES, ids=ids(ref.INFERENCE_CASES))
def test_the_integer_encode_is_the_oracles(t):
    c = ref.case_of(t)
    o = ref.oracle_of(c)
    uids = ref.call_lists(c)["order"]
    for mode in (0, 1):
        Z, worst = ref.exact_encode(c, o, mode, uids)
        assert worst < 2 ** 24
        np.testing.assert_array_equal(Z, o.encode(ref.SEED, ref.EPOCH, mode, uids))
        assert np.array_equal(Z.astype(np.float32).astype(np.float64), Z)
    if c.hyper["corruption_ratio"] == 1.0:                                   # both modes encode the empty input: z = b + wu
        want = c.P["b"].astype(np.float64) + (c.P["Wu"] if "Wu" in c.P else 0.0)
        np.testing.assert_array_equal(Z, np.broadcast_to(want, Z.shape))
    else:
        assert (Z != ref.exact_encode(c, o, 0, uids)[0]).any(axis=1).mean() > 0.5      # the mask matters


def test_the_data_sets_hold_their_seams():
    for name, (U, longs, pins, I, B) in ref._DATASETS.items():
        d, b = ref.dataset(name)
        lens = np.diff(d.train_ptr)
        assert d.num_users == U and b == B and sorted(lens[lens > 3].tolist()) == sorted(n for n in longs if n > 3)
        assert all(lens[u] == n for u, n in pins.items()) and lens.min() >= 1 and lens.max() < d.num_items
        if I is None:
            assert d.num_items == lens.sum() and np.unique(d.train_col).size == d.num_items      # pairwise disjoint rows
    assert ref.unit_of(16, 50) == 64 and ref.unit_of(2048, 1100) == 128 and ref.unit_of(2048, 1024) == 64
    assert ref.unit_of(800, 800) == 64 and ref.unit_of(1100, 1400) == 128
    d, _ = ref.dataset("chunk")
    lens = np.diff(d.train_ptr)
    assert d.num_users == ref.CHUNK + 70 and lens[ref.CHUNK - 1] == 129 and lens[ref.CHUNK] == 65 and np.count_nonzero(lens > 3) == 2


def test_a_list_with_repeats_outweighs_every_batch_of_distinct_users():
    """the `repeats` list names the heaviest user batch_users times: more work units than the heaviest min(batch_users, num_users)
    distinct users have, which is what the handle's partial-sum rows are sized for (cdae_dataset_plan.h encode_unit_bound)"""
    for ds in ("seam64", "seam128"):
        c = ref.case_of((ds, 64, {}))
        units = -(-np.diff(c.data.train_ptr) // c.unit)
        B = min(c.B, c.data.num_users)
        assert units.max() * B > np.sort(units)[::-1][:B].sum()
        assert np.count_nonzero(ref.call_lists(c)["repeats"] == np.argmax(units)) >= c.B >= B


@pytest.mark.parametrize("t", [("seam64", 65, {}), ("seam64", 257, dict(gate=False)), ("seam128", 64, {})], ids=ref.case_id)
def test_the_emulation_returns_the_integers_on_the_grid(t):
    """emulate_encode in either association equals the exact integers where every order is exact: the emulator adds what it should"""
    c = ref.case_of(t)
    o = ref.oracle_of(c)
    uids = ref.call_lists(c)["order"]
    for mode in (0, 1):
        Z = ref.exact_encode(c, o, mode, uids)[0]
        for waves in (None, ref.ENC_WAVES):
            np.testing.assert_array_equal(ref.emulate_encode(c, o, mode, uids, waves)[0].astype(np.float64), Z)


@pytest.mark.parametrize("t", ref.ORDER_CASES, ids=ids(ref.ORDER_CASES))
def test_the_emulated_order_is_within_its_rounding_bound_of_the_oracle(t):
    c = ref.case_of(t)
    o = ref.oracle_of(c)
    uids = ref.call_lists(c)["order"]
    for mode in (0, 1):
        want = o.encode(ref.SEED, ref.EPOCH, mode, uids)
        two, bound = ref.emulate_encode(c, o, mode, uids)
        one, _ = ref.emulate_encode(c, o, mode, uids, ref.ENC_WAVES)
        assert (np.abs(two - want) <= bound).all() and (np.abs(one - want) <= bound).all()
        long_rows = np.diff(c.data.train_ptr) > ref.ENC_WAVES * c.unit
        assert long_rows.any() and np.array_equal(one[~long_rows], two[~long_rows])      # the same sum up to 16 units ...
        assert (one[long_rows] != two[long_rows]).any()                                  # ... and another one beyond
        assert (two != want.astype(np.float32)).mean() > 0.05                            # off the grid: the order shows in the bits


@pytest.mark.parametrize("t", ref.TRAINING_CASES, ids=ids(ref.TRAINING_CASES))
def test_the_expected_decoder_rows(t):
    c = ref.case_of(t, training=True)
    o = ref.oracle_of(c)
    assert c.hyper["num_neg"] == 0 and not c.P["V"].any() and (c.P["bp"] == -1000).all()
    V, room = ref.expected_decoder(c, o)
    assert room < ref.SECOND_CORRUPTION_ROOM
    owners = np.repeat(np.arange(c.data.num_users), np.diff(c.data.train_ptr))
    assert np.array_equal(np.sort(c.data.train_col), np.arange(c.data.num_items))        # every item row holds one positive
    if c.kind == "grid":
        Vq, worst = ref.exact_decoder(c, o)
        assert worst < 2 ** 24
        np.testing.assert_array_equal(V.astype(np.float64) / ref.LR, Vq)
        if c.hyper["num_corruptions"] == 1:
            uids = np.arange(c.data.num_users, dtype=np.uint32)
            np.testing.assert_array_equal(Vq[c.data.train_col.astype(np.int64)], o.encode(ref.SEED, ref.EPOCH, 1, uids)[owners])
    elif c.hyper["num_corruptions"] == 1:
        uids = np.arange(c.data.num_users, dtype=np.uint32)
        want = o.encode(ref.SEED, ref.EPOCH, 1, uids)
        _, bound = ref.emulate_encode(c, o, 1, uids)
        got = V[c.data.train_col.astype(np.int64)].astype(np.float64) / ref.LR
        assert (np.abs(got - want[owners]) <= bound[owners]).all()
    assert np.abs(V).max(axis=1).min() > 0                                                # no row is trivially zero


LOSS_TABLE = ref.LOSS_CASES + [ref.CHUNK_CASE] + ref.SHARDED_CASES


@pytest.mark.parametrize("t", LOSS_TABLE, ids=ids(LOSS_TABLE))
def test_the_integer_data_loss_is_the_oracles(t):
    c = ref.case_of(t)
    o = ref.oracle_of(c)
    r = ref.exact_data_loss(c, o)
    ref.assert_loss_premises(r)
    assert r["loss"] == o.data_loss(ref.SEED, ref.EPOCH) and r["loss"] > 0
    if c.hyper["lambda_"]:
        assert ref.exact_penalty(c) == o.penalty_loss() > 0
        assert r["loss"] + ref.exact_penalty(c) == o.data_loss(ref.SEED, ref.EPOCH) + o.penalty_loss()


@pytest.mark.parametrize("t", ref.PENALTY_CASES, ids=ids(ref.PENALTY_CASES))
def test_the_integer_penalty_is_the_oracles_and_leaves_the_gate_out(t):
    c = ref.case_of(t)
    assert c.flags["linear_function"] and (c.P["Uu"] != 1).any() and c.hyper["lambda_"] == 2.0 ** -6
    want = ref.exact_penalty(c)
    assert want == ref.oracle_of(c).penalty_loss() > 0
    sq = {k: float((v.astype(np.float64) ** 2).sum()) for k, v in c.P.items()}
    assert want == 0.5 * 2.0 ** -6 * sum(v for k, v in sq.items() if k != "Uu") and sq["Uu"] > 0
    assert ("Wu" in sq) == c.flags["user_factor"] and ("V" in sq) == c.flags["asymmetric"]
