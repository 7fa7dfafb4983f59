"""-m gpu: the fold-in (cdae_hip_fold_in_rows, fold_in_rows_kernel<NI>) BIT FOR BIT against the fp64 yardstick tests/fold_in_ref.py, on
the exact family of that file: linear activation, SQUARE loss, plain SGD, power-of-two learn rate / lambda / scale, W and V with two
+-1 entries per item row, b / b' / start wu in {-1, 0, 1}, uu = 1.  On those models every operation of the definition is exact in fp32
in any summation order, for two steps — tests/test_fold_in_reference.py PROVES that for every (case, row, step) run here, with the
real draws, and this file asserts that it runs exactly the proved list.  The frozen rows make this possible where the training step
(conflicts, an order) cannot be pinned: one dropped or doubled example, one LDS partial from the wrong wavefront, one draw index off
changes bits here and stays far below the 2e-4 of tests/test_gpu_fold_in.py.

Every case takes two steps, as two epochs ("2ep": the fitted node feeds the next z) and as num_corruptions = 2 in one epoch ("nc2":
the draw indices c n + pos and c m + i), and compares all four arrays with assert_array_equal:
  * K = 1, 2, 63, 64, 65, 128, 129, 256, 257, 300, 512: both edges of NI = 1, 2, 4, 8 (pad guard, Kp strides, the copy's pitch);
  * rows of 1, 2, 3, 42 | 43, 63, 64, 65, 128, 129, 300 items: the chunk seams, both roles, more than a chunk per wavefront;
  * num_neg = 0, 1, 5, 12 with a row either side of each role seam (256 | 257, 128 | 129, 42 | 43, 19 | 20);
  * symmetric and asymmetric tables; rows with one unrated item left (every negative the fallback, all duplicates), both roles;
  * start nodes: NO_USER, users, guests;
  * linear_function with and without user_factor at NI = 2, 4, 8, both roles (without user_factor wu / wu_ag stay 0 / 1e-4);
  * corruption_ratio = 0 (every item kept) and = 1 unscaled (nothing kept: S = 0, z = b + wu), both roles;
  * the host's slot list: 32 768 + 40 rows, long rows in BOTH chunks, the second chunk's at its first, a middle and its last slot,
    with and without install, each long row alone, and served back through the guest table; a chunk of long rows only;
  * stale staging rows: every call here follows a call of equal shape whose rows are all short and whose results differ, so a row
    the launch skips returns that call's bits.
No case reads a kernel's code, sets an environment variable or starts a process.
"""
import numpy as np
import pytest

import cdae_amd
from test_gpu_fold_in import GUEST, NO_USER, fold_all, same_bits
from test_gpu_rows import csr
from test_fold_in_reference import PROVED, proved_case

import fold_in_ref as ref

pytestmark = pytest.mark.gpu

CASES = tuple(ref.EXACT_CASES) + ("seam",)
NAMES = ("wu", "wu_ag", "uu", "uu_ag")


def test_the_cases_run_here_are_the_cases_proved_on_the_cpu():
    assert CASES == PROVED and all(proved_case(n) is ref.EXACT_CASES[n] for n in CASES if n != "seam")
    assert ref.NO_USER == NO_USER and ref.GUEST_BIT | 5 == GUEST(5)


def handle_of(family):
    """a handle over eight users of three items each, holding the family's tables: no training"""
    ocfg, P, (Wu, Uu) = family
    I, K = P["W"].shape
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.SQUARE, using_adagrad=False, linear=True, lambda_=ocfg.lambda_,
                              learn_rate=ocfg.learn_rate, corruption_ratio=ocfg.corruption_ratio, num_corruptions=ocfg.num_corruptions,
                              asymmetric=ocfg.asymmetric, user_factor=ocfg.user_factor, num_neg=ocfg.num_neg, scaled=ocfg.scaled,
                              beta=ocfg.beta, linear_function=ocfg.linear_function, batch_users=8)
    m = cdae_amd.CDAE(cfg)
    U = Wu.shape[0]
    m.set_interactions(U, I, *csr([np.array(sorted({(7 * u + k) % I for k in range(3)}), np.uint32) for u in range(U)]))
    m.init_params(0)
    m.set(cdae_amd.P_W, P["W"])
    m.set(cdae_amd.P_B, P["b"])
    m.set(cdae_amd.P_BP, P["bp"])
    if ocfg.asymmetric:
        m.set(cdae_amd.P_V, P["V"])
    if ocfg.user_factor:
        m.set(cdae_amd.P_WU, Wu)
    if ocfg.linear_function:
        m.set(cdae_amd.P_UU, Uu)
    return m


def scrub(model, ptr, uids, I):
    """a call of the same shape whose rows are all short (one item each): it leaves its results in the staging rows the next call
    uses.  -> its four arrays"""
    R = ptr.size - 1
    return fold_all(model, np.arange(R + 1, dtype=np.int64), (np.arange(R) * 13 % I).astype(np.uint32), uids, seed=ref.EXACT_SEED + 1, n_epochs=1)


def as_f32(arrays):
    out = [a.astype(np.float32) for a in arrays]
    for a, b in zip(out, arrays):
        assert np.array_equal(a.astype(np.float64), b)
    return out


def compare(got, want, rows, msg):
    for name, g, w in zip(NAMES, got, want):
        np.testing.assert_array_equal(g[rows], w[rows], err_msg=f"{msg} {name}")


def run_case(name, also=None):
    case = proved_case(name)
    family, (ptr, col, uids), start, want, _ = ref.exact_reference(case)
    ocfg, P, _ = family
    model = handle_of(family)
    if case["uids"] == "guest":
        model.set_guest_nodes(ref.guest_table(case))
    rows = np.arange(ptr.size - 1) if case["check"] is None else np.array(case["check"])
    before = scrub(model, ptr, uids, P["W"].shape[0])
    got = fold_all(model, ptr, col, uids, seed=ref.EXACT_SEED, n_epochs=case["n_epochs"])
    want32, start32 = as_f32(want), as_f32(start)
    compare(got, want32, rows, name)
    if not ocfg.user_factor:                                         # nothing but (uu, uu_ag) moves: wu / wu_ag are the start values
        assert (got[0] == 0).all() and (got[1] == np.float32(1e-4)).all()
        same_bits(got[:2], start32[:2], "without user_factor")
    if not ocfg.linear_function:
        assert (got[2] == 1).all() and (got[3] == np.float32(1e-4)).all()
    if also:
        also(model, case, (ptr, col, uids), before, got, want32, rows)
    model.close()


@pytest.mark.parametrize("name", [n for n in CASES if n != "seam"])
def test_two_steps_return_the_yardsticks_bits(built, name):
    run_case(name)


@pytest.mark.parametrize("name", ["sweep-K129-2ep", "neg0-K128-2ep", "neg1-K128-nc2", "neg12-K300-2ep", "lf-nouf-K256-2ep", "long-only-K257-2ep"])
def test_a_skipped_row_would_return_the_bits_of_the_call_before(built, name):
    """the premise of `scrub`: the all-short call of equal shape leaves other bits than the yardstick's in EVERY staging row, in the
    arrays the configuration fits — so a row that neither role takes (the host list and the device test disagreeing about which rows
    are long) cannot pass; and the call repeated returns the same bits again"""
    def also(model, case, rows_, before, got, want32, rows):
        ptr, col, uids = rows_
        k = 0 if model.cfg.user_factor else 2
        assert (before[k] != want32[k]).any(axis=1).all()
        assert (np.diff(ptr) * (1 + model.cfg.num_neg) > 256).any() and 1 + model.cfg.num_neg <= 256       # long rows here, none before
        same_bits(fold_all(model, ptr, col, uids, seed=ref.EXACT_SEED, n_epochs=case["n_epochs"]), got, "repeat")
    run_case(name, also)


def test_long_rows_in_every_chunk_of_one_call(built):
    """32 768 + 40 rows: the first chunk holds long rows at slots 5, 9 and 30, the second at its slots 0, 17 and 39 — the offset
    d_fold_long + long_off[chunk] != 0, the slot relative to c0, and under install the staging offset c0 Kp"""
    def also(model, case, rows_, before, got, want32, rows):
        ptr, col, uids = rows_
        assert all(np.isfinite(a).all() for a in got)
        inst = fold_all(model, ptr, col, uids, seed=ref.EXACT_SEED, n_epochs=case["n_epochs"], install=True)
        same_bits(inst, got, "install")                              # every row of both chunks
        assert model.num_guest_nodes == ref.SEAM_R
        for r in sorted(ref.SEAM_LONG):
            row = col[ptr[r]:ptr[r + 1]]
            alone = fold_all(model, np.array([0, row.size], np.int64), row, uids[r:r + 1], seed=ref.EXACT_SEED, n_epochs=case["n_epochs"],
                             stream_id_base=r)
            same_bits(alone, [a[r:r + 1] for a in want32], f"row {r} alone")
        # the installed table serves those bits: n_epochs = 0 from the guest ids of the second chunk and of the first chunk's head
        for lo, hi in ((ref.SEAM_CHUNK - 3, ref.SEAM_R), (0, 40)):
            back = fold_all(model, ptr[lo:hi + 1] - ptr[lo], col[ptr[lo]:ptr[hi]], GUEST(np.arange(lo, hi)), n_epochs=0)
            same_bits(back, [a[lo:hi] for a in want32], f"guests {lo}..{hi}")
        model.set_guest_nodes(np.zeros((0, ref.SEAM_K), np.float32))
    run_case("seam", also)
