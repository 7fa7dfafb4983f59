"""CPU: the premises the WARP GPU tests rest on, asserted on the fp64 reference (tests/warp_ref.py) for the very seeds and epochs
tests/test_gpu_warp.py trains with.  A trajectory test only pins the search if the searches it follows are of every kind: a violator at
the first draw, inside the first round of 64 candidates, beyond it, and none at all; if fp32 scores are accurate far inside the band
`tol` (|score| <= 16); and if next to no comparison falls into that band, so that "the device may decide either way inside the band"
cannot hide a broken search; and if the trajectory does not amplify rounding by itself (warp_ref.CASES has the reasoning), so that the
parameter bound measures the kernel.

The loop on D40 at the eight K tier edges runs with WARPConfig's defaults.  From cdae_hip_init_params' state the score bound cannot hold
above K = 65 there: with AdaGrad and no beta a young coordinate's step is learn_rate whatever the gradient, so a pair's score moves by
about num_dim * learn_rate^2 = 1.3 ... 5.1 per step at K = 128 ... 512 (measured maxima over the two epochs, within a few percent for
every stream seed: 26.7, 24.6, 57.7, 47.4, 93.1).  Those five fixtures keep the default hyper-parameters and start their accumulators at
3, 5, 10 (warp_ref.CASES); with that start every premise below holds for them too.

The cases of the pinning pass (item biases that start at +-0.5, two dense users, a tail block of one user) meet the same premises, and
what their data adds: pairs that step with l[0], l[1] and l[2], a block of one user in every epoch.  The sensitivity test holds the
parameter bound itself to account: the fp64 reference with ONE step done wrong (warp_ref.WRONG: nine ways) must end at least 10 x 2e-4
from its true self on every case family the variant applies to, and a bias-blind loop must fail to verify the true decisions.
Draws(uid_offset) is held against a data set with users in front.

The saturation pass: SQUARE and CROSS_ENTROPY on the loop and on blocks of 8 meet the same premises.  The five cases that start their
item biases uniform in +-100 (`saturated` in their hyper-parameters) are exempt from |score| <= 16 — an fp32 score of 100 is still
accurate to 1e-5, a hundredth of tol — and must instead train pairs whose yui - score lies below -18 and below -88.5 (the shares are
printed) with a score beyond 88.5; every other premise, the float32 drift among them, holds for them as for the rest.  All of them are
held against the nine wrong loops as well.
"""
import numpy as np
import pytest

import mf_conflict_ref as mc
import warp_ref as wr


@pytest.mark.parametrize("case", wr.CASES, ids=[c[0] for c in wr.CASES])
def test_the_free_running_reference_reaches_every_search_depth(case):
    t = wr.run_free(case)
    print({k: (round(float(v), 3) if isinstance(v, float) else v) for k, v in t.items()})
    assert case[7] != 0, "the stream seed has not been chosen (tools/warp_cases.py)"
    if case[5].get("saturated"):
        print(f"{case[0]}: of {t['trained']} trained pairs {t['pred_lt18'] / t['trained']:.3f} have yui - score < -18, "
              f"{t['pred_lt88'] / t['trained']:.3f} < -88.5; max |score| {t['max_abs_score']:.4g}, drift {t['drift']:.2e}")
    # every search depth, the near-tie share, the drift, |score|; a dense data set's low rank weights; a tail block of one user
    assert not wr.unmet(case, t)


# ---- would the 2e-4 bound notice a wrong loop? ---------------------------------------------------------------------------------------
BOUND = 2e-4                     # tests/test_gpu_warp.py's parameter bound
MARGIN = 10                      # the FISM pin's: the fp64 reference with a step done wrong ends >= 10 x BOUND from the true one
SATURATED = tuple(c[0] for c in wr.CASES if c[5].get("saturated"))          # the five losses from item biases of +-100
LOOP = ("d40-loop-K65", "d40-loop-sgd", "d40-loop-log", "d40-loop-neg12", "dense-loop-K24", "d40-loop-square", "d40-loop-ce") + SATURATED
BLOCK = ("d40-block8", "d40p1-block8", "d40-block8-square", "d40-block8-ce")
BIAS = ("d40-loop-bias-K65", "d40-loop-bias-K200", "d40-block8-bias", "tiny-block33-bias-K24") + SATURATED
# variant -> (the cases it is held against, the count of run_free's totals that must be >= 1 for the variant to differ at all)
SENSITIVITY = {
    # (HINGE from biases of +-100: g = -1 for every trained pair and the biases decide every search, so a fresh yui changes no bit there)
    "yui-fresh": (tuple(n for n in LOOP + BLOCK if n != "d40-loop-bias100-hinge"), "positives_twice"),
    "post-step-uv": (LOOP + BLOCK, "trained"),
    "lambda-once": (LOOP + BLOCK, "trained"),
    "rank-minus-one": (LOOP + BLOCK, "trained"),
    "items-left-all": (LOOP + BLOCK, "trained"),
    "stale-positive-row": (LOOP + ("d40p1-block8",), "positives_twice"),       # (d40p1-block8: its tail block of one user runs in place)
    "stale-repeated-negative": (LOOP, "negatives_twice"),
    "phase-I-reversed": (BLOCK, "rows_twice"),
    "bias-blind": (BIAS, "trained"),
}
_TRUE = {}


def true_run(name):
    if name not in _TRUE:
        case = next(c for c in wr.CASES if c[0] == name)
        _TRUE[name] = (case, wr.run_free(case)) + wr.run_wrong(case)
    return _TRUE[name]


@pytest.mark.parametrize("wrong,name", [(w, n) for w, (names, _) in SENSITIVITY.items() for n in names])
def test_a_loop_with_one_step_done_wrong_ends_far_outside_the_bound(wrong, name):
    """The GPU test holds the device to 2e-4 of the fp64 reference.  That says something only if a loop that differs from the reference
    in ONE of the subtleties ends far outside: here the fp64 reference itself, run with the step done wrong, against its true self —
    at least 10 x the bound, in the measure of the bound.  `followed` is what the GPU test would see of such a device: the true reference
    FOLLOWING the wrong run's decisions — decisions it cannot verify, or parameters that far off."""
    case, totals, st, records, bad = true_run(name)
    assert not bad and wr.max_err(st, st)[0] == 0.0
    assert totals[SENSITIVITY[wrong][1]] >= 1, f"{wrong} cannot differ on {name}: no {SENSITIVITY[wrong][1]}"
    if wrong == "stale-positive-row" and case[2] > 1:
        assert totals["one_user_blocks"] >= 1
    if wrong == "bias-blind":
        assert np.abs(st.ib).max() > 0.4                                   # (the case's own start: biases are never stepped)
    w_st, w_records, _ = wr.run_wrong(case, wrong)
    dist, which = wr.max_err(w_st, st)
    f_st, _, f_bad = wr.run_wrong(case, follow=w_records)                  # the true loop following the wrong one's decisions
    f_dist, f_which = wr.max_err(w_st, f_st)
    print(f"{wrong} on {name}: {dist:.3g} ({which}) = {dist / BOUND:.0f} x bound; followed: {len(f_bad)} unverified decisions, "
          f"{f_dist:.3g} ({f_which}) = {f_dist / BOUND:.0f} x bound")
    assert dist >= MARGIN * BOUND, (dist, which)
    assert f_bad or f_dist >= MARGIN * BOUND, (f_dist, f_which)
    if wrong == "bias-blind":
        # ... and fed the TRUE decisions, the bias-blind loop cannot verify them: the biases decide which candidate is the first violator
        _, _, b_bad = wr.run_wrong(case, wrong, follow=records)
        print(f"    bias-blind following the true decisions: {len(b_bad)} unverified")
        assert len(b_bad) >= 1


def test_the_uid_offset_shifts_the_keys():
    """Draws(uid_offset=3) of D40 = rows 3.. of Draws of D40 with three users in front"""
    d = mc.d40()
    rows = [d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]] for u in range(d.num_users)]
    y = mc.from_rows([[0], [5], [39]] + rows, 40)
    dx = wr.Draws(d.train_ptr, d.train_col, 40, 2, 5, 1, uid_offset=3)
    dy = wr.Draws(y.train_ptr, y.train_col, 40, 2, 5, 1)
    dz = wr.Draws(d.train_ptr, d.train_col, 40, 2, 5, 1)
    np.testing.assert_array_equal(dx.keys, dy.keys[3:])
    assert not (dx.keys == dz.keys).any()
    np.testing.assert_array_equal(dx.head, dy.head[3 * 2:])
    assert (dx.head != dz.head).any()
    for pos in range(d.num_users):
        n = int(d.train_ptr[pos + 1] - d.train_ptr[pos])
        for p, k in ((0, 0), (n - 1, 1)):
            np.testing.assert_array_equal(dx.candidates(dx.q(pos, p, k), wr.LOOK), dy.candidates(dy.q(pos + 3, p, k), wr.LOOK))
            key = wr.rng_key(5, 1, pos + 3, wr.STREAM_NEGATIVE)
            row = rows[pos]
            assert dx.candidates(dx.q(pos, p, k), 3).tolist() == [wr.sample_negative(key, wr.draw_index(p, 2, k, t), row, 40) for t in range(3)]


def test_the_two_restatements_of_the_mixer_agree():
    """Python integers (the literal include/cdae_rng.h) against the uint64 arrays every other function here uses — on D12, whose rows
    of up to 9 of 12 items reject most draws, and on a user with every item but one, who reaches the walk behind 32 rejected draws"""
    d = mc.d12()
    dr = wr.Draws(d.train_ptr, d.train_col, d.num_items, 3, 5, 1)
    for pos in range(d.num_users):
        row = d.train_col[d.train_ptr[pos]:d.train_ptr[pos + 1]]
        key = wr.rng_key(5, 1, pos, wr.STREAM_NEGATIVE)
        assert int(dr.keys[pos]) == key
        for p, k in ((0, 0), (row.size - 1, 2)):
            lit = [wr.sample_negative(key, wr.draw_index(p, 3, k, t), row, d.num_items) for t in range(wr.LOOK)]
            np.testing.assert_array_equal(dr.candidates(dr.q(pos, p, k), wr.LOOK), lit)
            np.testing.assert_array_equal(dr.candidates(dr.q(pos, p, k), 7), lit[:7])
    full = mc.from_rows([np.delete(np.arange(40), 17), [3]], 40)
    dr = wr.Draws(full.train_ptr, full.train_col, 40, 1, 9, 0)
    key = wr.rng_key(9, 0, 0, wr.STREAM_NEGATIVE)
    walked = [wr.rng_draw(key, wr.draw_index(38, 1, 0, t) * wr.NEG_MAX_TRY + 31) * 40 >> 32 != 17 for t in range(wr.LOOK)]
    assert sum(walked) > 100                         # (draws whose 32nd candidate is still rated: the walk decides)
    assert set(dr.candidates(dr.q(0, 38, 0), wr.LOOK).tolist()) == {17}
    assert all(wr.sample_negative(key, wr.draw_index(38, 1, 0, t), full.train_col[:39], 40) == 17 for t in range(0, wr.LOOK, 50))


def test_the_rank_weights_are_the_harmonic_numbers_rounded_once():
    st = wr.init_state(3, 40, 4, 1)
    h = 0.0
    for idx in range(40):
        h += 1.0 / (idx + 1)
        assert st.l[idx] == np.float32(h)


def test_the_search_is_the_literal_loop():
    """search() against a loop written out candidate by candidate, on a state whose scores spread over the margin"""
    d = mc.d40()
    rng = np.random.default_rng(3)
    st = wr.State(rng.normal(0, 0.6, (8, 6)), np.ones((8, 6)), rng.normal(0, 0.6, (40, 6)), np.ones((40, 6)), rng.normal(0, 0.3, 40))
    dr = wr.Draws(d.train_ptr, d.train_col, 40, 2, 4, 0)
    seen = set()
    for pos in range(8):
        row = d.train_col[d.train_ptr[pos]:d.train_ptr[pos + 1]]
        key = wr.rng_key(4, 0, pos, wr.STREAM_NEGATIVE)
        for p in range(row.size):
            yui = st.ib[row[p]] + st.iv[row[p]] @ st.uv[pos]
            for k in range(2):
                want = (wr.NONE, wr.MAX_TRY)
                for t in range(wr.LOOK):
                    j = wr.sample_negative(key, wr.draw_index(p, 2, k, t), row, 40)
                    if st.ib[j] + st.iv[j] @ st.uv[pos] > yui - 1.0:
                        want = (j, t + 1)
                        break
                item, cnt, margin = wr.search(st, dr, pos, p, k)
                assert (item, cnt) == want
                seen.add("exhausted" if cnt == wr.MAX_TRY else "first" if cnt == 1 else "later")
    assert seen == {"exhausted", "first", "later"}
