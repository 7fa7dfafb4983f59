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
"""
import numpy as np
import pytest

import mf_conflict_ref as mc
import warp_ref as wr


@pytest.mark.parametrize("case", wr.CASES, ids=[c[0] for c in wr.CASES])
def test_the_free_running_reference_reaches_every_search_depth(case):
    t = wr.run_free(case)
    print({k: (round(float(v), 3) if isinstance(v, float) else v) for k, v in t.items()})
    assert t["disagreements"] == 0 and t["cnt1"] + t["cnt2_64"] + t["cnt65_499"] == t["trained"]
    assert t["cnt1"] >= 1, "no search ends at the first draw"
    assert t["cnt2_64"] >= 1, "no search ends inside the first round of 64 candidates"
    assert t["cnt65_499"] >= 1, "no search ends beyond the first round"
    assert t["exhausted"] >= 1, "no search is exhausted"
    if case[2] > 1:
        assert t["mixed_blocks"] >= 1, "no block both skips and trains pairs"
    assert t["near"] < wr.NEAR_SHARE * t["comparisons"], (t["near"], t["comparisons"])
    assert t["drift"] <= wr.DRIFT_MAX, t["drift"]               # rounding alone leaves three quarters of the GPU test's bound to the kernel
    assert t["max_abs_score"] <= wr.SCORE_MAX, t["max_abs_score"]


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
