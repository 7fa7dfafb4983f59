"""-m gpu: WARP training (cdae_hip_create_warp, cdae_warp_kernels.hpp) against tests/warp_ref.py, the fp64 restatement of the loop
and of the block schedule, over two epochs.

A WARP trajectory branches on comparisons of scores, and an fp32 and an fp64 score may fall on different sides of a margin; one flipped
decision changes everything after it.  So the handle records its choices (record_choices) and after every epoch the reference FOLLOWS
them, verifying each one: every candidate before the chosen one has margin <= +tol, the chosen one > -tol, a skipped pair nothing above
+tol among its 499 candidates (tol = 1e-3; tests/test_warp_reference.py shows that next to no comparison falls into that band and that
the searches are of every depth).  Decisions that differ from the reference's own free decision are counted and capped at 1e-3 of the
comparisons — they are expected to be 0; the cap only keeps the band from hiding a broken search.  The parameters must then agree within
tests/test_gpu_mf.py's bound: 2e-4 of the parameter's range (the same arithmetic — fp32 storage, 1-ulp rcp / sqrt — against fp64).

Cases (warp_ref.CASES): the loop on D40 at both edges of every K tier with the defaults (from K = 128 on the accumulators start at 3, 5, 10
and not at 1e-4, so that |score| stays below 16: warp_ref.CASES has the reasoning); at K = 200 with plain SGD, LOG loss, num_neg 1
and 12; the loop on "tiny" (300 users: two launch windows); blocks of 8 on D40; blocks of 33 on "tiny" at K = 24, 200 and 300 (a partial
last block, the activity-grouped order of user_order()).
"""
import numpy as np
import pytest

import cdae_amd
import warp_ref as wr
from helpers import record_measured

pytestmark = pytest.mark.gpu

TABLES = (("uv", cdae_amd.P_WU), ("uva", cdae_amd.P_WU_AG), ("iv", cdae_amd.P_W), ("iva", cdae_amd.P_W_AG))
USER_INDEXED = {cdae_amd.P_WU, cdae_amd.P_WU_AG}


def config(K, num_neg, B, hyper):
    return cdae_amd.WARPConfig(num_dim=K, num_neg=num_neg, batch_users=B, lt=hyper.get("loss", cdae_amd.HINGE),
                               using_adagrad=hyper.get("adagrad", True), learn_rate=hyper.get("learn_rate", 0.1), lambda_=hyper.get("lambda_", 0.1))


def by_position(m, which, order):
    a = m.get(which).astype(np.float64)
    return a[order] if which in USER_INDEXED else a


def in_training_order(d, order):
    lens = np.diff(d.train_ptr)[order]
    ptr = np.r_[0, np.cumsum(lens)].astype(np.int64)
    col = np.concatenate([d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]] for u in order]).astype(np.uint32)
    return ptr, col


def make(case):
    name, ds, B, K, num_neg, hyper, pseed, sseed = case
    d = wr.fixture_data(ds)
    m = cdae_amd.WARP(config(K, num_neg, B, hyper))
    m.reset(d, seed=pseed)
    if hyper.get("acc0"):                                                  # a fixture that starts its accumulators elsewhere (warp_ref.CASES)
        m.set(cdae_amd.P_WU_AG, np.full((d.num_users, K), hyper["acc0"], dtype=np.float32))
        m.set(cdae_amd.P_W_AG, np.full((d.num_items, K), hyper["acc0"], dtype=np.float32))
    order = m.user_order().astype(np.int64)
    assert sorted(order.tolist()) == list(range(d.num_users))
    if B == 1:
        np.testing.assert_array_equal(order, np.arange(d.num_users))      # the reference's order
    ptr, col = in_training_order(d, order)
    st = wr.State(*(by_position(m, w, order) for _, w in TABLES), m.get(cdae_amd.P_BP), **hyper)
    ini = wr.init_state(d.num_users, d.num_items, K, pseed, **hyper)      # IMF's init: the same streams, keyed by position
    for n, _ in TABLES:
        np.testing.assert_allclose(getattr(st, n), getattr(ini, n), rtol=1e-6, atol=1e-9)
    assert not st.ib.any() and not m.get(cdae_amd.P_UB).any()
    return d, m, st, order, ptr, col


def max_err(m, st, order):
    worst, name = 0.0, None
    for n, w in TABLES:
        ref = getattr(st, n)
        err = np.abs(by_position(m, w, order) - ref).max() / (1e-3 + np.abs(ref).max())
        if err > worst:
            worst, name = err, n
    return worst, name


_RUNS = {}


def run_case(case):
    """the case's two epochs, once per session: the device trains, the reference follows its recorded choices"""
    name, ds, B, K, num_neg, hyper, pseed, sseed = case
    if name not in _RUNS:
        d, m, st, order, ptr, col = make(case)
        assert m.batch_users == B
        m.record_choices(True)
        r = dict(comparisons=0, disagreements=0, bad=[], exhausted=0, beyond=0)
        for ep in range(wr.EPOCHS):
            stats = m.train_one_iteration(sseed, ep)
            assert stats.users == d.num_users
            o = wr.train(st, wr.Draws(ptr, col, d.num_items, num_neg, sseed, ep), B, choices=m.choices(), tol=wr.TOL)
            r["bad"] += [(ep,) + b for b in o["bad"]]
            r["comparisons"] += o["comparisons"]; r["disagreements"] += o["disagreements"]
            r["exhausted"] += o["exhausted"]; r["beyond"] += o["cnt65_499"]
            r["err"], r["which"] = max_err(m, st, order)
            print(f"{name} epoch {ep}: {o['comparisons']} comparisons, {o['disagreements']} disagreements, {len(o['bad'])} unverified, "
                  f"{o['exhausted']} exhausted, {o['cnt65_499']} beyond the first round, max |score| {o['max_abs_score']:.3g}, "
                  f"err {r['err']:.3g} ({r['which']})")
        r["biases"] = bool(m.get(cdae_amd.P_BP).any() or m.get(cdae_amd.P_UB).any())
        record_measured(f"warp_{name}", err=r["err"], comparisons=r["comparisons"], disagreements=r["disagreements"], unverified=len(r["bad"]))
        m.close()
        _RUNS[name] = r
    return _RUNS[name]


@pytest.mark.parametrize("case", wr.CASES, ids=[c[0] for c in wr.CASES])
def test_every_decision_of_the_trajectory_verifies(built, case):
    r = run_case(case)
    assert not r["bad"], (len(r["bad"]), r["bad"][:5])
    assert r["disagreements"] <= wr.NEAR_SHARE * r["comparisons"], (r["disagreements"], r["comparisons"])
    assert r["exhausted"] >= 1 and r["beyond"] >= 1       # the searches the device made are of the depths the CPU file promises
    assert not r["biases"]                                 # biases are part of no step


@pytest.mark.parametrize("case", wr.CASES, ids=[c[0] for c in wr.CASES])
def test_parameters_of_the_trajectory_agree(built, case):
    """2e-4 of the parameter's range after two epochs, the bound tests/test_gpu_mf.py holds IMF / BPR to."""
    r = run_case(case)
    assert r["err"] < 2e-4, (r["err"], r["which"])


def trained(case, record, epochs=wr.EPOCHS):
    d, m, *_ = make(case)
    if record is not None:
        m.record_choices(record)
    for ep in range(epochs):
        m.train_one_iteration(case[7], ep)
    out = [m.get(w).copy() for _, w in TABLES]
    m.close()
    return out


@pytest.mark.parametrize("case", [c for c in wr.CASES if c[0] in ("d40-loop-K65", "d40-block8")], ids=lambda c: c[0])
def test_recording_changes_no_bit_and_a_run_repeats_bit_for_bit(built, case):
    plain, again, recorded, switched_off = trained(case, None), trained(case, None), trained(case, True), trained(case, False)
    for a, b, c, e in zip(plain, again, recorded, switched_off):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(a, e)


def test_the_record_covers_the_users_a_call_trained(built):
    case = next(c for c in wr.CASES if c[0] == "d40-loop-K64")
    d, m, *_ = make(case)
    m.record_choices(True)
    item, cnt = m.choices()
    assert (item == wr.NONE).all() and (cnt == 0).all()                   # nothing trained yet
    m.train_users(case[7], 0, 2, 5)
    item, cnt = m.choices()
    lo, hi = int(d.train_ptr[2]) * 5, int(d.train_ptr[5]) * 5
    assert (cnt[lo:hi] >= 1).all() and (cnt[:lo] == 0).all() and (cnt[hi:] == 0).all()
    assert ((cnt[lo:hi] == wr.MAX_TRY) == (item[lo:hi] == wr.NONE)).all()
    m.close()


def test_a_warp_handle_is_served_like_an_imf_handle(built):
    """the same tables in a WARP handle and in an IMF handle: the same lists from recommend_all, the same neighbours from similar_items"""
    d = wr.fixture_data("tiny")
    rng = np.random.default_rng(4)
    K = 24
    w = cdae_amd.WARP(cdae_amd.WARPConfig(num_dim=K)); w.reset(d, seed=3)
    f = cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, batch_users=1)); f.reset(d, seed=3)
    tables = {cdae_amd.P_WU: rng.standard_normal((d.num_users, K)), cdae_amd.P_W: rng.standard_normal((d.num_items, K)),
              cdae_amd.P_UB: rng.standard_normal(d.num_users), cdae_amd.P_BP: rng.standard_normal(d.num_items)}
    for which, t in tables.items():
        w.set(which, t.astype(np.float32)); f.set(which, t.astype(np.float32))
        np.testing.assert_array_equal(w.get(which), t.astype(np.float32))
    for topk in (10, 20):
        np.testing.assert_array_equal(w.recommend_all(topk), f.recommend_all(topk))
    np.testing.assert_array_equal(w.recommend_all(10, 40, 90), f.recommend_all(10)[40:90])
    np.testing.assert_array_equal(w.similar_items(np.arange(30), topk=5), f.similar_items(np.arange(30), topk=5))
    w.set_test_rows(d.test_ptr, d.test_col); f.set_test_rows(d.test_ptr, d.test_col)
    np.testing.assert_array_equal(w.eval_topn(10)[0], f.eval_topn(10)[0])
    assert w.current_loss(1, 0) == 0.0
    w.close(); f.close()
