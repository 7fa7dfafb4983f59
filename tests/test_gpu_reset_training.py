"""-m gpu: one handle is given data sets in a row that switch every data-dependent device buffer on and off, and trains on each.

The training-side sibling of tests/test_gpu_rows_reset.py.  Many buffers of a handle double as flags — the 16-bit sort keys, the
bucket sort's cuts and cells, the late rows' bitmap and G columns, an item shard's whole-row positions, the test rows — and
cdae_hip_set_interactions drops them all through ONE list (cdae_hip.hip visit_data_set_bufs).  A buffer missing from that list would
leak, and its stale pointer would pick a code path for the next data set.  So: after every set_interactions the reused handle must
return, bit for bit, what a fresh handle returns that has only ever seen that data set.  Two fresh handles are compared first: a
family that is not reproducible from run to run shows up as that, not as a reset bug.

The shapes (synth.generate(U, I, nnz, seed=3, min_items=5), num_dim 32, num_neg 5, batch_users 256 — a handle has ONE batch size; the
plans were computed on the CPU with tests/plan_ref.py for it):

    dense (400, 200, 24000)    60 late rows, 60 hot rows, bucket sort with cells, 16-bit keys, sort_bits 8
    wide  (96, 70000, 2880)    no late or hot rows, the library sort on 32-bit keys, sort_bits 17
    small (40, 300, 800)       no late or hot rows, bucket sort with cells, sort_bits 9

in the order dense, wide, small, dense.  The full-output kind has shapes of its own (its matrices are dense in the items).
"""
import functools

import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth

pytestmark = pytest.mark.gpu

K, NEG, B = 32, 5, 256
CE = cdae_amd.CROSS_ENTROPY
SHAPES = {"dense": (400, 200, 24000), "wide": (96, 70000, 2880), "small": (40, 300, 800),
          "full_a": (200, 3000, 4000), "full_b": (64, 400, 1500)}
ORDER = ("dense", "wide", "small", "dense")


@functools.lru_cache(maxsize=None)
def data(shape):
    return synth.generate(*SHAPES[shape], seed=3, min_items=5)


def params(model):
    """every parameter this handle kind has"""
    out = {}
    for which in range(cdae_amd.P_COUNT):
        try:
            out[f"p{which}"] = model.get(which)
        except cdae_amd.CDAEError:
            pass
    assert out
    return out


def run_sampled(model, d):
    model.set_interactions(d.num_users, d.num_items, d.train_ptr, d.train_col)
    model.init_params(5)
    for ep in range(2):
        model.train_one_iteration(5, ep)
    out = params(model)
    out["top10"] = model.recommend_all(10)
    out["loss"] = np.array([model.data_loss(5, 0)], np.float64)
    return out


def run_wrmf(model, d):
    model.set_interactions(d.num_users, d.num_items, d.train_ptr, d.train_col)
    model.init_params(5)
    for _ in range(2):
        model.half_step(cdae_amd.ALS_USERS)
        model.half_step(cdae_amd.ALS_ITEMS)
    out = params(model)
    out["gram_users"], out["gram_items"] = model.gram(cdae_amd.ALS_USERS), model.gram(cdae_amd.ALS_ITEMS)
    out["top10"] = model.recommend_all(10)
    out["loss"] = np.array([model.data_loss(5, 0)], np.float64)
    return out


def run_multi(model, d):
    model.set_interactions(d.num_users, d.num_items, d.train_ptr, d.train_col)
    model.init_params(5)
    for ep in range(2):
        model.train_one_iteration(5, ep)
    out = params(model)
    out["top10"] = model.recommend_all(10)
    out["loss"] = np.array([model.current_loss(5, 0)], np.float64)
    return out


def cdae(**kw):
    return lambda: cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, num_neg=NEG, lt=CE, beta=1.0, batch_users=B, user_factor=True, **kw))


# kind -> (constructor, run, the data sets in order, {shape: (late rows?, fused launch?)} to confirm or None)
SAMPLED_PLAN = {"dense": (True, True), "wide": (False, False), "small": (False, False)}
KINDS = {
    "cdae": (cdae(), run_sampled, ORDER, SAMPLED_PLAN),
    "cdae_linear_function": (cdae(linear_function=True), run_sampled, ORDER, SAMPLED_PLAN),
    "full_output": (cdae(full_output=True), run_sampled, ("full_a", "full_b", "full_a"), None),
    "imf": (lambda: cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, num_neg=NEG, batch_users=1)), run_sampled, ORDER, None),
    "bpr": (lambda: cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, num_neg=NEG, batch_users=1, pairwise=True)), run_sampled, ORDER, None),
    "wrmf": (lambda: cdae_amd.WRMF(cdae_amd.WRMFConfig(num_dim=K)), run_wrmf, ORDER, None),
    "item_rows_2": (lambda: cdae_amd.MultiCDAE(cdae_amd.CDAEConfig(num_dim=K, num_neg=NEG, lt=CE, beta=1.0, batch_users=B, user_factor=True),
                                               [0, 0], item_rows=True), run_multi, ("dense", "small"), None),
}


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def differing(a, b):
    """names of the arrays that differ in shape or in any bit"""
    assert a.keys() == b.keys()
    return [n for n in a if a[n].shape != b[n].shape or not np.array_equal(bits(a[n]), bits(b[n]))]


_fresh = {}


def fresh(kind, shape):
    """what a handle returns that has only ever seen this data set: computed once, on two handles that must agree"""
    if (kind, shape) not in _fresh:
        make, run = KINDS[kind][:2]
        got = []
        for _ in range(2):
            m = make()
            got.append(run(m, data(shape)))
            m.close()
        assert differing(got[0], got[1]) == [], f"{kind} on {shape} is not reproducible from run to run"
        floats = [v for v in got[0].values() if v.dtype.kind == "f"]
        assert all(np.isfinite(v).all() for v in floats) and sum(bool(np.any(v)) for v in floats) >= 2      # (it did train)
        _fresh[kind, shape] = got[0]
    return _fresh[kind, shape]


@pytest.mark.parametrize("kind", list(KINDS))
def test_training_after_every_set_interactions(built, kind):
    make, run, order, plan = KINDS[kind]
    model = make()
    for step, shape in enumerate(order):
        got = run(model, data(shape))
        if plan:                                                 # the shape reaches what it is here for
            dp = model.decode_plan
            print(kind, shape, dp)
            assert (dp["late_rows"] > 0, dp["fused"]) == plan[shape], (shape, dp)
        assert differing(got, fresh(kind, shape)) == [], f"{kind}: data set {step} ({shape}) on the reused handle"
    model.close()


def test_test_rows_do_not_survive_set_interactions(built):
    """set_test_rows + eval_topn twice on one handle, with test rows of different sizes and a set_interactions in between: the new
    data set has no test rows until it is given some."""
    def start(m, d):
        m.set_interactions(d.num_users, d.num_items, d.train_ptr, d.train_col)
        m.init_params(5)
        m.train_one_iteration(5, 0)

    def evaluate(m, d):
        m.set_test_rows(d.test_ptr, d.test_col)
        rets, hits, ids = m.eval_topn(10, with_ids=True)
        return dict(rets=rets, hits=hits, ids=ids)

    big, small = data("dense"), data("small")
    assert big.test_col.size != small.test_col.size and small.test_col.size > 0
    model = cdae()()
    start(model, big)
    first = evaluate(model, big)
    start(model, small)
    with pytest.raises(cdae_amd.CDAEError, match="cdae_hip_set_test_rows first"):
        model.eval_topn(10)
    second = evaluate(model, small)
    for d, got in ((big, first), (small, second)):
        m = cdae()()
        start(m, d)
        assert differing(got, evaluate(m, d)) == []
        m.close()
    model.close()
