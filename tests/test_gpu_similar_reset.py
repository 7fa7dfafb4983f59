"""-m gpu: a handle that has served similar_items is given new interactions with another item count and serves it again.

cdae_hip_similar_items keeps its device arrays (the queries, the table image, the +0.0 bias, the masks, the lists) in grow-only
workspaces of the handle, and cdae_hip_set_interactions frees them all.  A LARGER catalogue first (5 000 items), both metrics on both
top-k paths with an allow list and an excl CSR, then a SMALLER one (300 items) on the same handle: every array of the second round must
carry the bits a fresh handle returns that has only ever seen the second data set (tests/test_gpu_rows_reset.py, for this entry point).
"""
import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth
from test_gpu_rows_reset import BATCH, K, bits, csr, draw, start

pytestmark = pytest.mark.gpu


def serve(model, I, Q, n_allow, seed):
    rng = np.random.default_rng(seed)
    queries = rng.integers(0, I, Q).astype(np.uint32)
    eptr, ecol = csr([draw(rng, I, rng.integers(1, 11)) for _ in range(Q)])
    allow = draw(rng, I, n_allow)
    out = {}
    for metric in ("dot", "cosine"):
        for topk in (10, 32):                                        # the matrix cores; the general path (above REC_TOPK_MAX = 16)
            for name, kw in (("plain", {}), ("filtered", dict(exclude=(eptr, ecol), allow=allow)), ("own", dict(exclude_self=False))):
                ids, sc = model.similar_items(queries, topk, metric, with_scores=True, **kw)
                out[f"{metric}{topk}{name}_ids"], out[f"{metric}{topk}{name}_scores"] = ids, sc
    return out


def test_similar_items_after_a_second_set_interactions(built):
    big = synth.generate(64, 5000, 64 * 20, seed=11, min_items=5)
    small = synth.generate(40, 300, 40 * 20, seed=12, min_items=5)
    cfg = cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=BATCH, user_factor=True)
    model = cdae_amd.CDAE(cfg)
    start(model, big)
    first = serve(model, big.num_items, 48, 200, seed=21)
    assert all(a.size for a in first.values())
    start(model, small)
    got = serve(model, small.num_items, 12, 40, seed=22)
    fresh = cdae_amd.CDAE(cfg)
    start(fresh, small)
    want = serve(fresh, small.num_items, 12, 40, seed=22)
    assert got.keys() == want.keys()
    for name in want:
        assert got[name].shape == want[name].shape and np.array_equal(bits(got[name]), bits(want[name])), name
    model.close()
    fresh.close()
