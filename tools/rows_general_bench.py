#!/usr/bin/env python
"""Wall-clock of recommend_rows on the general path (topk = 32, above the matrix cores' 16) at the shape of
tests/test_gpu_rows_filtered.py::test_timing_of_a_category_page_is_recorded: 4 096 rows of 1-60 items, 20 000 items, K = 200.
Median of nine calls after a warm one, each ending in a device synchronise.

    python tools/rows_general_bench.py
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cdae_amd
from cdae_amd import synth
U, I, K, R, topk = 512, 20_000, 200, 4096, 32
d = synth.generate(U, I, U * 30, seed=4, min_items=5)
m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=64))
m.reset(d, seed=3)
m.train_one_iteration(3, 0)
rng = np.random.default_rng(9)
rows = [np.sort(rng.choice(I, int(rng.integers(1, 61)), replace=False)).astype(np.uint32) for _ in range(R)]
ptr, col = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64), np.concatenate(rows)
uids = rng.integers(0, U, R).astype(np.uint32)
m.recommend_rows(ptr, col, uids, topk)
times = []
for _ in range(9):
    m.synchronize(); t0 = time.perf_counter(); m.recommend_rows(ptr, col, uids, topk); m.synchronize(); times.append(time.perf_counter() - t0)
print(f"recommend_rows(topk={topk}) general path: median {1e3 * np.median(times):.3f} ms  (min {1e3 * min(times):.3f}, max {1e3 * max(times):.3f}, {len(times)} calls)")
