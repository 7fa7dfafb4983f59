#!/usr/bin/env python
"""Wall-clock of full_rank_rows next to recommend_rows(topk=10) over the same rows, in one process.

ML-10M shape (synth, K = 200): every user's train row as the rated set, the test split as the targets.  full_rank_rows is two sweeps
of the catalogue plus the counting by construction, so what it is recorded against is the one sweep of recommend_rows on the same
rows, not a fixed time.  Both calls end in a device synchronise and return their results to the host; the two are warmed up, then
timed alternately, and the medians are reported.

    python tools/full_rank_bench.py [--shape ml10m] [--dim 200] [--repeats 9] [--out profiles/full_rank_ml10m.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import cdae_amd  # noqa: E402
from cdae_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml10m")
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join("profiles", "full_rank_ml10m.txt"))
    a = ap.parse_args()
    d = synth.generate_shape(a.shape)
    m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=a.dim, lt=cdae_amd.CROSS_ENTROPY, beta=1.0, batch_users=512))
    m.set_interactions(d.num_users, d.num_items, d.train_ptr, d.train_col)
    m.init_params(1)
    m.train_one_iteration(1, 0)
    uids = np.arange(d.num_users, dtype=np.uint32)
    # the test split as targets; an item that is also in the user's train row (the synthetic split may repeat one) is not a target
    keep = np.ones(d.test_col.size, dtype=bool)
    for u in range(d.num_users):
        t0, t1 = d.test_ptr[u], d.test_ptr[u + 1]
        if t1 > t0:
            keep[t0:t1] = ~np.isin(d.test_col[t0:t1], d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]])
    row = np.repeat(np.arange(d.num_users), np.diff(d.test_ptr))[keep]
    tptr = np.r_[0, np.cumsum(np.bincount(row, minlength=d.num_users))].astype(np.int64)
    tcol = d.test_col[keep]

    def full_rank():
        return m.full_rank_rows(d.train_ptr, d.train_col, tptr, tcol, uids)

    def top10():
        return m.recommend_rows(d.train_ptr, d.train_col, uids, 10)
    for _ in range(2):
        ranks, ids = full_rank(), top10()
    t_rank, t_top = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter(); full_rank(); t1 = time.perf_counter(); top10(); t2 = time.perf_counter()
        t_rank.append(t1 - t0); t_top.append(t2 - t1)
    rank_s, top_s = float(np.median(t_rank)), float(np.median(t_top))
    # the two answers agree: a target the top-10 list holds has its place as rank
    at = {(int(r), int(c)): int(k) for r, c, k in zip(row, tcol, ranks) if k < 10}
    assert at and all(int(ids[r, k]) == c for (r, c), k in at.items())
    met = cdae_amd.ranking_metrics(tptr, ranks, d.num_items - np.diff(d.train_ptr))
    windows = int(((np.diff(tptr) + 15) // 16).sum())
    lines = [f"shape {a.shape}: {d.num_users} users x {d.num_items} items, num_dim {a.dim}, {tcol.size} targets in {int((np.diff(tptr) > 0).sum())} rows "
             f"({windows} columns of the counting launches)",
             f"full_rank_rows          median {rank_s * 1e3:10.2f} ms   (min {min(t_rank) * 1e3:.2f}, max {max(t_rank) * 1e3:.2f}, {a.repeats} calls)",
             f"recommend_rows(topk=10) median {top_s * 1e3:10.2f} ms   (min {min(t_top) * 1e3:.2f}, max {max(t_top) * 1e3:.2f}, {a.repeats} calls)",
             f"ratio full_rank_rows / recommend_rows = {rank_s / top_s:.2f}",
             f"recall@10 {met['recall@10']:.4f}  recall@100 {met['recall@100']:.4f}  ndcg@100 {met['ndcg@100']:.4f}  mrr {met['mrr']:.4f}  auc {met['auc']:.4f}"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
