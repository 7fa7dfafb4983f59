"""Instances and users per second of the FISM loop over a window of users (ML-10M synthetic shape, K = 64 and K = 200, FISM's defaults),
measured three ways: (a) with the first rows of a visit resident on chip, as shipped; (b) with every row streaming through memory
(set_resident(False)); (c) tests/fism_ref.py's fp64 numpy loop on one core, over a sample of the same users.  A measurement, not a test:
nothing is asserted.

Every figure is the mean of `--runs` fresh runs from the same initial parameters, after one warm-up run, with the smallest and the largest
run beside it.  The window is short so that the loop (one workgroup) finishes in seconds; instances/s of a window extrapolates to an epoch
only as far as the later users look like the first.  Beside the rates: resident_rows per K, the share of the window's users whose whole row
is resident, and the share of its row steps (instances x rows) that touch a resident row.

    python tools/fism_bench.py [--users 64] [--ref-users 4] [--runs 5] [--out profiles/fism_measured.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cdae_amd  # noqa: E402
from cdae_amd import synth  # noqa: E402


def timed(m, n, runs):
    out = []
    for r in range(runs + 1):                             # run 0 warms up
        m.init_params(3)
        m.synchronize()
        t0 = time.perf_counter()
        m.train_users(5, 0, 0, n)
        m.synchronize()
        if r:
            out.append(time.perf_counter() - t0)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=64)
    ap.add_argument("--ref-users", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs="*", default=[64, 200])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = synth.generate_shape("ml10m", seed=1)
    n = a.users
    lens = np.diff(d.train_ptr)[:n].astype(np.int64)
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for K in a.dims:
        cfg = cdae_amd.FISMConfig(num_dim=K)
        m = cdae_amd.FISM(cfg)
        m.reset(d, seed=3)
        C = m.plan()["resident_rows"]
        inst = int(lens.sum()) * (1 + cfg.num_neg)
        emit(f"fism_bench num_dim={K} users={n} instances={inst} mean_row={lens.mean():.1f} max_row={lens.max()} resident_rows={C} "
             f"users_fully_resident={(lens <= C).mean():.3f} row_steps_resident={(lens * np.minimum(lens, C)).sum() / (lens * lens).sum():.3f}")
        for name, resident in (("resident", True), ("streaming", False)):
            m.set_resident(resident)
            t = timed(m, n, a.runs)
            emit(f"fism_bench num_dim={K} tier={name} runs={a.runs} seconds_mean={t.mean():.4f} seconds_min={t.min():.4f} seconds_max={t.max():.4f} "
                 f"instances_per_s={inst / t.mean():.5g} (min {inst / t.max():.5g}, max {inst / t.min():.5g}) users_per_s={n / t.mean():.5g}")
        m.close()
        if a.ref_users:
            import fism_ref as fr
            st = fr.init_state(d.num_items, d.num_users, K, 3, num_neg=cfg.num_neg)
            t0 = time.perf_counter()
            cnt = fr.train(st, d.train_ptr, d.train_col, 5, 0, users=(0, a.ref_users))
            dt = time.perf_counter() - t0
            emit(f"fism_bench num_dim={K} tier=numpy_fp64_one_core users={a.ref_users} instances={cnt} seconds={dt:.3f} instances_per_s={cnt / dt:.5g} "
                 f"users_per_s={a.ref_users / dt:.5g}")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
