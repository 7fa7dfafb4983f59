"""Users per second of a WARP epoch beside a BPR handle at the same settings (ML-10M synthetic shape, K = 200, WARP's defaults), for the
reference loop (batch_users = 1) and for blocks of 8 users.  A measurement, not a test: nothing is asserted.

A WARP step costs what its search costs, and that depends on the state: from the initial parameters nearly every first draw violates
the margin; once a user's positives are separated a search runs tens to hundreds of draws.  So each range of users is timed twice —
its first visit (epoch 0) and its second (epoch 1) — and both are printed.  The ranges are short so that the loop (one wavefront)
finishes in seconds; users/s of a range extrapolates to an epoch only as far as the later users look like the first.

    python tools/warp_bench.py [--loop-users 256] [--block-users 2048] [--out profiles/warp_measured.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cdae_amd  # noqa: E402
from cdae_amd import synth  # noqa: E402


def timed(m, seed, epoch, n):
    m.synchronize()
    t0 = time.perf_counter()
    m.train_users(seed, epoch, 0, n)
    m.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-users", type=int, default=256)
    ap.add_argument("--block-users", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = synth.generate_shape("ml10m", seed=1)
    lines = []
    for B, n in ((1, a.loop_users), (8, a.block_users)):
        models = {
            "WARP": cdae_amd.WARP(cdae_amd.WARPConfig(num_dim=200, batch_users=B)),
            "BPR": cdae_amd.MF(cdae_amd.MFConfig(num_dim=200, pairwise=True, lt=cdae_amd.HINGE, lambda_=0.1, learn_rate=0.1, beta=0.0,
                                                 using_bias_term=False, batch_users=B)),
        }
        for name, m in models.items():
            m.reset(d, seed=3)
            first, second = timed(m, 5, 0, n), timed(m, 5, 1, n)
            lines.append(f"warp_bench model={name} batch_users={B} users={n} num_dim=200 users_per_s_first_visit={first:.5g} "
                         f"users_per_s_second_visit={second:.5g}")
            print(lines[-1], flush=True)
            m.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
