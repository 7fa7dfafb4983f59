#!/usr/bin/env python
"""Developer aid: wall time of cdae_hip_set_interactions on ONE handle, the flagship configuration of bench.py (sampled decode, K = 200,
the library's batch size) at a synthetic shape.  The first call fills a fresh handle; every later one frees the data set before it and
allocates the next, which is what a change to the handle's buffer ownership moves.  One JSON line: every call in ms, the median of the
repeats after the first.  A/B against another build of the same ABI: CDAE_HIP_LIBRARY=<that .so>.

    python tools/set_interactions_bench.py [--shape ml10m] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cdae_amd  # noqa: E402
from cdae_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml10m")
    ap.add_argument("--num-dim", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    d = synth.generate_shape(a.shape)
    m = cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=a.num_dim, lt=cdae_amd.CROSS_ENTROPY, num_neg=5, beta=1.0, user_factor=True))
    ms = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        m.set_interactions(d.num_users, d.num_items, d.train_ptr, d.train_col)
        ms.append(1e3 * (time.perf_counter() - t0))
    m.close()
    print(json.dumps({"shape": a.shape, "first_ms": round(ms[0], 3), "repeat_ms": [round(x, 3) for x in ms[1:]],
                      "median_repeat_ms": round(float(np.median(ms[1:])), 3)}))


if __name__ == "__main__":
    main()
