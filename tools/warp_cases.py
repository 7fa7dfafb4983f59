#!/usr/bin/env python
"""The search behind the stream seeds of tests/warp_ref.py's CASES: per case the first stream seed of 1, 2, 3, ... at which the
free-running fp64 reference meets every premise tests/test_warp_reference.py asserts (warp_ref.unmet: every search depth, near-ties
below NEAR_SHARE, float32 drift at most DRIFT_MAX, |score| at most SCORE_MAX — or, for a case marked `saturated`, trained pairs with
yui - score below -18 and below -88.5 — and what the case's data set adds).  CPU only.
Prints one line per case: the seed to write into the case's last field, and what the seeds before it missed.

    python tools/warp_cases.py [name ...]        (default: every case whose stream seed is 0, "not chosen yet")
"""
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import warp_ref  # noqa: E402

SEEDS = range(1, 200)


def search(case):
    tried = []
    for seed in SEEDS:
        c = case[:7] + (seed,)
        missed = warp_ref.unmet(c, warp_ref.run_free(c))
        if not missed:
            return f"{case[0]}: stream seed {seed}", tried
        tried.append((seed, missed))
    return f"# {case[0]}: no stream seed of {SEEDS} meets the premises", tried


if __name__ == "__main__":
    cases = [c for c in warp_ref.CASES if (c[0] in sys.argv[1:] if sys.argv[1:] else c[7] == 0)]
    with multiprocessing.Pool(min(len(cases), 12)) as pool:
        for line, tried in pool.imap(search, cases):
            print(line, flush=True)
            for seed, missed in tried:
                print(f"#   seed {seed}: " + "; ".join(missed), flush=True)
