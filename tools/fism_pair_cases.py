#!/usr/bin/env python
"""The search behind tests/fism_pair_ref.py's CASES, as tools/fism_cases.py is for FISM: per case the largest learn rate of 0.1, 0.03,
0.01 and, at that rate, the first stream seed of 1, 2, 3 at which the float32 run of the pair reference ends within DRIFT_MAX of its
float64 self (fism_pair_ref.run_free).  CPU only.  Prints one `_case(...)` line per case, to be pasted between the CASES markers of
tests/fism_pair_ref.py.

    python tools/fism_pair_cases.py [name ...]
"""
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import fism_pair_ref  # noqa: E402

A = dict(alpha=0.5)
SPECS = [(f"d40-K{K}", "d40", K, 5, A) for K in (1, 64, 65, 128, 129, 256, 257, 512)] + [
    (f"d40-sgd-K{K}", "d40", K, 5, dict(adagrad=False, alpha=0.5)) for K in (64, 128, 200, 512)] + [
    ("d40-log", "d40", 200, 5, dict(loss=2, alpha=0.5)),
    ("d40-nobias", "d40", 200, 5, dict(bias=False, alpha=0.5)),
    ("d40-alpha0", "d40", 64, 5, dict(alpha=0.0)),     # (at K = 200 no rate and seed of this search meets the premise: 3.0e-4 at best)
    ("d40-alpha05", "d40", 200, 5, dict(alpha=0.5)),
    ("d40-alpha1", "d40", 200, 5, dict(alpha=1.0)),
    ("d40-neg1", "d40", 200, 1, A),
    ("d12-neg12", "d12", 24, 12, A),
    ("d12-neg64", "d12", 24, 64, A),
    ("d12-neg65", "d12", 24, 65, A),
    ("ones", "ones", 24, 5, A),
    ("dense", "dense", 24, 5, A),
    ("gaps-K24", "gaps", 24, 5, A),
    ("gaps-K200", "gaps", 200, 5, A),
    ("win", "win", 64, 5, A),
    ("seam64", "seam64", 64, 5, dict(alpha=1.0)),
    ("seam256", "seam256", 256, 5, dict(alpha=1.0)),
    ("seam512", "seam512", 512, 5, dict(alpha=1.0)),
]
RATES = (0.1, 0.03, 0.01)
SEEDS = (1, 2, 3)


def search(spec):
    name, ds, K, nn, hyper = spec
    tried = []
    for lr in RATES:
        h = dict(hyper) if lr == 0.1 else dict(hyper, learn_rate=lr)
        for seed in SEEDS:
            r = fism_pair_ref.run_free((name, ds, K, nn, h, seed))
            tried.append((lr, seed, r["drift"]))
            if r["drift"] <= fism_pair_ref.DRIFT_MAX:
                return f'_case("{name}", "{ds}", {K}, {nn}, {h!r}, {seed}, {r["drift"]:.2e})    # max |d| {r["max_abs_pred"]:.3g}', tried
    return f"# {name}: no (learn rate, seed) meets the premise", tried


if __name__ == "__main__":
    specs = [s for s in SPECS if not sys.argv[1:] or s[0] in sys.argv[1:]]
    with multiprocessing.Pool(min(len(specs), 12)) as pool:
        for line, tried in pool.imap(search, specs):
            print(line, flush=True)
            print("#   tried (learn rate, seed, drift):", ", ".join(f"({a}, {b}, {c:.1e})" for a, b, c in tried), flush=True)
