"""Seconds of the FISMauc loop (cdae_amd.FISMP) over a window of users, beside the existing FISM loop at the same shape: ML-10M synthetic
shape and one short-row shape (synth "yelp"), K = 64 and K = 200, num_neg 5, the defaults otherwise, each with the first rows of a visit
resident on chip (as shipped) and with every row streaming through memory (set_resident(False)).  A measurement, not a test: nothing is
asserted.

Method: every (shape, K) is measured in `--rounds` FRESH processes, one after the other; inside a process the four loops (FISM resident,
FISM streaming, FISMP resident, FISMP streaming) run interleaved, `--runs` times each after one warm-up each, every run from the same
initial parameters.  A figure is the MEDIAN over all runs of all processes, with the smallest and the largest beside it.  The window is
short so that a loop (one workgroup) finishes in well under a second; seconds of a window extrapolate to an epoch only as far as the
later users look like the first.  The parent stops at the first child that fails.

    python tools/fism_pair_bench.py [--rounds 3] [--runs 3] [--out profiles/fism_pair_measured.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SHAPES = {"ml10m": 64, "yelp": 256}          # shape -> users of the window (the first ones)
LOOPS = (("fism", True), ("fism", False), ("fismp", True), ("fismp", False))


def child(path, K, runs):
    import cdae_amd
    from cdae_amd import synth
    z = np.load(path)
    n = int(z["ptr"].size - 1)
    d = synth.Interactions(n, int(z["num_items"]), z["ptr"], z["col"], np.zeros(n + 1, np.int64), np.empty(0, np.uint32))
    models = {"fism": cdae_amd.FISM(cdae_amd.FISMConfig(num_dim=K)), "fismp": cdae_amd.FISMP(cdae_amd.FISMPConfig(num_dim=K))}
    for m in models.values():
        m.reset(d, seed=3)
    out = {f"{name}-{'resident' if res else 'streaming'}": [] for name, res in LOOPS}
    resident_rows = models["fismp"].plan()["resident_rows"]          # (before any loop switches residency off)
    examples = {}
    for r in range(runs + 1):                             # run 0 warms up
        for name, res in LOOPS:
            m = models[name]
            m.set_resident(res)
            m.init_params(3)
            m.synchronize()
            t0 = time.perf_counter()
            st = m.train_users(5, 0, 0, n)
            m.synchronize()
            if r:
                out[f"{name}-{'resident' if res else 'streaming'}"].append(time.perf_counter() - t0)
            examples[name] = int(st.examples)
    print(json.dumps(dict(seconds=out, examples=examples, resident_rows=resident_rows)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dims", type=int, nargs="*", default=[64, 200])
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.runs)
    from cdae_amd import synth
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        for shape, n in SHAPES.items():
            d = synth.generate_shape(shape, seed=1)
            end = int(d.train_ptr[n])
            files[shape] = os.path.join(tmp, shape + ".npz")
            np.savez(files[shape], ptr=d.train_ptr[:n + 1], col=d.train_col[:end], num_items=d.num_items)
            lens = np.diff(d.train_ptr[:n + 1])
            emit(f"fism_pair_bench shape={shape} users={n} nnz={end} mean_row={lens.mean():.1f} max_row={lens.max()} num_items={d.num_items}")
        got = {}
        for rnd in range(a.rounds):                       # fresh processes, the configurations in turn
            for shape in SHAPES:
                for K in a.dims:
                    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", files[shape], str(K), "--runs", str(a.runs)],
                                         capture_output=True, text=True, timeout=300)
                    if run.returncode != 0:
                        sys.stderr.write(run.stdout + run.stderr)
                        raise SystemExit(f"fism_pair_bench: the child for {shape} K={K} failed ({run.returncode}); nothing more is started")
                    r = json.loads(run.stdout.strip().splitlines()[-1])
                    g = got.setdefault((shape, K), dict(seconds={}, examples=r["examples"], resident_rows=r["resident_rows"]))
                    for k, v in r["seconds"].items():
                        g["seconds"].setdefault(k, []).extend(v)
    for (shape, K), g in got.items():
        med = {k: float(np.median(v)) for k, v in g["seconds"].items()}
        for k, v in g["seconds"].items():
            name = k.split("-")[0]
            emit(f"fism_pair_bench shape={shape} num_dim={K} loop={k} samples={len(v)} seconds_median={med[k]:.4f} seconds_min={min(v):.4f} "
                 f"seconds_max={max(v):.4f} examples={g['examples'][name]} us_per_example={1e6 * med[k] / g['examples'][name]:.2f}")
        emit(f"fism_pair_bench shape={shape} num_dim={K} resident_rows={g['resident_rows']} "
             f"fismp_over_fism_resident={med['fismp-resident'] / med['fism-resident']:.3f} "
             f"fismp_over_fism_streaming={med['fismp-streaming'] / med['fism-streaming']:.3f} "
             f"residency_gain_fism={med['fism-streaming'] / med['fism-resident']:.3f} "
             f"residency_gain_fismp={med['fismp-streaming'] / med['fismp-resident']:.3f}")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
