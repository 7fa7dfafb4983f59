#!/usr/bin/env python
"""Times cdae_hip_train_epoch of a WRMF handle (two half-steps) at the ML-10M synthetic shape, K = 200, cg_steps = 3.

    python tools/als_bench.py                    one process: 2 warm-up epochs, then 5 timed ones -> one JSON line with their median
    python tools/als_bench.py --processes 3      three fresh processes one after the other -> the median of their medians
    python tools/als_bench.py --processes 3 --parity FILE --out profiles/als_measured.txt
                                                 ... and the report: the timed epoch with its two floors, and the worst half-step
                                                 parity error per K tier from FILE (what tests/test_gpu_als.py appends to the file
                                                 named by CDAE_ALS_MEASURED)
    python tools/als_bench.py --weighted         the same process also times the epoch with per-pair confidence weights (geometric(0.3) play
                                                 counts through cdae_hip_als_set_confidence: one 4-byte load more per interaction and product)
                                                 and one cdae_hip_als_objective call -> "weighted_*" and "objective_seconds" in the JSON line
The two floors the time can be read against, both from the shapes (estimates, not measurements):
  matrix work   4 (U + I) 2 Kp^2 flops per half-step pair — (cg_steps + 1) = 4 products G p per row of either side, 2 Kp^2 flops each —
                at the fp32 matrix rate;
  G traffic     every block of 32 rows reads G (Kp^2 floats) once per product: 4 ceil(rows / 32) Kp^2 4 B per side, from L2.
Nothing is asserted: there is no earlier number to hold this one against."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MATRIX_TFLOPS = 157.3       # MI355X, fp32 matrix (vendor figure)
L2_TBPS = 10.0                   # order of magnitude of the aggregate L2 bandwidth: the traffic floor is a reading aid


def one_process(a):
    import cdae_amd
    from cdae_amd import synth
    d = synth.generate_shape(a.shape, seed=5)
    m = cdae_amd.WRMF(cdae_amd.WRMFConfig(lambda_=1.0, scalar=40.0, num_dim=a.num_dim, cg_steps=a.cg_steps))
    m.reset(d, seed=11)
    for _ in range(a.warmup):
        m.train_one_iteration()
    t = [m.train_one_iteration().wall_seconds for _ in range(a.epochs)]
    Kp = int(m.lib.cdae_hip_row_stride(m.h))
    out = {"shape": a.shape, "users": d.num_users, "items": d.num_items, "nnz": int(d.train_ptr[-1]), "num_dim": a.num_dim,
           "row_stride": Kp, "cg_steps": a.cg_steps, "epoch_seconds": t, "median_epoch_seconds": statistics.median(t)}
    if a.weighted:
        import time
        import numpy as np
        m.set_confidence(np.random.default_rng(7).geometric(0.3, int(d.train_ptr[-1])).astype(np.float32))
        for _ in range(a.warmup):
            m.train_one_iteration()
        tw = [m.train_one_iteration().wall_seconds for _ in range(a.epochs)]
        m.objective()                                         # (the second Gram buffer and the per-row terms are allocated here)
        to = []
        for _ in range(a.epochs):
            t0 = time.perf_counter()
            m.objective()
            to.append(time.perf_counter() - t0)
        out.update({"weighted_epoch_seconds": tw, "weighted_median_epoch_seconds": statistics.median(tw),
                    "objective_seconds": to, "median_objective_seconds": statistics.median(to)})
    print(json.dumps(out))


def parity_lines(path):
    worst = {}
    for line in open(path):
        fx, side, K, steps, e = line.split()
        key = (int(K), int(steps))
        worst[key] = max(worst.get(key, 0.0), float(e))
    out = ["worst single half-step error against the fp64 restatement, max |a - b| / max(1, row max |b|), over both fixtures and both sides",
           "(tests/test_gpu_als.py::test_single_half_step_parity; asserted below 2e-4)", "    K  cg_steps=1  cg_steps=3"]
    for K in sorted({k for k, _ in worst}):
        out.append(f"{K:5d}  {worst.get((K, 1), float('nan')):.3e}   {worst.get((K, 3), float('nan')):.3e}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml10m")
    ap.add_argument("--num-dim", type=int, default=200)
    ap.add_argument("--cg-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--processes", type=int, default=0, help="0: measure in this process; N: N fresh processes, one after the other")
    ap.add_argument("--weighted", action="store_true", help="also time the weighted epoch and one objective call")
    ap.add_argument("--parity", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.processes == 0:
        one_process(a)
        return
    runs = []
    for _ in range(a.processes):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", a.shape, "--num-dim", str(a.num_dim), "--cg-steps", str(a.cg_steps),
                              "--warmup", str(a.warmup), "--epochs", str(a.epochs)] + (["--weighted"] if a.weighted else []), check=True, capture_output=True, text=True, timeout=600).stdout
        runs.append(json.loads(out.strip().splitlines()[-1]))
    r = runs[0]
    U, I, Kp, prods = r["users"], r["items"], r["row_stride"], r["cg_steps"] + 1
    med = statistics.median(x["median_epoch_seconds"] for x in runs)
    flops = prods * (U + I) * 2 * Kp * Kp
    traffic = prods * (-(-U // 32) + -(-I // 32)) * Kp * Kp * 4
    lines = [f"WRMF / ALS, cdae_hip_train_epoch (user half-step + item half-step), {r['shape']} synthetic shape: {U} users x {I} items, "
             f"{r['nnz']} interactions, K = {r['num_dim']} (row stride {Kp}), cg_steps = {r['cg_steps']}",
             f"{a.processes} fresh processes, each {a.warmup} warm-up epochs then {a.epochs} timed ones; per-process medians (s): "
             + ", ".join(f"{x['median_epoch_seconds']:.4f}" for x in runs),
             f"median epoch: {med * 1e3:.2f} ms",
             f"floor, matrix work: {prods} (U + I) 2 Kp^2 = {flops / 1e9:.1f} GFLOP -> {flops / (FP32_MATRIX_TFLOPS * 1e12) * 1e3:.3f} ms at {FP32_MATRIX_TFLOPS} TFLOP/s fp32 matrix",
             f"floor, G traffic: {prods} ceil(rows / 32) Kp^2 4 B over both sides = {traffic / 1e9:.2f} GB from L2 -> {traffic / (L2_TBPS * 1e12) * 1e3:.3f} ms at ~{L2_TBPS:.0f} TB/s",
             "(both floors are estimates from the shapes; the sparse part — one wavefront dot product and axpy per interaction and product — is on neither)"]
    if a.weighted:
        wmed = statistics.median(x["weighted_median_epoch_seconds"] for x in runs)
        omed = statistics.median(x["median_objective_seconds"] for x in runs)
        lines += [f"with per-pair confidence weights (geometric(0.3) play counts), same processes; per-process medians (s): "
                  + ", ".join(f"{x['weighted_median_epoch_seconds']:.4f}" for x in runs),
                  f"median weighted epoch: {wmed * 1e3:.2f} ms ({(wmed / med - 1) * 100:+.1f} % against the binary epoch)",
                  f"one cdae_hip_als_objective call (host wall clock, weighted handle): {omed * 1e3:.2f} ms"]
    if a.parity:
        lines += [""] + parity_lines(a.parity)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
