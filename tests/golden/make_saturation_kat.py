#!/usr/bin/env python
"""Generates tests/golden/saturation_kat.npz (run from the repo root: python tests/golden/make_saturation_kat.py).

Plain fp64 closed forms, in numpy, of the formulas the model switches between at fixed magnitudes: the CROSS_ENTROPY loss at a
score of +-18, the sigmoid at a hidden pre-activation of +-18 and tanh at +-9, the LOG loss at z = pred * truth = +-18, HINGE at
z = 1.  Nothing here calls the oracle or the HIP library: tests/test_golden.py checks the oracle against this file, and
tests/test_gpu_saturation.py the device.

Every grid point is an fp32 value (stored as fp64), so a device that reads the point as a float sees exactly the value the columns
were computed from.  The grid crosses every switch and every fp32 overflow edge of the device's branch-free forms:
  0, +-1; +-8.99, +-9, +-9.01, +-17.99, +-18, +-18.01 and the fp32 neighbours of each; +-30; +-44.5 (exp(-2x) overflows fp32:
  the tanh form (1 - r) / (1 + r) is inf / inf there); +-87.3 (e^-x reaches the fp32 denormals); +-88.72 (expf overflows);
  +-89, +-100, +-1000.
Columns (pred = grid):
  sq_eval_t{0,1}, sq_grad_t{0,1}, ce_eval_t{0,1}, ce_grad_t{0,1}    evaluate / gradient for truth 0 and 1
  sigmoid, tanh                                                      the hidden activations of the pre-activation `grid`
  log_grad_tp1, log_grad_tm1                                         LOG gradient for truth +1 / -1 (IMF / BPR labels)
  hinge_pred, hinge_truth, hinge_grad                                HINGE gradient at z = 1 - ulp, 1, 1 + ulp for truth +-1
"""
import os

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def grid():
    f32 = np.float32
    pts = [0.0, 1.0]
    for v in (8.99, 9.0, 9.01, 17.99, 18.0, 18.01):
        x = f32(v)
        pts += [float(np.nextafter(x, f32(0))), float(x), float(np.nextafter(x, f32(np.inf)))]
    pts += [30.0, 44.5, 87.3, 88.72, 89.0, 100.0, 1000.0]
    pts = [float(f32(p)) for p in pts]
    g = np.array(sorted(set(pts) | {-p for p in pts}), dtype=np.float64)
    assert np.array_equal(g, g.astype(np.float32).astype(np.float64))
    return g


def sq_eval(p, t):
    return (t - p) ** 2


def sq_grad(p, t):
    return -2.0 * (t - p)


def ce_eval(p, t):
    ret = (1.0 - t) * p
    if p > 18:
        return ret + np.exp(-p)
    if p < -18:
        return ret - p
    return ret + np.log1p(np.exp(-p))


def ce_grad(p, t):
    if p < -18:
        return np.exp(p) - t
    if p > 18:
        return 1.0 - t
    return 1.0 / (1.0 + np.exp(-p)) - t


def sigmoid(x):
    if x > 18.0:
        return 1.0
    if x < -18.0:
        return 0.0
    return 1.0 / (1.0 + np.exp(-x))


def tanh(x):
    if x > 9.0:
        return 1.0
    if x < -9.0:
        return -1.0
    r = np.exp(-2.0 * x)
    return (1.0 - r) / (1.0 + r)


def log_grad(p, t):
    z = p * t
    if z > 18:
        return -t * np.exp(-z)
    if z < -18:
        return -t
    return -t / (1.0 + np.exp(z))


def hinge_grad(p, t):
    return 0.0 if p * t > 1 else -t


def main():
    g = grid()
    out = {"grid": g}
    for t in (0, 1):
        out[f"sq_eval_t{t}"] = np.array([sq_eval(p, float(t)) for p in g])
        out[f"sq_grad_t{t}"] = np.array([sq_grad(p, float(t)) for p in g])
        out[f"ce_eval_t{t}"] = np.array([ce_eval(p, float(t)) for p in g])
        out[f"ce_grad_t{t}"] = np.array([ce_grad(p, float(t)) for p in g])
    out["sigmoid"] = np.array([sigmoid(x) for x in g])
    out["tanh"] = np.array([tanh(x) for x in g])
    out["log_grad_tp1"] = np.array([log_grad(p, 1.0) for p in g])
    out["log_grad_tm1"] = np.array([log_grad(p, -1.0) for p in g])
    one = np.float32(1)
    z = np.array([np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2))], dtype=np.float64)
    out["hinge_pred"] = np.concatenate([z, -z])
    out["hinge_truth"] = np.array([1.0] * 3 + [-1.0] * 3)
    out["hinge_grad"] = np.array([hinge_grad(p, t) for p, t in zip(out["hinge_pred"], out["hinge_truth"])])
    assert all(np.isfinite(v).all() for v in out.values())
    np.savez(os.path.join(OUT, "saturation_kat.npz"), **out)
    print(f"saturation_kat.npz: {g.size} grid points")


if __name__ == "__main__":
    main()
