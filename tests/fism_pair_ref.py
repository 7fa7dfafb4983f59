"""Test infrastructure: FISMauc (the pairwise FISM of include/cdae_hip.h's FISM-pair section) in numpy, fp64, written from that
description on top of tests/fism_ref.py: its State, _step, negatives, scale_table, hidden, measure and fixture_data are used as they are.

  train(st, ptr, col, seed, epoch, ...)   one epoch of the pair loop over users in id order (or a sub-range) -> the number of pairs
  grads(st, rows, i, j)                   the gradients one pair steps on, for the finite-difference check
  instance_loss(st, rows, i, j, loss_value)

train() takes `fault`, one of the three ways a kernel is likely to get the loop wrong (tests/test_fism_pair_reference.py shows that the
fixtures tell each from the right loop):
  "stale_positive"   Q[i] and bi[i] are read as they were at the start of the positive for all of its pairs
  "stale_repeat"     a negative that repeats inside a positive is read as it was before its first step of that positive
  "self_in_v"        v = x, with P[i] left inside
"""
import functools

import numpy as np

import fism_ref as fr
from fism_ref import State, _step, negatives, scale_table, hidden, measure, fixture_data, init_state, resident_rows, WAVES, WINDOW_INSTANCES  # noqa: F401
from warp_ref import loss_grad

TABLES = ("P", "Pa", "Q", "Qa", "bi")          # the five the GPU tests compare (a pair handle has no bu)
EPOCHS = fr.EPOCHS
DRIFT_MAX = fr.DRIFT_MAX
BOUND = fr.BOUND
PSEED = fr.PSEED
FAULTS = ("stale_positive", "stale_repeat", "self_in_v")


def train(st, ptr, col, seed, epoch, users=None, fault=None):
    """one epoch over users [0, U) (or the range `users`) in id order -> the number of pairs"""
    ptr = np.asarray(ptr, dtype=np.int64); col = np.asarray(col, dtype=np.int64)
    I = st.P.shape[0]
    dt = st.P.dtype.type
    first, end = users if users is not None else (0, ptr.size - 1)
    count = 0
    for u in range(first, end):
        rows = col[ptr[u]:ptr[u + 1]]
        n = rows.size
        if n == 0:
            continue
        neg = negatives(ptr, col, I, st.num_neg, seed, epoch, u)
        s = st.scale[n - 1]
        x = st.P[rows].sum(axis=0)
        for p in range(n):
            i = int(rows[p])
            idx = np.delete(rows, p)
            qi0, bi0 = st.Q[i].copy(), st.bi[i]
            seen = {}
            for k in range(st.num_neg):
                j = int(neg[p, k])
                v = x if fault == "self_in_v" else x - st.P[i]
                qi, bii = (qi0, bi0) if fault == "stale_positive" else (st.Q[i].copy(), st.bi[i])
                qj, bij = st.Q[j].copy(), st.bi[j]
                if fault == "stale_repeat":
                    qj, bij = seen.setdefault(j, (qj, bij))
                qd = qi - qj
                d = s * (v @ qd)
                if st.bias:
                    d = d + (bii - bij)
                st.max_abs_pred = max(st.max_abs_pred, abs(float(d)))
                fr._classify(st, float(d), True)
                g = dt(loss_grad(st.loss, d, dt(1.0)))
                if st.bias:
                    st.bi[i], st.bia[i] = _step(st, bii, st.bia[i], g + st.lam * bii)
                    st.bi[j], st.bia[j] = _step(st, bij, st.bia[j], -g + st.lam * bij)
                before = st.P[idx]
                after, st.Pa[idx] = _step(st, before, st.Pa[idx], (g * s) * qd[None, :] + st.lam * before)
                st.P[idx] = after
                st.Q[i], st.Qa[i] = _step(st, qi, st.Qa[i], (g * s) * v + st.lam * qi)
                st.Q[j], st.Qa[j] = _step(st, qj, st.Qa[j], -(g * s) * v + st.lam * qj)
                x = x + (after - before).sum(axis=0)
                count += 1
    return count


# ---- one pair as a function of the parameters: what the finite-difference check differentiates ----------------------------------------
def instance_loss(st, rows, i, j, loss_value):
    """loss(d, 1) + lambda / 2 (bi[i]^2 + bi[j]^2 + |Q[i]|^2 + |Q[j]|^2 + sum_{r != i} |P[r]|^2)"""
    rows = np.asarray(rows, dtype=np.int64)
    idx = rows[rows != i]
    s = st.scale[rows.size - 1]
    d = s * (st.P[idx].sum(axis=0) @ (st.Q[i] - st.Q[j])) + (st.bi[i] - st.bi[j] if st.bias else 0.0)
    reg = 0.5 * st.lam * ((st.P[idx] ** 2).sum() + (st.Q[i] ** 2).sum() + (st.Q[j] ** 2).sum() + (st.bi[i] ** 2 + st.bi[j] ** 2 if st.bias else 0.0))
    return loss_value(st.loss, d) + reg


def grads(st, rows, i, j):
    """the gradients train() steps on at this state: -> dict(idx, P=[len(idx), K] over idx, Qi=[K], Qj=[K], bi, bj)"""
    rows = np.asarray(rows, dtype=np.int64)
    idx = rows[rows != i]
    s = st.scale[rows.size - 1]
    v = st.P[rows].sum(axis=0) - st.P[i]
    qd = st.Q[i] - st.Q[j]
    d = s * (v @ qd) + (st.bi[i] - st.bi[j] if st.bias else 0.0)
    g = loss_grad(st.loss, d, 1.0)
    return dict(idx=idx, P=(g * s) * qd[None, :] + st.lam * st.P[idx], Qi=(g * s) * v + st.lam * st.Q[i], Qj=-(g * s) * v + st.lam * st.Q[j],
                bi=g + st.lam * st.bi[i], bj=-g + st.lam * st.bi[j])


# ---- the cases shared by tests/test_fism_pair_reference.py (their premises, on the CPU) and tests/test_gpu_fism_pair.py ----------------
# (name, data set, num_dim, num_neg, hyper-parameters beyond FISMPConfig's defaults, stream seed); the learn rate and the seed are chosen
# as fism_ref's are (the largest of 0.1, 0.03, 0.01 and the first seed of 1, 2, 3 with drift <= DRIFT_MAX): tools/fism_pair_cases.py is
# the search, and DRIFTS holds what it measured.
CASES = []
DRIFTS = {}


def _case(name, ds, K, nn, hyper, sseed, drift):
    CASES.append((name, ds, K, nn, hyper, sseed))
    DRIFTS[name] = drift


def case(name):
    return next(c for c in CASES if c[0] == name)


def new_state(c, dtype64=True):
    name, ds, K, nn, hyper, sseed = c
    d = fixture_data(ds)
    st = init_state(d.num_items, d.num_users, K, PSEED, num_neg=nn, **hyper)
    return st if dtype64 else st.as_float32()


def run(c, dtype64=True, fault=None):
    d = fixture_data(c[1])
    st = new_state(c, dtype64)
    for ep in range(EPOCHS):
        train(st, d.train_ptr, d.train_col, c[5], ep, fault=fault)
    return st


@functools.lru_cache(maxsize=None)
def reference(name):
    """the fp64 state after EPOCHS epochs of the case (computed once per session; do not modify)"""
    return run(case(name))


def run_free(c):
    """-> dict(max_abs_pred, drift): the largest |d| of the fp64 run and how far the same loop in float32 ends from it, the largest
    measure() over the five tables"""
    st = reference(c[0]) if c[0] in DRIFTS else run(c)
    st32 = run(c, dtype64=False)
    return dict(max_abs_pred=st.max_abs_pred, drift=max(measure(getattr(st32, n), getattr(st, n)) for n in TABLES))


@functools.lru_cache(maxsize=None)
def grid_reference(name):
    """the fp64 state after EPOCHS epochs of the pair loop from fism_ref's grid fixture (fism_ref.GRID_PAIR_CASES; computed once per
    session; do not modify)"""
    K, hyper = fr.GRID_PAIR_CASES[name]
    return fr.grid_run(train, K, hyper)


# CASES-BEGIN (written from tools/fism_pair_cases.py's output; the last number is the measured drift)
_case("d40-K1", "d40", 1, 5, {'alpha': 0.5}, 1, 1.17e-06)
_case("d40-K64", "d40", 64, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 2, 1.13e-05)
_case("d40-K65", "d40", 65, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 4.79e-06)
_case("d40-K128", "d40", 128, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 3, 4.60e-05)
_case("d40-K129", "d40", 129, 5, {'alpha': 0.5, 'learn_rate': 0.01}, 1, 3.30e-06)
_case("d40-K256", "d40", 256, 5, {'alpha': 0.5, 'learn_rate': 0.01}, 1, 2.88e-05)
_case("d40-K257", "d40", 257, 5, {'alpha': 0.5, 'learn_rate': 0.01}, 3, 3.82e-05)
_case("d40-K512", "d40", 512, 5, {'alpha': 0.5, 'learn_rate': 0.01}, 1, 3.95e-05)
_case("d40-sgd-K64", "d40", 64, 5, {'adagrad': False, 'alpha': 0.5}, 1, 6.78e-06)
_case("d40-sgd-K128", "d40", 128, 5, {'adagrad': False, 'alpha': 0.5}, 1, 5.47e-06)
_case("d40-sgd-K200", "d40", 200, 5, {'adagrad': False, 'alpha': 0.5}, 1, 5.26e-06)
_case("d40-sgd-K512", "d40", 512, 5, {'adagrad': False, 'alpha': 0.5}, 1, 4.77e-06)
_case("d40-log", "d40", 200, 5, {'loss': 2, 'alpha': 0.5}, 1, 4.75e-05)
_case("d40-nobias", "d40", 200, 5, {'bias': False, 'alpha': 0.5, 'learn_rate': 0.01}, 2, 1.73e-05)
_case("d40-alpha0", "d40", 64, 5, {'alpha': 0.0, 'learn_rate': 0.01}, 1, 3.63e-05)
_case("d40-alpha05", "d40", 200, 5, {'alpha': 0.5, 'learn_rate': 0.01}, 2, 4.44e-05)
_case("d40-alpha1", "d40", 200, 5, {'alpha': 1.0, 'learn_rate': 0.03}, 1, 2.61e-05)
_case("d40-neg1", "d40", 200, 1, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 1.92e-05)
_case("d12-neg12", "d12", 24, 12, {'alpha': 0.5}, 1, 1.71e-06)
_case("d12-neg64", "d12", 24, 64, {'alpha': 0.5}, 1, 1.03e-05)
_case("d12-neg65", "d12", 24, 65, {'alpha': 0.5}, 1, 2.14e-06)
_case("ones", "ones", 24, 5, {'alpha': 0.5}, 1, 9.53e-07)
_case("dense", "dense", 24, 5, {'alpha': 0.5}, 2, 2.57e-05)
_case("gaps-K24", "gaps", 24, 5, {'alpha': 0.5}, 1, 4.39e-05)
_case("gaps-K200", "gaps", 200, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 5.78e-06)
_case("win", "win", 64, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 2.77e-05)
_case("seam64", "seam64", 64, 5, {'alpha': 1.0, 'learn_rate': 0.03}, 1, 1.53e-05)
_case("seam256", "seam256", 256, 5, {'alpha': 1.0, 'learn_rate': 0.01}, 1, 1.12e-05)
_case("seam512", "seam512", 512, 5, {'alpha': 1.0, 'learn_rate': 0.01}, 1, 3.26e-05)
# CASES-END
