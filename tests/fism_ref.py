"""Test infrastructure: FISM in numpy, fp64 — the training loop and the served hidden row of include/cdae_hip.h's FISM section, written from
that description.  The project's streams (include/cdae_rng.h) are the ones tests/warp_ref.py restates; its functions are used as they are.

  init_state(I, U, K, seed, **hyper)      the state cdae_hip_init_params(seed) leaves
  train(st, ptr, col, seed, epoch, ...)   one epoch of the loop over users in id order (or a sub-range)
  negatives(...), candidates(...)         a user's drawn negatives, and the 32 candidates behind each of them
  hidden(st, rated)                     z of a rated set: n^-alpha * the sum of its rows of P
  grads(st, u, rows, item, rated)         the gradients one instance steps on, for the finite-difference check

A state holds P, Pa, Q, Qa [I, K], bi, bia [I], bu, bua [U] as float64 (or, for the drift measure, all float32) and the hyper-parameters.
"""
import functools

import numpy as np

from warp_ref import rng_key, rng_draw, sample_negatives, init_table, loss_grad, STREAM_NEGATIVE, NEG_MAX_TRY

P_W, P_V = 0, 2
WAVES = 8                        # FISM_WAVES (cdae_amd/csrc/cdae_fism_host.h)
RESIDENT_FLOATS = 64             # FISM_RESIDENT_FLOATS
RESIDENT_SLOTS = 32              # FISM_RESIDENT_SLOTS
WINDOW_INSTANCES = 2048          # FISM_WINDOW_INSTANCES


def resident_rows(K):
    """cdae_hip_fism_plan's resident_rows at num_dim K"""
    ni = 1 if K <= 64 else 2 if K <= 128 else 4 if K <= 256 else 8
    return WAVES * min(RESIDENT_FLOATS // ni, RESIDENT_SLOTS)


def scale_table(max_n, alpha, dtype=np.float64):
    """scale[n] = n^-alpha (fp64 pow, rounded once to fp32), scale[0] = 0"""
    s = np.zeros(max_n + 1, dtype=np.float64)
    s[1:] = np.power(np.arange(1, max_n + 1, dtype=np.float64), -float(alpha))
    return s.astype(np.float32).astype(dtype)


class State:
    def __init__(self, P, Q, U, *, lambda_=0.01, learn_rate=0.1, loss=0, adagrad=True, bias=True, alpha=1.0, num_neg=5, acc0=1e-4):
        I = P.shape[0]
        self.P, self.Q = np.array(P, dtype=np.float64), np.array(Q, dtype=np.float64)
        self.Pa, self.Qa = np.full(self.P.shape, np.float32(acc0), dtype=np.float64), np.full(self.Q.shape, np.float32(acc0), dtype=np.float64)
        self.bi, self.bia = np.zeros(I), np.full(I, np.float32(acc0), dtype=np.float64)
        self.bu, self.bua = np.zeros(U), np.full(U, np.float32(acc0), dtype=np.float64)
        self.lam, self.lr, self.loss, self.adagrad, self.bias, self.alpha, self.num_neg = lambda_, learn_rate, loss, adagrad, bias, alpha, num_neg
        self.scale = scale_table(I, alpha)
        self.max_abs_pred = 0.0
        self.classes = {}                # (positive label?, sign of the prediction) -> instances met beyond +-18 (_classify)

    TABLES = ("P", "Pa", "Q", "Qa", "bi", "bu")          # the six the GPU tests compare
    ALL = TABLES + ("bia", "bua", "scale")

    def as_float32(self):
        for n in self.ALL:
            setattr(self, n, getattr(self, n).astype(np.float32))
        self.lam, self.lr = np.float32(self.lam), np.float32(self.lr)
        return self


def init_state(I, U, K, seed, **hyper):
    """P and Q drawn as Random() * 0.001 with the keys of CDAE_P_W and CDAE_P_V, accumulators 1e-4, biases 0"""
    return State(init_table(I, K, P_W, seed, 0.001), init_table(I, K, P_V, seed, 0.001), U, **hyper)


def _step(st, w, a, grad):
    """one AdaGrad (no beta) or SGD step -> (new w, new a); nothing in place"""
    if st.adagrad:
        a = a + grad * grad
        return w - st.lr * grad / np.sqrt(a), a
    return w - st.lr * grad, a


def negatives(ptr, col, num_items, num_neg, seed, epoch, u):
    """neg[p][k]: cdae_sample_negative(key of user u, p * num_neg + k, row, n, num_items)"""
    row = np.asarray(col[ptr[u]:ptr[u + 1]], dtype=np.int64)
    rated = np.zeros((1, num_items), dtype=bool)
    rated[0, row] = True
    m = row.size * num_neg
    key = rng_key(seed, epoch, u, STREAM_NEGATIVE)
    return sample_negatives(np.full(m, key, dtype=np.uint64), np.arange(m, dtype=np.uint64), np.zeros(m, dtype=np.int64), rated,
                            num_items).reshape(row.size, num_neg)


def candidates(ptr, col, num_items, num_neg, seed, epoch, u):
    """cand[p][k][t]: the NEG_MAX_TRY candidates of draw p * num_neg + k of user u, none rejected yet (include/cdae_rng.h, in Python
    integers).  negatives() is the first of them the user has not rated, or the walk from the last when all are rated."""
    n = int(ptr[u + 1] - ptr[u])
    key = rng_key(seed, epoch, u, STREAM_NEGATIVE)
    return np.array([[[(rng_draw(key, (p * num_neg + k) * NEG_MAX_TRY + t) * num_items) >> 32 for t in range(NEG_MAX_TRY)]
                      for k in range(num_neg)] for p in range(n)], dtype=np.int64).reshape(n, num_neg, NEG_MAX_TRY)


def neg_label(loss):
    return -1.0 if loss in (2, 3) else 0.0


FAULTS = ("neg_label_0", "exp_sign", "clamp18", "no_bias", "no_s_in_row_step")


def _faulty_grad(fault, loss, pred, label):
    """loss_grad with one of FAULTS written into it: the exponent's argument with the other sign; SQUARE on a prediction clamped to +-18"""
    if fault == "exp_sign" and loss == 2:
        return -label / (1.0 + np.exp(-pred * label))
    if fault == "exp_sign" and loss == 5:
        return 1.0 / (1.0 + np.exp(pred)) - label
    if fault == "clamp18" and loss == 0:
        return loss_grad(loss, min(max(pred, -18.0), 18.0), label)
    return loss_grad(loss, pred, label)


def _classify(st, pred, positive):
    """counts the saturated instances a run meets: st.classes[(positive label?, sign of pred)] for |pred| > 18"""
    if abs(pred) > 18.0:
        key = (bool(positive), 1 if pred > 0 else -1)
        st.classes[key] = st.classes.get(key, 0) + 1


def train(st, ptr, col, seed, epoch, users=None, fault=None):
    """one epoch over users [0, U) (or the range `users`) in id order -> the number of instances.  fault: one of FAULTS, a way a kernel
    is likely to get a saturated instance wrong (tests/test_fism_reference.py shows that the grid fixture tells each from the right loop):
      "neg_label_0"        LOG's (and HINGE's) negative label taken as 0
      "exp_sign"           the sign of the exponent's argument flipped (LOG, CROSS_ENTROPY)
      "clamp18"            the prediction clamped to +-18 before SQUARE's gradient
      "no_bias"            bu + bi left out of the prediction
      "no_s_in_row_step"   the rows of P step on g Q[item] where the loop has g s Q[item]"""
    assert fault is None or fault in FAULTS, fault
    ptr = np.asarray(ptr, dtype=np.int64); col = np.asarray(col, dtype=np.int64)
    I = st.P.shape[0]
    dt = st.P.dtype.type
    first, end = users if users is not None else (0, ptr.size - 1)
    count = 0
    for u in range(first, end):
        rows = col[ptr[u]:ptr[u + 1]]
        n = rows.size
        neg = negatives(ptr, col, I, st.num_neg, seed, epoch, u)
        s_pos, s_neg = st.scale[n - 1], st.scale[n]
        x = st.P[rows].sum(axis=0)
        for p in range(n):
            i = int(rows[p])
            for k in range(st.num_neg + 1):
                rated = k == 0
                item = i if rated else int(neg[p, k - 1])
                s = s_pos if rated else s_neg
                label = dt(1.0 if rated else 0.0 if fault == "neg_label_0" else neg_label(st.loss))
                v = x - st.P[i] if rated else x
                pred = s * (v @ st.Q[item])
                if st.bias and fault != "no_bias":
                    pred = pred + (st.bu[u] + st.bi[item])
                st.max_abs_pred = max(st.max_abs_pred, abs(float(pred)))
                _classify(st, float(pred), rated)
                g = dt(_faulty_grad(fault, st.loss, pred, label))
                if st.bias:
                    st.bu[u], st.bua[u] = _step(st, st.bu[u], st.bua[u], g + st.lam * st.bu[u])
                    st.bi[item], st.bia[item] = _step(st, st.bi[item], st.bia[item], g + st.lam * st.bi[item])
                idx = np.delete(rows, p) if rated else rows
                q = st.Q[item].copy()
                before = st.P[idx]
                after, st.Pa[idx] = _step(st, before, st.Pa[idx], (g if fault == "no_s_in_row_step" else g * s) * q[None, :] + st.lam * before)
                st.P[idx] = after
                st.Q[item], st.Qa[item] = _step(st, q, st.Qa[item], (g * s) * v + st.lam * q)
                x = x + (after - before).sum(axis=0)
                count += 1
    return count


def hidden(st, rated):
    """z of a rated set (any iterable of item ids): scale[n] * the sum of its rows of P; 0 for an empty set"""
    rated = np.asarray(list(rated), dtype=np.int64)
    return st.scale[rated.size] * st.P[rated].sum(axis=0)


# ---- one instance as a function of the parameters: what the finite-difference check differentiates -----------------------------------
def instance_loss(st, u, rows, item, rated, loss_value):
    """loss(pred, label) + lambda / 2 (bu^2 + bi^2 + |Q[item]|^2 + sum_j |P[j]|^2 over the rows the instance steps)"""
    rows = np.asarray(rows, dtype=np.int64)
    n = rows.size
    s = st.scale[n - 1] if rated else st.scale[n]
    idx = rows[rows != item] if rated else rows
    v = st.P[idx].sum(axis=0)
    pred = s * (v @ st.Q[item]) + (st.bu[u] + st.bi[item] if st.bias else 0.0)
    label = 1.0 if rated else neg_label(st.loss)
    reg = 0.5 * st.lam * ((st.P[idx] ** 2).sum() + (st.Q[item] ** 2).sum() + (st.bu[u] ** 2 + st.bi[item] ** 2 if st.bias else 0.0))
    return loss_value(st.loss, pred, label) + reg


def grads(st, u, rows, item, rated):
    """the gradients train() steps on at this state: -> dict(P=[len(idx), K] over idx, idx, Q=[K], bu, bi)"""
    rows = np.asarray(rows, dtype=np.int64)
    n = rows.size
    s = st.scale[n - 1] if rated else st.scale[n]
    x = st.P[rows].sum(axis=0)
    v = x - st.P[item] if rated else x
    pred = s * (v @ st.Q[item]) + (st.bu[u] + st.bi[item] if st.bias else 0.0)
    g = loss_grad(st.loss, pred, 1.0 if rated else neg_label(st.loss))
    idx = rows[rows != item] if rated else rows
    return dict(idx=idx, P=(g * s) * st.Q[item][None, :] + st.lam * st.P[idx], Q=(g * s) * v + st.lam * st.Q[item],
                bu=g + st.lam * st.bu[u], bi=g + st.lam * st.bi[item])


# ---- fixtures shared by tests/test_fism_reference.py (their premises, on the CPU) and tests/test_gpu_fism.py (the trajectories) --------
def rows_data(lengths, num_items, seed=2):
    import mf_conflict_ref
    rng = np.random.default_rng(seed)
    return mf_conflict_ref.from_rows([np.sort(rng.choice(num_items, n, replace=False)) for n in lengths], num_items)


def seam_lengths(K):
    """rows of 1, 2, W - 1, W, W + 1, C - 1, C, C + 1 and 2C + 1 items: every edge of the residency plan at num_dim K"""
    C = resident_rows(K)
    return (1, 2, WAVES - 1, WAVES, WAVES + 1, C - 1, C, C + 1, 2 * C + 1)


GAPS_LENGTHS = (0, 3, 0, 0, 8, 5, 0, 9, 2, 7, 0)


@functools.lru_cache(maxsize=None)
def fixture_data(name):
    import mf_conflict_ref
    from cdae_amd import synth
    if name == "d40":
        return mf_conflict_ref.d40()
    if name == "d12":
        return mf_conflict_ref.d12()
    if name == "tiny":
        return synth.generate_shape("tiny", seed=5)
    if name == "ones":                   # rows of 1 and 2 items: s_pos = 0 and the empty neighbourhood of a lone positive
        return rows_data((1, 2, 1, 1, 2, 2, 1), 9)
    if name == "win":                    # 2 754 instances at num_neg 5: more than one launch window
        return rows_data((17, 9, 22, 14, 30, 11, 25, 19, 8, 27, 13, 21, 16, 29, 10, 24, 18, 12, 26, 15, 23, 20, 9, 11), 60)
    if name == "gaps":                   # users without train items: the first, the last, two in a row, one between trained users
        return rows_data(GAPS_LENGTHS, 12)
    if name == "dense":                  # two users have rated 11 of 12 items: draws whose 32 candidates are all rated take the walk
        return rows_data((11, 4, 0, 10, 1, 11), 12)
    if name.startswith("seam"):          # seam64 / seam256 / seam512
        K = int(name[4:])
        return rows_data(seam_lengths(K), 2 * resident_rows(K) + 200)
    raise KeyError(name)


EPOCHS = 2
DRIFT_MAX = 5e-5                 # float32 against float64 on the reference alone: a quarter of the GPU test's 2e-4
BOUND = 2e-4                     # the device against the fp64 reference (the IMF / BPR / WARP bound)
PSEED = 11
# (name, data set, num_dim, num_neg, hyper-parameters beyond FISMConfig's defaults, stream seed)
# AdaGrad without beta from accumulators of 1e-4 moves a young coordinate by the learn rate whatever the gradient, so at the default
# 0.1 a trajectory amplifies rounding until the same loop in float32 ends far from its float64 self (run_free's `drift`), and a
# bound of 2e-4 on the device would measure the trajectory, not the kernel.  Per case the learn rate is the largest of 0.1, 0.03, 0.01
# and the stream seed the first of 1, 2, 3, ... (at that rate) with drift <= DRIFT_MAX; tools/fism_cases.py is the search, and
# DRIFTS holds what it measured.  Short rows carry alpha = 0.5 (and the K = 200 cases each alpha), the seam cases alpha = 1.
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


def measure(a, b):
    """max |a - b| / (1e-3 + max |b|): the measure of every parameter bound here"""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (1e-3 + np.abs(b).max())) if b.size else 0.0


@functools.lru_cache(maxsize=None)
def reference(name):
    """the fp64 state after EPOCHS epochs of the case (computed once per session; do not modify)"""
    c = case(name)
    d = fixture_data(c[1])
    st = new_state(c)
    for ep in range(EPOCHS):
        train(st, d.train_ptr, d.train_col, c[5], ep)
    return st


def run_free(c):
    """-> dict(max_abs_pred, drift): the largest |pred| of the fp64 run and how far the same loop in float32 ends from it, the largest
    measure() over the six tables — what rounding alone does to this trajectory, whatever the kernel"""
    d = fixture_data(c[1])
    st = reference(c[0]) if c[0] in DRIFTS else None
    if st is None:
        st = new_state(c)
        for ep in range(EPOCHS):
            train(st, d.train_ptr, d.train_col, c[5], ep)
    st32 = new_state(c, dtype64=False)
    for ep in range(EPOCHS):
        train(st32, d.train_ptr, d.train_col, c[5], ep)
    return dict(max_abs_pred=st.max_abs_pred, drift=max(measure(getattr(st32, n), getattr(st, n)) for n in State.TABLES))


# ---- the grid fixture: predictions on the +-18 / +-88 / +-1000 grid of tests/golden/saturation_kat.npz -------------------------------------
# tests/test_gpu_model_saturation.py trains FISM and FISMauc from it; tests/test_fism_reference.py and tests/test_fism_pair_reference.py
# assert its premises on the CPU.  Modelled on tests/test_gpu_saturation.py::test_mf_from_grid_scores:
#   53 users and 100 items; user u's row is item u and four of the items 53 .. 99 (five items: three of the eight wavefronts own no row);
#   rows 53 .. 99 of P are 0.25 e_0, rows 0 .. 52 carry 0 in coordinate 0 and N(0, 0.1) elsewhere; coordinate 0 of Q is 2 grid[i] for
#   i < 53 and 0 beyond, the other coordinates N(0, 0.1); alpha = 0.5, so s_pos = scale[4] = 0.5 exactly; biases 0.
# For user u's rated item u then x = P[u] + e_0 and v = x - P[u] = e_0 in every arithmetic (each coordinate is one value plus zeros), so
# s_pos v . Q[u] = 0.5 * 2 grid[u] = grid[u] bit for bit; a drawn negative j < 53 scores about 5^-0.5 * 2 grid[j], saturated as well.
GRID_BOUND = 1e-3                # the device against fp64, element by element: |gpu - ref| <= GRID_BOUND * (GRID_FLOOR + |ref|)
GRID_FLOOR = 1e-2                # (test_mf_from_grid_scores' MF_BOUND and FLOOR: fp32 storage, __expf, 1-ulp rcp and sqrt against fp64)
GRID_DRIFT_MAX = GRID_BOUND / 4  # float32 against float64 on the reference alone, in the same measure
GRID_SSEED = 2                   # the first stream seed of 1, 2, 3, ... at which every case below meets GRID_DRIFT_MAX and all four classes
GRID_HYPER = dict(alpha=0.5, lambda_=0.01, learn_rate=2.0 ** -5)
GRID_SGD = dict(adagrad=False, learn_rate=2.0 ** -10)
# name -> (num_dim, hyper-parameters beyond GRID_HYPER); num_neg is 5.  SQUARE with plain SGD is left out: on the full grid its fp64
# reference overflows by itself (a step of lr * 2 * 1000 * 2000 on a row whose prediction it multiplies), at 2^-10 and at 2^-20 alike.
GRID_CASES = {
    "sq-ada": (16, dict(loss=0)),
    "log-ada": (16, dict(loss=2)),
    "ce-ada": (16, dict(loss=5)),
    "log-sgd": (16, dict(loss=2, **GRID_SGD)),
    "ce-sgd": (16, dict(loss=5, **GRID_SGD)),
    "log-ada-K300": (300, dict(loss=2)),                       # NI = 8
    "log-ada-nobias": (16, dict(loss=2, bias=False)),
}
GRID_PAIR_CASES = {
    "sq-ada": (16, dict(loss=0)),
    "log-ada": (16, dict(loss=2)),
    "log-sgd": (16, dict(loss=2, **GRID_SGD)),
    "log-ada-K300": (300, dict(loss=2)),
    "log-ada-nobias": (16, dict(loss=2, bias=False)),
}


@functools.lru_cache(maxsize=None)
def grid():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "saturation_kat.npz"))["grid"].astype(np.float32)


@functools.lru_cache(maxsize=None)
def grid_data():
    """53 users: user u's first (smallest) item is item u, then four of the items 53 .. 99"""
    import mf_conflict_ref
    rng = np.random.default_rng(3)
    n = grid().size
    return mf_conflict_ref.from_rows([np.r_[u, np.sort(rng.choice(np.arange(n, n + 47), 4, replace=False))] for u in range(n)], n + 47)


def grid_tables(K):
    """-> (P, Q) float32 [100, K]"""
    g = grid()
    n, I = g.size, g.size + 47
    rng = np.random.default_rng(5)
    P = rng.normal(0.0, 0.1, (I, K)); Q = rng.normal(0.0, 0.1, (I, K))
    P[:, 0] = 0.0; P[n:] = 0.0; P[n:, 0] = 0.25
    Q[:, 0] = 0.0; Q[:n, 0] = 2.0 * g.astype(np.float64)
    return P.astype(np.float32), Q.astype(np.float32)


def grid_state(K, hyper, dtype64=True, tables=None):
    """the state a grid case starts from (tables: (P, Q) read back from a handle; default grid_tables(K))"""
    d = grid_data()
    P, Q = tables if tables is not None else grid_tables(K)
    st = State(P, Q, d.num_users, num_neg=5, **{**GRID_HYPER, **hyper})
    return st if dtype64 else st.as_float32()


def grid_first(st):
    """the prediction of every user's first instance (FISM), the score of the positive of every user's first pair (FISMauc), in the
    state's own arithmetic: s_pos (x - P[u]) . Q[u] + bi[u] (+ bu[u], zero at the start)"""
    d = grid_data()
    out = []
    for u in range(d.num_users):
        rows = d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]].astype(np.int64)
        assert rows[0] == u and rows.size == 5 < WAVES
        v = st.P[rows].sum(axis=0) - st.P[u]
        out.append(st.scale[rows.size - 1] * (v @ st.Q[u]) + (st.bu[u] + st.bi[u]))
    return np.array(out)


def share_beyond(x, t):
    return float(np.mean(np.abs(np.asarray(x)) > t))


def grid_measure(a, b):
    """max over the elements of |a - b| / (GRID_FLOOR + |b|): a range that includes 2000 would hide the small entries"""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / (GRID_FLOOR + np.abs(b))).max())


def grid_run(train_fn, K, hyper, dtype64=True, fault=None, tables=None):
    """EPOCHS epochs of train_fn (this module's train or fism_pair_ref's) from the grid start -> the state; every table finite after
    every epoch"""
    d = grid_data()
    st = grid_state(K, hyper, dtype64, tables)
    for ep in range(EPOCHS):
        with np.errstate(over="ignore"):                       # exp of a saturated prediction overflows to inf and 1 / inf is 0: meant
            train_fn(st, d.train_ptr, d.train_col, GRID_SSEED, ep, **({"fault": fault} if fault else {}))
        for n in State.ALL:
            assert np.isfinite(getattr(st, n)).all(), (n, ep)
    return st


@functools.lru_cache(maxsize=None)
def grid_reference(name):
    """the fp64 state after EPOCHS epochs of the FISM grid case (computed once per session; do not modify)"""
    K, hyper = GRID_CASES[name]
    return grid_run(train, K, hyper)


# CASES-BEGIN (written from tools/fism_cases.py's output; the last number is the measured drift)
_case("d40-K1", "d40", 1, 5, {'alpha': 0.5}, 1, 7.79e-07)
_case("d40-K64", "d40", 64, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 1.45e-05)
_case("d40-K65", "d40", 65, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 2.69e-05)
_case("d40-K128", "d40", 128, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 7.31e-06)
_case("d40-K129", "d40", 129, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 6.61e-06)
_case("d40-K256", "d40", 256, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 8.49e-06)
_case("d40-K257", "d40", 257, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 1.49e-05)
_case("d40-K512", "d40", 512, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 2.31e-05)
_case("d40-sgd", "d40", 200, 5, {'adagrad': False, 'alpha': 0.5}, 1, 5.29e-07)
_case("d40-ce", "d40", 200, 5, {'loss': 5, 'alpha': 0.5}, 1, 2.76e-05)
_case("d40-log", "d40", 200, 5, {'loss': 2, 'alpha': 0.5}, 1, 2.13e-05)
_case("d40-neg1", "d40", 200, 1, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 5.27e-06)
_case("d40-neg12", "d40", 200, 12, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 2.09e-05)
_case("d40-nobias", "d40", 200, 5, {'bias': False, 'alpha': 0.5, 'learn_rate': 0.03}, 1, 6.02e-06)
_case("d40-alpha0", "d40", 200, 5, {'alpha': 0.0, 'learn_rate': 0.01}, 1, 3.42e-05)
_case("d40-alpha05", "d40", 200, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 6.96e-06)
_case("d40-alpha1", "d40", 200, 5, {'alpha': 1.0}, 1, 2.95e-05)
_case("ones", "ones", 24, 5, {'alpha': 0.5}, 1, 1.09e-05)
_case("d12-neg12", "d12", 24, 12, {'alpha': 0.5}, 1, 2.94e-05)
_case("win", "win", 64, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 2.30e-05)
_case("seam64", "seam64", 64, 5, {'alpha': 1.0, 'learn_rate': 0.03}, 1, 4.89e-06)
_case("seam256", "seam256", 256, 5, {'alpha': 1.0, 'learn_rate': 0.03}, 1, 2.63e-06)
_case("seam512", "seam512", 512, 5, {'alpha': 1.0, 'learn_rate': 0.03}, 1, 1.45e-06)
_case("gaps-K24", "gaps", 24, 5, {'alpha': 0.5}, 1, 1.05e-05)
_case("gaps-K200", "gaps", 200, 5, {'alpha': 0.5, 'learn_rate': 0.03}, 1, 2.07e-05)
_case("dense", "dense", 24, 5, {'alpha': 0.5}, 1, 4.88e-06)
_case("d12-neg64", "d12", 24, 64, {'alpha': 0.5}, 1, 3.36e-05)
_case("d12-neg65", "d12", 24, 65, {'alpha': 0.5}, 1, 3.96e-05)
_case("d12-neg130", "d12", 24, 130, {'alpha': 0.5, 'learn_rate': 0.03}, 2, 3.68e-05)
_case("d40-neg65", "d40", 200, 65, {'alpha': 0.5, 'learn_rate': 0.01}, 2, 4.88e-05)
_case("d40-sgd-K64", "d40", 64, 5, {'adagrad': False, 'alpha': 0.5}, 1, 7.36e-07)
_case("d40-sgd-K128", "d40", 128, 5, {'adagrad': False, 'alpha': 0.5}, 1, 7.03e-07)
_case("d40-sgd-K512", "d40", 512, 5, {'adagrad': False, 'alpha': 0.5}, 1, 7.65e-07)
_case("d40-nobias-K64", "d40", 64, 5, {'bias': False, 'alpha': 0.5, 'learn_rate': 0.03}, 1, 7.47e-06)
_case("d40-nobias-K512", "d40", 512, 5, {'bias': False, 'alpha': 0.5, 'learn_rate': 0.03}, 1, 1.30e-05)
# CASES-END
