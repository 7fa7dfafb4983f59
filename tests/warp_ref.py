"""Test infrastructure: WARP in numpy, fp64 — the search and the training loop of include/cdae_hip.h's WARP section, written from that
description and from include/cdae_rng.h (whose mixer is restated here twice: in Python integers, literally, and on numpy uint64 arrays
for whole batches of draws; tests/test_warp_reference.py holds the two against each other).

  Draws(ptr, col, num_items, num_neg, seed, epoch)   the candidate lists of every pair of a data set whose rows are in POSITION order
                                                     (uid_offset: the handle's user_id_offset, added to the position in the key)
  search(state, draws, pos, p, k)                    the literal search -> (item, cnt, margin)
  train(state, draws, B, ...)                        one epoch: B = 1 the loop, B > 1 the block schedule; with `choices` it follows the
                                                     device's decisions and verifies each one within `tol`; with `wrong` it is the loop
                                                     with ONE step done wrong (WRONG), the yardstick of the parameter bound's sensitivity
  max_err(tables, state)                             the measure of the GPU test's parameter bound

A state holds uv, uva [U, K] BY POSITION, iv, iva [I, K], ib [I] as float64 and the hyper-parameters.
"""
import numpy as np

MAX_TRY = 500                    # CDAE_WARP_MAX_TRY
LOOK = MAX_TRY - 1               # draws that can train a pair
NONE = 0xFFFFFFFF
NEG_MAX_TRY = 32                 # CDAE_NEG_MAX_TRY
STREAM_NEGATIVE = 1
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


# ---- include/cdae_rng.h in Python integers ------------------------------------------------------------------------------------------
def mix64(x):
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def rng_key(seed, epoch, uid, stream):
    x = mix64((seed + GOLDEN * (epoch + 1)) & M64)
    return mix64(x ^ ((uid * 0xD1B54A32D192ED03 + stream + 1) & M64))


def rng_draw(key, idx):
    return mix64((key + GOLDEN * (idx + 1)) & M64) >> 32


def sample_negative(key, draw_index, row, num_items):
    """cdae_sample_negative: `row` any container of the user's positives"""
    row = set(int(i) for i in row)
    cand = 0
    for t in range(NEG_MAX_TRY):
        cand = (rng_draw(key, draw_index * NEG_MAX_TRY + t) * num_items) >> 32
        if cand not in row:
            return cand
    for _ in range(num_items):
        cand = 0 if cand + 1 == num_items else cand + 1
        if cand not in row:
            return cand
    return cand


def draw_index(p, num_neg, k, t):
    return (p * num_neg + k) * MAX_TRY + t


# ---- the same on uint64 arrays ------------------------------------------------------------------------------------------------------
def _u(x):
    return np.uint64(x)


def _mix64_v(x):
    x = x ^ (x >> _u(30)); x = x * _u(0xBF58476D1CE4E5B9)
    x = x ^ (x >> _u(27)); x = x * _u(0x94D049BB133111EB)
    return x ^ (x >> _u(31))


def sample_negatives(keys, draw_idx, urow, rated, num_items):
    """cdae_sample_negative for arrays: keys[n], draw_idx[n] uint64, urow[n] the row of `rated` [U, I] bool each draw is rejected against"""
    keys = np.asarray(keys, dtype=np.uint64); draw_idx = np.asarray(draw_idx, dtype=np.uint64); urow = np.asarray(urow, dtype=np.int64)
    out = np.zeros(keys.size, dtype=np.int64)
    todo = np.arange(keys.size)
    for t in range(NEG_MAX_TRY):
        if todo.size == 0:
            return out
        idx = draw_idx[todo] * _u(NEG_MAX_TRY) + _u(t)
        r = _mix64_v(keys[todo] + _u(GOLDEN) * (idx + _u(1))) >> _u(32)
        cand = ((r * _u(num_items)) >> _u(32)).astype(np.int64)
        out[todo] = cand
        todo = todo[rated[urow[todo], cand]]
    for _ in range(num_items):                     # the deterministic walk behind 32 rejected draws
        if todo.size == 0:
            break
        cand = out[todo] + 1
        cand[cand == num_items] = 0
        out[todo] = cand
        todo = todo[rated[urow[todo], cand]]
    return out


class Draws:
    """The candidates of every pair (position, p, k) of one (data set, num_neg, seed, epoch): they do not depend on the parameters.
    The first HEAD of every pair are drawn at once; a longer list is drawn when a search asks for it."""
    HEAD = 16

    def __init__(self, ptr, col, num_items, num_neg, seed, epoch, uid_offset=0):
        self.ptr = np.asarray(ptr, dtype=np.int64); self.col = np.asarray(col, dtype=np.int64)
        self.U, self.I, self.num_neg = self.ptr.size - 1, int(num_items), int(num_neg)
        self.rated = np.zeros((self.U, self.I), dtype=bool)
        lens = np.diff(self.ptr)
        self.user_of = np.repeat(np.arange(self.U), lens)                     # position of every stored interaction
        self.rated[self.user_of, self.col] = True
        self.keys = np.array([rng_key(seed, epoch, u + uid_offset, STREAM_NEGATIVE) for u in range(self.U)], dtype=np.uint64)    # (cdae_hip_set_user_id_offset)
        self.p_of = np.arange(self.col.size) - self.ptr[self.user_of]         # index of the interaction in its row
        n_pairs = self.col.size * self.num_neg
        r = np.arange(n_pairs) // self.num_neg
        self.pair_user = self.user_of[r]
        self.pair_base = ((self.p_of[r] * self.num_neg + np.arange(n_pairs) % self.num_neg) * MAX_TRY).astype(np.uint64)
        t = np.arange(self.HEAD, dtype=np.uint64)
        self.head = sample_negatives(np.repeat(self.keys[self.pair_user], self.HEAD), (self.pair_base[:, None] + t[None, :]).ravel(),
                                     np.repeat(self.pair_user, self.HEAD), self.rated, self.I).reshape(n_pairs, self.HEAD)
        self.full = {}

    def q(self, pos, p, k):
        return (int(self.ptr[pos]) + p) * self.num_neg + k

    def candidates(self, q, need):
        if need <= self.HEAD:
            return self.head[q, :need]
        if q not in self.full:
            u = self.pair_user[q]
            t = np.arange(LOOK, dtype=np.uint64)
            self.full[q] = sample_negatives(np.full(LOOK, self.keys[u]), self.pair_base[q] + t, np.full(LOOK, u), self.rated, self.I)
        return self.full[q][:need]


# ---- the model ----------------------------------------------------------------------------------------------------------------------
class State:
    def __init__(self, uv, uva, iv, iva, ib, *, lambda_=0.1, learn_rate=0.1, loss=3, adagrad=True, acc0=None, ib0=None,
                 saturated=None):   # (acc0, ib0: init_state's; saturated: unmet()'s)
        self.uv, self.uva, self.iv, self.iva = (np.array(a, dtype=np.float64) for a in (uv, uva, iv, iva))
        self.ib = np.array(ib, dtype=np.float64)
        self.lam2, self.lr, self.loss, self.adagrad = 2.0 * lambda_, learn_rate, loss, adagrad
        # rounded once to fp32, as the device's table of num_items entries (one more here: what "items-left-all" reads at cnt = 1)
        self.l = np.cumsum(1.0 / np.arange(1, self.iv.shape[0] + 2)).astype(np.float32).astype(np.float64)


def loss_grad(loss, pred, truth=1.0):
    """mf_loss_grad (cdae_mf_kernels.hpp) in fp64: SQUARE 0, LOGISTIC 1, LOG 2, HINGE 3, CROSS_ENTROPY 5"""
    if loss == 0: return -2.0 * (truth - pred)
    if loss == 1: return (pred - truth) / (pred * (1.0 - pred))
    if loss == 2: return -truth / (1.0 + np.exp(pred * truth))
    if loss == 3: return 0.0 if pred * truth > 1.0 else -truth
    return 1.0 / (1.0 + np.exp(-pred)) - truth


def _step(st, w, a, grad):
    """one AdaGrad (no beta) or SGD step of the vector w with accumulator a, in place"""
    if st.adagrad:
        a += grad * grad
        w -= st.lr * grad / np.sqrt(a)
    else:
        w -= st.lr * grad


def _margins(st, uv, iv, cands, thr):
    return st.ib[cands] + iv[cands] @ uv - thr


def _first_violator(st, uv, iv, draws, q, thr, stats):
    """the free search: -> (cnt, margins of the candidates looked at); cnt == MAX_TRY: exhausted"""
    done = 0
    parts = []
    for need in (draws.HEAD, 64, LOOK):
        c = draws.candidates(q, need)[done:]
        m = _margins(st, uv, iv, c, thr)
        parts.append(m)
        hit = np.nonzero(m > 0.0)[0]
        if hit.size:
            parts[-1] = m[:hit[0] + 1]
            return done + int(hit[0]) + 1, np.concatenate(parts)
        done = need
    return MAX_TRY, np.concatenate(parts)


def search(st, draws, pos, p, k):
    """-> (item, cnt, margin): the first candidate t < 499 with s(j) > s(i) - 1, cnt = t + 1; (NONE, 500, 0.0) when there is none"""
    i = draws.col[draws.ptr[pos] + p]
    thr = st.ib[i] + st.iv[i] @ st.uv[pos] - 1.0
    q = draws.q(pos, p, k)
    cnt, m = _first_violator(st, st.uv[pos], st.iv, draws, q, thr, None)
    if cnt >= MAX_TRY:
        return NONE, MAX_TRY, 0.0
    return int(draws.candidates(q, cnt)[cnt - 1]), cnt, float(m[cnt - 1])


# The loop with one step done wrong: what train(wrong=...) can be asked for.  Each name is ONE `if` at the place the loop differs; the
# subtleties are the ones the comments of the reference's warp.hpp and of cdae_warp_kernels.hpp turn on.
WRONG = (
    "yui-fresh",                 # yui recomputed before every pair (it is taken once per positive and is stale between its pairs)
    "post-step-uv",              # iv_i and iv_j stepped with the user vector AFTER its step (all three step from pre-step values)
    "lambda-once",               # lambda where the loop has 2 * lambda
    "rank-minus-one",            # H_idx where the loop has H_{idx + 1} (H_0 = 0)
    "items-left-all",            # items_left = num_items (it is num_items - n_u)
    "stale-positive-row",        # in place: iv_i at the step is the positive's first load, not the row as it is now
    "stale-repeated-negative",   # in place: a j that repeats inside a user sees the row from before its earlier step
    "phase-I-reversed",          # block schedule: an item row takes its pairs' steps in reverse order
    "bias-blind",                # ib left out of yui (the search's candidates keep theirs)
)


def train(st, draws, B=1, choices=None, tol=1e-3, positions=None, wrong=None):
    """One epoch over the positions 0 .. U - 1 (or the range `positions`) in blocks of B (a block of one user is the loop).  choices = (item, cnt) by
    (row offset * num_neg + k) in position order: the decisions to FOLLOW; each is verified —
      every candidate before cnt has margin <= +tol, the chosen one has margin > -tol, a skipped pair has no candidate with margin > +tol
      among the first 499 — and `bad` lists the ones that fail.
    wrong: one of WRONG.
    -> dict: comparisons, near (|margin| < tol), disagreements (followed decision != the free one), bad, and what the searches looked like:
    cnt1, cnt2_64, cnt65_499, exhausted, trained, max_abs_score, mixed_blocks (blocks with both a skipped and a trained pair); what the
    steps looked like: rank0, rank1, rank2 (trained pairs of users with one or two items left, by their rank weight l[0], l[1], l[2]),
    positives_twice (positives with two trained pairs), negatives_twice (trained pairs whose j the same user has stepped before),
    rows_twice (item rows with two steps in one block's phase I), one_user_blocks (blocks of one user under B > 1: they run in place),
    pred_lt18, pred_lt88 (trained pairs whose yui - score, what the loss sees, lies below -18 and below -88.5);
    and record = (item, cnt) of the decisions taken, indexed as `choices`."""
    assert wrong is None or wrong in WRONG, wrong
    out = dict(comparisons=0, near=0, disagreements=0, bad=[], cnt1=0, cnt2_64=0, cnt65_499=0, exhausted=0, trained=0, max_abs_score=0.0,
               mixed_blocks=0, rank0=0, rank1=0, rank2=0, positives_twice=0, negatives_twice=0, rows_twice=0, one_user_blocks=0, pred_lt18=0, pred_lt88=0,
               record=(np.full(draws.col.size * draws.num_neg, NONE, dtype=np.uint32), np.zeros(draws.col.size * draws.num_neg, dtype=np.uint32)))
    U, nn = draws.U, draws.num_neg
    lam2 = st.lam2 / 2.0 if wrong == "lambda-once" else st.lam2

    def decide(uv, iv, pos, p, k, yui):
        """-> (j, cnt, s(j)) of the decision taken; cnt == MAX_TRY: skipped"""
        q, thr = draws.q(pos, p, k), yui - 1.0
        if choices is None:
            cnt, m = _first_violator(st, uv, iv, draws, q, thr, out)
        else:
            cnt = int(choices[1][q])
            look = LOOK if cnt >= MAX_TRY else max(cnt, 1)
            c = draws.candidates(q, look)
            m = _margins(st, uv, iv, c, thr)
            free = np.nonzero(m > 0.0)[0]
            free_cnt = int(free[0]) + 1 if free.size else MAX_TRY
            if cnt >= MAX_TRY:
                ok = int(choices[0][q]) == NONE and not (m > tol).any()
            else:
                ok = 1 <= cnt <= LOOK and int(choices[0][q]) == int(c[cnt - 1]) and not (m[:cnt - 1] > tol).any() and m[cnt - 1] > -tol
            out["disagreements"] += free_cnt != cnt
            if not ok:                                   # (reported; the epoch goes on with the free decision)
                out["bad"].append((pos, p, k, int(choices[0][q]), cnt, free_cnt))
                cnt, m = _first_violator(st, uv, iv, draws, q, thr, out)
        out["comparisons"] += m.size
        out["near"] += int((np.abs(m) < tol).sum())
        out["max_abs_score"] = max(out["max_abs_score"], float(np.abs(m + thr).max()), abs(yui))
        key = "exhausted" if cnt >= MAX_TRY else "cnt1" if cnt == 1 else "cnt2_64" if cnt <= 64 else "cnt65_499"
        out[key] += 1
        out["record"][1][q] = cnt
        if cnt >= MAX_TRY:
            return None, cnt, 0.0
        out["trained"] += 1
        out["record"][0][q] = j = int(draws.candidates(q, cnt)[cnt - 1])
        return j, cnt, float(m[cnt - 1] + thr)

    first, end = positions if positions is not None else (0, U)
    for s0 in range(first, end, B):
        nb = min(B, end - s0)
        in_place = nb == 1
        out["one_user_blocks"] += in_place and B > 1
        iv0 = st.iv if in_place else st.iv.copy()       # the block schedule reads the item rows as the block found them
        records = []
        skipped = trained = 0
        for pos in range(s0, s0 + nb):
            row = draws.col[draws.ptr[pos]:draws.ptr[pos + 1]]
            items_left = draws.I if wrong == "items-left-all" else draws.I - row.size
            uv, ua = st.uv[pos], st.uva[pos]
            before = {}                                  # j -> iv_j as it was before this user's last step of it
            for p, i in enumerate(row):
                first_load = iv0[i].copy()
                yui = (0.0 if wrong == "bias-blind" else st.ib[i]) + iv0[i] @ uv             # once per positive
                steps = 0
                for k in range(nn):
                    if wrong == "yui-fresh":
                        yui = st.ib[i] + iv0[i] @ uv
                    j, cnt, yuj = decide(uv, iv0, pos, p, k, yui)
                    if j is None:
                        skipped += 1
                        continue
                    trained += 1
                    steps += 1
                    out["positives_twice"] += steps == 2
                    out["negatives_twice"] += j in before
                    pred = yui - yuj
                    out["pred_lt18"] += pred < -18.0
                    out["pred_lt88"] += pred < -88.5
                    if choices is not None and st.loss == 3:
                        # A followed decision says that the device saw a violator: pred < 1 in ITS arithmetic, while this one may be
                        # a hair above (a margin inside the band).  HINGE's gradient jumps from -1 to 0 exactly there: it is taken
                        # on the device's side of the jump.  (The other losses are smooth: a pred off by < tol moves g by < tol.)
                        pred = min(pred, 1.0)
                    rank = items_left // cnt
                    if draws.I - row.size <= 2:
                        out[f"rank{(draws.I - row.size) // cnt}"] += 1
                    g = loss_grad(st.loss, pred) * ((st.l[rank - 1] if rank else 0.0) if wrong == "rank-minus-one" else st.l[rank])
                    if in_place and wrong == "stale-positive-row":
                        st.iv[i][:] = first_load
                    if in_place and wrong == "stale-repeated-negative" and j in before:
                        st.iv[j][:] = before[j]
                    before[j] = st.iv[j].copy()
                    uv_grad = g * (iv0[i] - iv0[j]) + lam2 * uv
                    uvpre = uv.copy()                    # all three from the pre-step values
                    _step(st, uv, ua, uv_grad)
                    if wrong == "post-step-uv":
                        uvpre = uv.copy()
                    if in_place:
                        gi = g * uvpre + lam2 * st.iv[i]
                        gj = -g * uvpre + lam2 * st.iv[j]
                        _step(st, st.iv[i], st.iva[i], gi)
                        _step(st, st.iv[j], st.iva[j], gj)
                    else:
                        records.append((i, j, g, uvpre))
        stepped = [r for i, j, _, _ in records for r in (i, j)]
        out["rows_twice"] += len(stepped) - len(set(stepped))
        for i, j, g, uvpre in (reversed(records) if wrong == "phase-I-reversed" else records):
            # phase I: every item row takes its pairs' steps in (user, pair) order
            _step(st, st.iv[i], st.iva[i], g * uvpre + lam2 * st.iv[i])
            _step(st, st.iv[j], st.iva[j], -g * uvpre + lam2 * st.iv[j])
        out["mixed_blocks"] += bool(skipped and trained)
    return out


def max_err(tables, st):
    """-> (max over uv, uva, iv, iva of max |table - state's| / (1e-3 + max |state's|), the table's name): the measure of the 2e-4 bound.
    tables: name -> array BY POSITION (or an object with those attributes, another State)"""
    worst, name = 0.0, None
    for n in ("uv", "uva", "iv", "iva"):
        ref = getattr(st, n)
        got = tables[n] if isinstance(tables, dict) else getattr(tables, n)
        err = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / (1e-3 + np.abs(ref).max()))
        if err > worst:
            worst, name = err, n
    return worst, name


# ---- fixtures shared by tests/test_warp_reference.py (their premises, on the CPU) and tests/test_gpu_warp.py (the trajectories) --------
STREAM_INIT, P_W, P_WU = 3, 0, 4


def init_table(rows, K, which, seed, scale=0.01):
    """cdae_hip_init_params of an IMF-shaped handle: float32(cdae_init_uniform(key, row * K + k) * scale)"""
    key = _u(rng_key(seed, 0, which, STREAM_INIT))
    idx = np.arange(rows * K, dtype=np.uint64)
    r = _mix64_v(key + _u(GOLDEN) * (idx + _u(1))) >> _u(32)
    return ((((r.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)) * 2.0 - 1.0) * scale).astype(np.float32).reshape(rows, K)


BIAS_SEED = 17


def bias_start(spec, n, salt=0):
    """the item biases a case starts from (hyper["ib0"]): None -> zeros; "uniform<a>" -> float32 uniform in +-a from a fixed numpy seed.
    salt = 1: the user biases the GPU test sets next to them (they are part of no score)"""
    if not spec:
        return np.zeros(n, dtype=np.float32)
    assert spec.startswith("uniform"), spec
    a = float(spec[len("uniform"):])
    return np.random.default_rng(BIAS_SEED + salt).uniform(-a, a, n).astype(np.float32)


def init_state(U, I, K, seed, **hyper):
    """the state cdae_hip_init_params(seed) leaves: tables drawn as above, accumulators 1e-4, biases 0.  hyper["acc0"], hyper["ib0"]: a
    fixture that starts its accumulators or its item biases elsewhere (the GPU test sets them through set_param)"""
    acc0 = np.float32(hyper.get("acc0") or 1e-4)
    return State(init_table(U, K, P_WU, seed), np.full((U, K), acc0), init_table(I, K, P_W, seed), np.full((I, K), acc0),
                 bias_start(hyper.get("ib0"), I), **hyper)


EPOCHS = 2
# (name, data set, batch_users, num_dim, num_neg, hyper-parameters beyond WARPConfig's defaults, parameter seed, stream seed)
# The stream seeds are the first for which the free-running reference reaches every search depth AND is well conditioned: with AdaGrad
# and no beta a step is lr * grad / sqrt(1e-4 + sum grad^2), a sign function of the gradient while the accumulator is young, so a
# coordinate whose gradient passes through zero amplifies rounding by lr / sqrt(1e-4) x |g| per step.  On such a trajectory the same
# numpy loop in float32 ends 1e-3 of the range from its float64 self (stream seed 2 at K = 64: 1.2e-3; the device then measures 1.9e-3),
# and a parameter bound of 2e-4 would measure the trajectory, not the kernel.  run_free() reports that drift and
# tests/test_warp_reference.py bounds it at DRIFT_MAX, a quarter of the bound.
# Where the issue leaves the learn rate open it is chosen so that |score| stays below 16: with AdaGrad and no beta the first step of a
# coordinate is learn_rate whatever the gradient, so a pair's score moves by about num_dim * learn_rate^2 per step — 0.1 at K = 24 is
# 0.03 at K = 200 and 0.015 at K = 300 ("tiny" has rows of up to 60 positives: 0.05 for its loop at K = 24).
#
# The loop at the K tier edges runs with WARPConfig's defaults, learn rate included, and there a pair's score moves by num_dim * 0.01 per
# step while the accumulators are young: from cdae_hip_init_params' state (accumulators 1e-4) |score| reaches 26.7 / 24.6 / 57.7 / 47.4 /
# 93.1 at K = 128 / 129 / 256 / 257 / 512 whatever the seed.  The hyper-parameters stay the defaults; what those five fixtures change is
# their START: the accumulators begin at acc0 = 3, 5, 10 (about K / 50, the smallest of these at which the free reference stays below 16),
# so that a step moves a coordinate by at most lr * |g| / sqrt(acc0), a fraction of its value, and not by lr.  The GPU test writes that
# start through set_param; everything else of the state is init_params'.
CASES = [(f"d40-loop-K{K}", "d40", 1, K, 5, dict(acc0=a) if a else {}, 11, s)
         for K, s, a in ((1, 191, 0), (64, 4, 0), (65, 11, 0), (128, 5, 3.0), (129, 1, 3.0), (256, 1, 5.0), (257, 2, 5.0), (512, 5, 10.0))] + [
    ("d40-loop-sgd", "d40", 1, 200, 5, dict(adagrad=False, learn_rate=0.03), 11, 1),
    ("d40-loop-log", "d40", 1, 200, 5, dict(loss=2, learn_rate=0.03), 11, 3),
    ("d40-loop-neg1", "d40", 1, 200, 1, dict(learn_rate=0.03), 11, 29),
    ("d40-loop-neg12", "d40", 1, 200, 12, dict(learn_rate=0.03), 11, 2),
    ("tiny-loop", "tiny", 1, 24, 5, dict(learn_rate=0.05), 11, 1),
    ("d40-block8", "d40", 8, 24, 5, {}, 11, 9),
    ("tiny-block33-K24", "tiny", 33, 24, 5, {}, 11, 3),
    ("tiny-block33-K200", "tiny", 33, 200, 5, dict(learn_rate=0.02), 11, 1),
    ("tiny-block33-K300", "tiny", 33, 300, 5, dict(learn_rate=0.015), 11, 1),
    # The pinning pass (tools/warp_cases.py searched the stream seeds: the first that meets every premise of tests/test_warp_reference.py).
    # ib0: the item biases start uniform in +-0.5 (bias_start) where every other case starts them at 0 — half the margin, fifty times a
    # score of init_params' tables, so the biases decide which candidate is the first violator.
    # (d40-loop-bias-K200 is the worst-conditioned trajectory of the file: started one float32 ulp away and led through the same decisions,
    # the fp64 reference ends 2e-5 ... 6e-5 from itself, the other loop cases 5e-7 ... 1e-5; its float32 drift is 2.8e-5.)
    ("d40-loop-bias-K65", "d40", 1, 65, 5, dict(ib0="uniform0.5"), 11, 2),
    ("d40-loop-bias-K200", "d40", 1, 200, 5, dict(ib0="uniform0.5", learn_rate=0.03), 11, 3),
    ("d40-block8-bias", "d40", 8, 24, 5, dict(ib0="uniform0.5"), 11, 1),
    ("tiny-block33-bias-K24", "tiny", 33, 24, 5, dict(ib0="uniform0.5"), 11, 1),
    # D40 and two users with one and two items left: rank weights l[0], l[1], l[2], draws that end in the walk behind 32 rejections.
    # D40's own rows are part of it, so it reaches every search depth and is exempt from NO depth assertion; unmet() adds l[0 .. 2].
    ("dense-loop-K24", "d40dense", 1, 24, 5, {}, 11, 2),
    # a block handle whose range ends in a block of ONE user: that block runs in place
    ("d40p1-block8", "d40p1", 8, 24, 5, {}, 11, 1),
    ("tiny-block299", "tiny", 299, 24, 5, {}, 11, 1),
    # The saturation pass.  SQUARE and CROSS_ENTROPY had never run in warp_user_kernel: the loop and blocks of 8 with the defaults.
    ("d40-loop-square", "d40", 1, 24, 5, dict(loss=0), 11, 2),
    ("d40-loop-ce", "d40", 1, 24, 5, dict(loss=5), 11, 2),
    ("d40-block8-square", "d40", 8, 24, 5, dict(loss=0), 11, 1),
    ("d40-block8-ce", "d40", 8, 24, 5, dict(loss=5), 11, 26),
] + [
    # ib0 = "uniform100": item biases uniform in +-100.  Biases are never stepped, so the scores stay near +-100 for the whole run and
    # yui - score, what mf_loss_grad sees, reaches -200: beyond -18 and beyond -88.5, where __expf has overflowed (a trained pair has
    # yui - score < 1, so only that side exists).  SQUARE then steps on gradients of 400.  `saturated` exempts exactly these cases from
    # SCORE_MAX; unmet() asks them for trained pairs below -18 and below -88.5 in its place.  An fp32 score of 100 is still accurate to
    # 1e-5, a hundredth of TOL.
    # LOGISTIC's only pin is here: g = -1 / d near d = 0, so from biases of zero or +-0.5 its trajectory cannot be pinned (the float32
    # reference ends 1.0, respectively 1.7e-3 ... 6.4e-2, from the float64 one); at d near -100 it is as smooth as the others.
    (f"d40-loop-bias100-{n}", "d40", 1, 24, 5, dict(loss=l, ib0="uniform100", learn_rate=0.03, saturated=True), 11, 1)
    for n, l in (("square", 0), ("logistic", 1), ("log", 2), ("hinge", 3), ("ce", 5))
]
TOL = 1e-3                       # the band in which an fp32 and an fp64 margin may fall on different sides of 0
NEAR_SHARE = 1e-3                # ... and the share of comparisons that may lie inside it
SCORE_MAX = 16.0
DRIFT_MAX = 5e-5                 # float32 against float64 on the reference alone: a quarter of the GPU test's 2e-4


def fixture_data(name):
    import mf_conflict_ref
    from cdae_amd import synth
    if name == "tiny":
        return synth.generate_shape("tiny", seed=5)
    d = mf_conflict_ref.d40()
    rows = [d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]] for u in range(d.num_users)]
    if name == "d40dense":       # ... and a user with every item but one, one with every item but two: items_left 1 and 2
        rows += [np.delete(np.arange(40), 23), np.delete(np.arange(40), (7, 31))]
    if name == "d40p1":          # ... and a ninth user: under batch_users = 8 the second block holds one user
        rows += [np.sort(np.random.default_rng(7).choice(40, 9, replace=False))]
    return d if name == "d40" else mf_conflict_ref.from_rows(rows, 40)


def user_order(lens, B):
    """cdae_hip_user_order of a block handle (activity_order, cdae_dataset_plan.h): the users by descending row length (ties by id) cut
    into groups of B, the full groups in the order of their index's multiplicative hash, a short last group last.  B = 1, or one block
    that holds every user (dataset_plan::build): the identity."""
    lens = np.asarray(lens)
    if B <= 1 or lens.size <= B:
        return np.arange(lens.size)
    by_len = np.argsort(-lens, kind="stable")
    groups = [by_len[t:t + B] for t in range(0, lens.size, B)]
    tail = [groups.pop()] if lens.size % B else []
    groups = [groups[k] for k in sorted(range(len(groups)), key=lambda k: (k * 2654435761) & 0xFFFFFFFF)]
    return np.concatenate(groups + tail)


def _as_float32(st):
    for n in ("uv", "uva", "iv", "iva", "ib", "l"):
        setattr(st, n, getattr(st, n).astype(np.float32))
    st.lam2, st.lr = np.float32(st.lam2), np.float32(st.lr)
    return st


def run_free(case):
    """the free-running reference of one case: -> the totals of train()'s counts over the case's epochs (max_abs_score: the maximum)
    and `drift`: how far the same run in float32 ends from it, in the measure of the GPU test's bound (max |difference| / (1e-3 + max
    |value|) over the four tables) — what rounding alone does to this trajectory, whatever the kernel"""
    name, ds, B, K, nn, hyper, pseed, sseed = case
    d = fixture_data(ds)
    ptr, col = d.train_ptr, d.train_col           # (in id order: the premises of a block case are those of this order)
    st = init_state(d.num_users, d.num_items, K, pseed, **hyper)
    st32 = _as_float32(init_state(d.num_users, d.num_items, K, pseed, **hyper))
    tot = {}
    for ep in range(EPOCHS):
        draws = Draws(ptr, col, d.num_items, nn, sseed, ep)
        o = train(st, draws, B)
        with np.errstate(over="ignore"):                 # float32: exp of a saturated difference overflows to inf and 1 / inf is 0, as on the device
            train(st32, draws, B)
        for k, v in o.items():
            if k not in ("bad", "record"):
                tot[k] = max(tot.get(k, 0.0), v) if k == "max_abs_score" else tot.get(k, 0) + v
    tot["drift"] = max_err(st32, st)[0]
    return tot


def unmet(case, t):
    """the premises of run_free's totals `t` that do NOT hold, as texts: what tests/test_warp_reference.py asserts to be empty and what
    tools/warp_cases.py searches the stream seeds for"""
    checks = [
        (t["disagreements"] == 0 and t["cnt1"] + t["cnt2_64"] + t["cnt65_499"] == t["trained"], "the counts do not add up"),
        (t["cnt1"] >= 1, "no search ends at the first draw"),
        (t["cnt2_64"] >= 1, "no search ends inside the first round of 64 candidates"),
        (t["cnt65_499"] >= 1, "no search ends beyond the first round"),
        (t["exhausted"] >= 1, "no search is exhausted"),
        (case[2] == 1 or t["mixed_blocks"] >= 1, "no block both skips and trains pairs"),
        (t["near"] < NEAR_SHARE * t["comparisons"], f"near {t['near']} of {t['comparisons']}"),
        (t["drift"] <= DRIFT_MAX, f"drift {t['drift']:.3g}"),     # rounding alone leaves three quarters of the GPU test's bound to the kernel
    ]
    if case[5].get("saturated"):     # scores near +-100 on purpose: what the loss sees must reach both saturated regions
        checks += [(t["pred_lt18"] >= 1, "no trained pair has yui - score below -18"),
                   (t["pred_lt88"] >= 1, "no trained pair has yui - score below -88.5"),
                   (t["max_abs_score"] > 88.5, f"|score| {t['max_abs_score']:.3g} does not leave the middle")]
    else:
        checks += [(t["max_abs_score"] <= SCORE_MAX, f"|score| {t['max_abs_score']:.3g}")]
    if case[1] == "d40dense":
        checks += [(t[f"rank{r}"] >= 1, f"no pair steps with the rank weight l[{r}]") for r in range(3)]
    if case[2] > 1 and fixture_data(case[1]).num_users % case[2] == 1:
        checks += [(t["one_user_blocks"] == EPOCHS, "the tail block of one user did not run")]
    return [text for ok, text in checks if not ok]


def run_wrong(case, wrong=None, follow=None):
    """the case's epochs from its start with train(wrong=...) -> (the state it ends in, the record of every epoch, the `bad` of every
    epoch).  follow: the records of another run, taken as `choices` epoch by epoch"""
    name, ds, B, K, nn, hyper, pseed, sseed = case
    d = fixture_data(ds)
    ptr, col = d.train_ptr, d.train_col           # (in id order: the premises of a block case are those of this order)
    st = init_state(d.num_users, d.num_items, K, pseed, **hyper)
    records, bad = [], []
    for ep in range(EPOCHS):
        o = train(st, Draws(ptr, col, d.num_items, nn, sseed, ep), B, choices=follow[ep] if follow else None, tol=TOL, wrong=wrong)
        records.append(o["record"]); bad += o["bad"]
    return st, records, bad
