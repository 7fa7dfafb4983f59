"""numpy references of the user-parallel kernel family (encode_partial_kernel + encode_finish_kernel, encode_users_kernel,
data_loss_kernel, sqnorm_kernel) and the data sets, models and case tables tests/test_encode_reference.py (no GPU) and
tests/test_gpu_encode_exact.py (-m gpu) share.  No GPU here.

Two kinds of model:
  grid   every parameter an integer of small magnitude, linear hidden layer, a power-of-two scale: every hidden value, every score
         and every SQUARE loss term is an integer that fp32 holds exactly in ANY summation order (the premises are asserted from the
         operands: every sum of magnitudes < 2^24).  The references here work in int64 / exact fp64 from the masks
         Oracle.draw_inputs returns, independently of Oracle.encode / Oracle.data_loss, so a fault of the oracle does not hide.
  real   parameters from the counter-stream initialisation (rounded to fp32), off the grid.  emulate_encode restates in fp32 the
         ORDER include/cdae_hip.h promises: groups of `unit` consecutive positions of the row, each group's kept rows added from 0 in
         ascending position, the group sums added from 0 in group order (waves = 16: encode_users_kernel's association, wavefront w
         adds the groups w, w + 16, ... from 0, then the 16 sums are added from 0 in wavefront order); then the gate (a rounded
         product with Uu), h = fp32(acc * scale + b) rounded ONCE (a fused multiply-add), h = fp32(h + wu).  The scale is 1 or 2 in
         every case here: acc * scale is then exact in fp32, so `acc * scale + b` in numpy (two operations) rounds once as the
         fused form does — no double rounding to emulate.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import oracle as orc
from cdae_amd import synth

f32 = np.float32
SQUARE, CE = 0, 5                        # libcf::LossType
STREAM_CORRUPT, STREAM_LOSS = 0, 2       # include/cdae_rng.h CDAE_STREAM_CORRUPT / CDAE_STREAM_LOSS_CORRUPT
SEED, EPOCH = 77, 3                      # what every case draws its masks with
ENC_WAVES = 16                           # wavefronts of encode_users_kernel
ONE_LAUNCH_MAX = 768                     # batches of at most this many users take encode_users_kernel (include/cdae_hip.h)
LR = 2.0 ** -4

# one user per length: both sides of one unit (64 | 128), of the finish's eight partial rows in flight (512 = 8 x 64), of the 16
# wavefronts of the one-launch form (1024 = 16 x 64), and 1100
LENGTHS64 = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193, 511, 512, 513, 1023, 1024, 1025, 1100)
LENGTHS128 = LENGTHS64 + (255, 256, 257, 2047, 2048, 2049)       # ... and the same seams in units of 128
CATALOGUE = 2600


def unit_of(batch_users, num_users):
    """the handle's work-unit size (include/cdae_hip.h, `order`)"""
    return 64 if min(batch_users, num_users) <= 1024 else 128


# ---- data sets ---------------------------------------------------------------------------------------------------------------------
def _lengths(U, long_lengths, pins, rng):
    """[U] row lengths: `pins` {user: length} first, the other long lengths at random free users, 1 .. 3 items everywhere else"""
    lens = rng.integers(1, 4, size=U)
    rest = list(long_lengths)
    for n in pins.values():
        rest.remove(n)
    free = [u for u in rng.permutation(U).tolist() if u not in pins][:len(rest)]
    for u, n in list(pins.items()) + list(zip(free, rest)):
        lens[u] = n
    return lens


def _interactions(lens, I, rng, disjoint):
    if disjoint:                                                   # every item row holds ONE positive: I = sum of the lengths
        assert I is None
        I = int(lens.sum())
        perm, off = rng.permutation(I), np.r_[0, np.cumsum(lens)]
        rows = [np.sort(perm[off[u]:off[u + 1]]) for u in range(lens.size)]
    else:
        rows = [np.sort(rng.choice(I, size=int(n), replace=False)) for n in lens]
    assert all(1 <= r.size < I for r in rows)                      # what check_rows demands
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    return synth.Interactions(lens.size, I, ptr, np.concatenate(rows).astype(np.uint32), np.zeros(lens.size + 1, np.int64),
                              np.empty(0, np.uint32))


# name: (users, long lengths, pins, items or None (disjoint rows), batch_users)
_DATASETS = {
    # long rows at both ends, next to each other, and either side of the seam of a batch of 16
    "seam64": (50, LENGTHS64, {0: 1100, 1: 1025, 15: 1024, 16: 1023, 49: 513}, CATALOGUE, 16),
    "seam128": (1100, LENGTHS128, {0: 2049, 1: 2048, 1098: 1100, 1099: 2047}, CATALOGUE, 2048),
    "seam64d": (64, LENGTHS64, {0: 1100, 1: 1025, 63: 1024}, None, 64),                          # one batch, one launch
    "seam64d800": (800, LENGTHS64, {0: 1100, 1: 1025, 767: 513, 768: 1023, 799: 1024}, None, 800),   # one batch, two launches
    # batch 0 = users [0, 1100): two launches; the tail batch of 300: one launch, its 2049-item row wraps the 16 wavefronts
    "seam128d": (1400, LENGTHS128, {0: 2048, 1: 2047, 1099: 1025, 1100: 2049, 1101: 1100, 1399: 1024}, None, 1100),
}
CHUNK = 32768                            # users per launch group of cdae_hip_data_loss


@lru_cache(maxsize=None)
def dataset(name):
    """-> (Interactions, batch_users)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "chunk":                   # 32768 + 70 users over 200 items; the long rows are the last user of chunk 0 and the first of chunk 1
        lens = rng.integers(1, 4, size=CHUNK + 70)
        lens[CHUNK - 1], lens[CHUNK] = 129, 65
        return _interactions(lens, 200, rng, False), 64
    U, longs, pins, I, B = _DATASETS[name]
    return _interactions(_lengths(U, longs, pins, rng), I, rng, I is None), B


# ---- models ------------------------------------------------------------------------------------------------------------------------
def _sparse_pm1(rng, rows, K, per_row=6):
    """[rows, K] with min(K, per_row) entries of +-1 per row"""
    M = np.zeros((rows, K))
    for r in range(rows):
        k = rng.choice(K, size=min(K, per_row), replace=False)
        M[r, k] = rng.choice([-1.0, 1.0], size=k.size)
    return M


def make_case(ds, K, *, kind="grid", user_factor=True, gate=True, scaled=True, q=0.5, asymmetric=False, loss=SQUARE, nc=1,
              sparse_w=False, training=False, batch_users=None, lambda_=0.0, wu_range=2, seed=5):
    """A data set, a configuration and fp32 parameters.  kind "grid": integers (W in -2 .. 2, or six +-1 per row with sparse_w;
    V six +-1 per row; b' in -2 .. 2, Wu in -wu_range .. wu_range, b in -3 .. 3, the gate Uu in {-1, 1, 2}); "real": the counter-stream initialisation
    rounded to fp32, b ~ N(0, 0.1), Uu in [0.5, 1.5).  training: the decoder set up so that one epoch leaves lr z in every positive's
    V row (asymmetric, CE, plain SGD, lr 2^-4, lambda 0, no negatives, V = 0, b' = -1000)."""
    data, B = dataset(ds)
    B = B if batch_users is None else batch_users
    if training:
        asymmetric, loss, lambda_ = True, CE, 0.0
    c = SimpleNamespace(ds=ds, data=data, B=B, K=K, kind=kind, training=training, unit=unit_of(B, data.num_users),
                        scale=(1.0 / (1.0 - q) if scaled else 1.0),
                        flags=dict(using_adagrad=False, asymmetric=asymmetric, user_factor=user_factor, linear=True, scaled=scaled,
                                   tanh=False, linear_function=gate),
                        hyper=dict(lambda_=lambda_, learn_rate=LR, corruption_ratio=q, beta=1.0, num_neg=0 if training else 5,
                                   num_corruptions=nc),
                        loss=loss)
    assert c.scale in (1.0, 2.0)
    U, I = data.num_users, data.num_items
    rng = np.random.default_rng(1000 * seed + K)
    P = {}
    if kind == "grid":
        P["W"] = _sparse_pm1(rng, I, K) if sparse_w else rng.integers(-2, 3, size=(I, K)).astype(np.float64)
        P["b"] = rng.integers(-3, 4, size=K)
        P["bp"] = rng.integers(-2, 3, size=I)
        if asymmetric:
            P["V"] = _sparse_pm1(rng, I, K)
        if user_factor:
            P["Wu"] = rng.integers(-wu_range, wu_range + 1, size=(U, K))
        if gate:
            P["Uu"] = rng.choice([-1.0, 1.0, 2.0], size=(U, K))
    else:
        o = oracle_of(c, params=False)
        o.init_params(seed)
        P["W"] = o.get(orc.binding.P_W).reshape(I, K)
        P["b"] = rng.normal(0.0, 0.1, size=K)
        P["bp"] = rng.normal(0.0, 0.1, size=I)
        if asymmetric:
            P["V"] = o.get(orc.binding.P_V).reshape(I, K)
        if user_factor:
            P["Wu"] = o.get(orc.binding.P_WU).reshape(U, K)
        if gate:
            P["Uu"] = rng.uniform(0.5, 1.5, size=(U, K))
    if training:
        P["V"], P["bp"] = np.zeros((I, K)), np.full(I, -1000.0)
    c.P = {k: np.ascontiguousarray(v, dtype=f32) for k, v in P.items()}
    c.G = {k: _ints(v) for k, v in c.P.items()} if kind == "grid" else None        # the grid in int64
    return c


_WHICH = dict(W=orc.binding.P_W, V=orc.binding.P_V, Wu=orc.binding.P_WU, b=orc.binding.P_B, bp=orc.binding.P_BP, Uu=orc.binding.P_UU)


def oracle_of(c, params=True):
    """the fp64 oracle of a case, holding its fp32 parameters"""
    d = c.data
    o = orc.Oracle(orc.OracleConfig(num_dim=c.K, loss_type=c.loss, **c.flags, **c.hyper), d.num_users, d.num_items, d.train_ptr, d.train_col)
    if params:
        o.init_params(0)
        for name, a in c.P.items():
            o.set(_WHICH[name], a.astype(np.float64))
    return o


def row_of(c, u):
    return c.data.train_col[c.data.train_ptr[u]:c.data.train_ptr[u + 1]]


def kept_positions(c, o, u, *, mode=1, cidx=0, stream=STREAM_CORRUPT, seed=SEED, epoch=EPOCH):
    """positions of user u's row that enter the input sum.  mode 0: the whole row (none when corruption_ratio == 1, cdae.hpp:168-172);
    mode 1: the mask Oracle.draw_inputs draws for (seed, epoch, u, cidx, stream) — draw index cidx n + pos"""
    row = row_of(c, u)
    if mode == 0:
        return np.arange(0 if c.hyper["corruption_ratio"] == 1.0 else row.size)
    kept = o.draw_inputs(seed, epoch, int(u), cidx, stream)
    pos = np.searchsorted(row, kept)
    assert np.array_equal(row[pos], kept)
    return pos


def _ints(a):
    r = np.rint(a.astype(np.float64))
    assert np.array_equal(r, a), "not on the integer grid"
    return r.astype(np.int64)


# ---- exact references (grid) -----------------------------------------------------------------------------------------------------
def exact_hidden(c, u, pos, mode=1):
    """-> (z int64 [K], the largest sum of magnitudes behind an element of z): z = Uu (.) (scale sum_kept W) + b + Wu in integers"""
    G = c.G
    rows = G["W"][row_of(c, u)[pos].astype(np.int64)]
    sc = 1 if mode == 0 else int(c.scale)
    S, mag = rows.sum(axis=0) * sc, np.abs(rows).sum(axis=0) * sc
    if "Uu" in G:
        S, mag = S * G["Uu"][u], mag * np.abs(G["Uu"][u])
    S, mag = S + G["b"], mag + np.abs(G["b"])
    if "Wu" in G:
        S, mag = S + G["Wu"][u], mag + np.abs(G["Wu"][u])
    return S, int(mag.max())


def exact_encode(c, o, mode, uids):
    """-> (Z float64 [n, K] of integers, the largest sum of magnitudes): what cdae_hip_encode must return bit for bit"""
    memo, worst = {}, 0
    for u in set(int(u) for u in uids):
        memo[u], m = exact_hidden(c, u, kept_positions(c, o, u, mode=mode), mode)
        worst = max(worst, m)
    return np.array([memo[int(u)] for u in uids], dtype=np.float64).reshape(len(uids), c.K), worst


def exact_data_loss(c, o, seed=SEED, epoch=EPOCH):
    """SQUARE data_loss (cdae.hpp:78-101) of a grid model in integers, with the stream-2 masks (draw index c n + pos).
    -> dict(loss, max_err = max |1 - y|, max_mag = max (sum |z D| + |b'|) and of the hidden sums, nonzero = share of positives
    with 1 - y != 0)"""
    assert c.loss == SQUARE
    nc = c.hyper["num_corruptions"]
    total, max_err, max_mag, nonzero, count = 0, 0, 0, 0, 0
    for u in range(c.data.num_users):
        items = row_of(c, u).astype(np.int64)
        for ci in range(nc):
            z, m = exact_hidden(c, u, kept_positions(c, o, u, cidx=ci, stream=STREAM_LOSS, seed=seed, epoch=epoch))
            D = c.G["V" if "V" in c.G else "W"][items]
            e = 1 - (D @ z + c.G["bp"][items])
            total += int((e * e).sum())
            max_err = max(max_err, int(np.abs(e).max()))
            max_mag = max(max_mag, m, int((np.abs(D) @ np.abs(z) + np.abs(c.G["bp"][items])).max()))
            nonzero += int(np.count_nonzero(e))
            count += e.size
    assert nc in (1, 2) and total < 2 ** 53
    return dict(loss=total / nc, max_err=max_err, max_mag=max_mag, nonzero=nonzero / count)


def assert_loss_premises(ref):
    """under these every fp32 operation of data_loss_kernel is exact in any order, and a dropped positive changes the sum"""
    assert ref["max_err"] <= 4095 and ref["max_mag"] < 2 ** 24 and ref["nonzero"] >= 0.99, ref


def exact_penalty(c):
    """penalty_loss (cdae.hpp:103-107): 0.5 lambda (|W|^2 + |V|^2 + |Wu|^2 + |b|^2 + |b'|^2) — the gate Uu is NOT counted, V only
    when asymmetric, Wu only under user_factor"""
    G = c.G
    s = sum(int((G[k] * G[k]).sum()) for k in ("W", "V", "Wu", "b", "bp") if k in G)
    assert s < 2 ** 40
    return 0.5 * c.hyper["lambda_"] * s


# ---- the documented order in fp32 (real values) ------------------------------------------------------------------------------------
def emulate_hidden(c, u, pos, mode=1, waves=None):
    """-> (z float32 [K], sum of magnitudes float64 [K], kept rows): the order of the module docstring"""
    W = c.P["W"]
    row = row_of(c, u)
    n_units = -(-row.size // c.unit)
    sums = np.zeros((n_units, c.K), f32)
    mag = np.zeros(c.K)
    for p in pos:                                                           # ascending positions
        w = W[row[p]]
        sums[p // c.unit] = sums[p // c.unit] + w
        mag += np.abs(w)
    acc = np.zeros(c.K, f32)
    if waves is None:
        for g in range(n_units):
            acc = acc + sums[g]
    else:
        part = np.zeros((waves, c.K), f32)
        for g in range(n_units):                                            # wavefront g % waves takes the groups g, g + waves, ...
            part[g % waves] = part[g % waves] + sums[g]
        for w in range(min(n_units, waves)):
            acc = acc + part[w]
    sc = f32(1.0 if mode == 0 else c.scale)
    if "Uu" in c.P:
        acc, mag = acc * c.P["Uu"][u], mag * np.abs(c.P["Uu"][u])
    h = acc * sc + c.P["b"]                                                 # acc * sc is exact (sc = 1 or 2): one rounding, as fmaf
    mag = mag * float(sc) + np.abs(c.P["b"])
    if "Wu" in c.P:
        h, mag = h + c.P["Wu"][u], mag + np.abs(c.P["Wu"][u])
    assert h.dtype == f32
    return h, mag, len(pos)


def emulate_encode(c, o, mode, uids, waves=None):
    """-> (Z float32 [n, K], bound float64 [n, K]): bound = the rounding error the fp32 order may have against exact arithmetic,
    (terms + 3) 2^-24 / (1 - (terms + 3) 2^-24) times the sum of magnitudes (a sum of `terms` rows in any grouping, the gate, the
    fused multiply-add, + wu)"""
    memo = {}
    for u in set(int(u) for u in uids):
        z, mag, n = emulate_hidden(c, u, kept_positions(c, o, u, mode=mode), mode, waves)
        g = (n + 3) * 2.0 ** -24
        memo[u] = (z, g / (1 - g) * mag)
    return np.array([memo[int(u)][0] for u in uids], f32).reshape(len(uids), c.K), np.array([memo[int(u)][1] for u in uids]).reshape(len(uids), c.K)


# ---- the training encode, observed through the decoder -----------------------------------------------------------------------------
def training_waves(c, u):
    """the association the training encode of user u's batch takes: one launch (16 wavefronts) for a batch of at most 768 users"""
    B, U = min(c.B, c.data.num_users), c.data.num_users
    nb = min(B, U - u // B * B)
    return ENC_WAVES if nb <= ONE_LAUNCH_MAX else None


def expected_decoder(c, o, seed=SEED, epoch=EPOCH):
    """V after one epoch of a training case: every positive's gradient is -1 exactly and nothing else moves, so the row of item i,
    owned by user u, is fmaf(-lr, -z_c, V) over the corruptions c in order: fp32(lr z_0), then fp32(fp32(lr z_0) + lr z_1) (lr is a
    power of two: the products are exact).  -> (V float32 [I, K], the largest lr |z_0| . |z_1|: what the score of a positive may have
    moved by when the second corruption reads it)"""
    assert c.training
    V = np.zeros((c.data.num_items, c.K), f32)
    worst = 0.0
    for u in range(c.data.num_users):
        zs = [emulate_hidden(c, u, kept_positions(c, o, u, cidx=ci, seed=seed, epoch=epoch), 1, training_waves(c, u))[0]
              for ci in range(c.hyper["num_corruptions"])]
        v = np.zeros(c.K, f32)
        for z in zs:
            v = v + f32(LR) * z
        V[row_of(c, u).astype(np.int64)] = v
        if len(zs) == 2:
            worst = max(worst, LR * float(np.abs(zs[0]).astype(np.float64) @ np.abs(zs[1]).astype(np.float64)))
    return V, worst


def exact_decoder(c, o, seed=SEED, epoch=EPOCH):
    """the same on the grid, in integers: V / lr = sum over the corruptions of z_c.  -> (V / lr float64 [I, K], largest magnitude sum)"""
    Vq = np.zeros((c.data.num_items, c.K))
    worst = 0
    for u in range(c.data.num_users):
        tot, mags = 0, 0
        for ci in range(c.hyper["num_corruptions"]):
            z, m = exact_hidden(c, u, kept_positions(c, o, u, cidx=ci, seed=seed, epoch=epoch))
            tot, mags = tot + z, mags + m
        Vq[row_of(c, u).astype(np.int64)] = tot
        worst = max(worst, mags)
    return Vq, worst


# the second corruption of a training case reads V = lr z_0: its positives score lr z_0 . z_1 - 1000, and the gradient stays -1 exactly
# while exp(-score) overflows fp32 (score < -89); 850 leaves room
SECOND_CORRUPTION_ROOM = 850.0


# ---- case tables -------------------------------------------------------------------------------------------------------------------
K_ALL = (1, 63, 64, 65, 128, 129, 200, 256, 257, 512)          # every NI (row stride 64, 128, 256, 512) and both edges of each
K_PER_NI = (64, 128, 200, 512)
K_ORDER = (65, 200, 257, 512)

# tier 1: (data set, K, make_case keywords)
INFERENCE_CASES = ([("seam64", K, dict()) for K in K_ALL]
                   + [("seam64", K, kw) for K in (65, 257) for kw in (dict(user_factor=False), dict(gate=False), dict(scaled=False),
                                                                        dict(scaled=False, q=1.0))]
                   + [("seam128", K, dict()) for K in K_PER_NI])
CALL_SHAPE_K = (65, 257)                                          # n = 2 B + 1 with B = 7, and B = 1

# tier 2: real values, both unit sizes, scale 2 and (one case each) scale 1
ORDER_CASES = ([("seam64", K, dict(kind="real")) for K in K_ORDER] + [("seam64", 200, dict(kind="real", scaled=False, gate=False))]
               + [("seam128", K, dict(kind="real")) for K in K_ORDER] + [("seam128", 65, dict(kind="real", scaled=False, user_factor=False))])

# tier 3: the grid of the two-corruption case is sparse and ungated so that lr z_0 . z_1 stays inside SECOND_CORRUPTION_ROOM
TRAINING_CASES = ([("seam64d", K, dict(kind=kind, gate=False)) for K in K_ORDER for kind in ("grid", "real")]
                  + [("seam64d", 200, dict(kind=kind)) for kind in ("grid", "real")]
                  + [("seam64d800", 129, dict(kind=kind, gate=False)) for kind in ("grid", "real")]
                  + [("seam128d", 200, dict(kind=kind, gate=False)) for kind in ("grid", "real")]
                  + [("seam64d", 65, dict(kind="grid", gate=False, nc=2, sparse_w=True, user_factor=False)),
                     ("seam64d", 65, dict(kind="real", gate=False, nc=2))])

# tier 4: one K per NI plus 63 and 257; tied (W itself sparse) and asymmetric, the gate on and off, one or two corruptions.  Wu in
# -40 .. 40 spreads the scores (a sum of six +-z) so that fewer than 1 % of the positives have 1 - y = 0.
_WIDE = dict(wu_range=40)
LOSS_CASES = ([("seam64", K, dict(**_WIDE, sparse_w=True, gate=bool(n % 2), nc=1 + n % 2)) for n, K in enumerate((63, 64, 128, 200, 257, 512))]
              + [("seam64", K, dict(**_WIDE, asymmetric=True, gate=not n % 2, nc=1 + (n // 2) % 2)) for n, K in enumerate((63, 64, 128, 200, 257, 512))]
              + [("seam128", 64, dict(**_WIDE, sparse_w=True, nc=2)), ("seam128", 200, dict(**_WIDE, asymmetric=True, gate=False)),
                 ("seam128", 257, dict(**_WIDE, asymmetric=True, nc=2)), ("seam128", 512, dict(**_WIDE, sparse_w=True, gate=False))])
CHUNK_CASE = ("chunk", 8, dict(**_WIDE, asymmetric=True, nc=2))
PENALTY_CASES = [("seam64", 65, dict(lambda_=2.0 ** -6)), ("seam64", 257, dict(lambda_=2.0 ** -6, asymmetric=True)),
                 ("seam64", 129, dict(lambda_=2.0 ** -6, user_factor=False, asymmetric=True))]
SHARDED_CASES = [("seam64", 65, dict(**_WIDE, sparse_w=True, lambda_=2.0 ** -6, nc=2)), ("seam64", 257, dict(**_WIDE, asymmetric=True, lambda_=2.0 ** -6))]


def case_id(t):
    ds, K, kw = t
    return "-".join([ds, f"K{K}"] + [f"{k}={v}" for k, v in kw.items()])


@lru_cache(maxsize=None)
def _case(ds, K, kw):
    return make_case(ds, K, **dict(kw))


def case_of(t, **more):
    """the case of a table entry (built once per process), `more` added to its make_case keywords"""
    ds, K, kw = t
    return _case(ds, K, tuple(sorted({**kw, **more}.items())))


def call_lists(c):
    """the user lists of a tier-1 / tier-2 call: in order, reversed, and one with repeats in which the heaviest user appears
    batch_users times (more work units than any batch of distinct users has)"""
    U = c.data.num_users
    heavy = int(np.argmax(np.diff(c.data.train_ptr)))
    order = np.arange(U, dtype=np.uint32)
    return dict(order=order, reversed=order[::-1].copy(),
                repeats=np.array([heavy] * c.B + [U - 1, heavy, 0, U // 2, heavy], dtype=np.uint32))
