"""numpy fp64 restatement of the fold-in definition (include/cdae_hip.h cdae_hip_fold_in_rows): the reference step
train_one_user_corruption (cdae.hpp:198-358) with every update of a shared parameter removed.  A yardstick, not a test:
tests/test_fold_in_reference.py checks it against one literal Oracle.step_user, tests/test_gpu_fold_in.py checks the device against it.
The second half of the file is the exact family: models, fixtures and the proof under which tests/test_gpu_fold_in_exact.py may
ask the device for the yardstick's bits.

The masks and negatives come from Oracle.draw_inputs / Oracle.draw_negatives of an oracle built over the guest rows (uid = row index,
i.e. stream_id_base = 0): the counter streams of include/cdae_rng.h, evaluated by the oracle's own C++.
"""
import numpy as np

AG_INIT = 1e-4          # reset()'s accumulator value (cdae.hpp:109-134)


def no_node(K):
    """the start node of a row without a user: wu = 0, uu = 1, both accumulators 1e-4"""
    return np.zeros(K), np.full(K, AG_INIT), np.ones(K), np.full(K, AG_INIT)


def activate(cfg, h):
    """get_hidden_values' activation with the reference's clamps (cdae.hpp:391-414)"""
    if cfg.linear:
        return h.copy()
    if not cfg.tanh:
        return np.where(h > 18.0, 1.0, np.where(h < -18.0, 0.0, 1.0 / (1.0 + np.exp(-np.clip(h, -18.0, 18.0)))))
    r = np.exp(-2.0 * np.clip(h, -9.0, 9.0))
    return np.where(h > 9.0, 1.0, np.where(h < -9.0, -1.0, (1.0 - r) / (1.0 + r)))


def act_deriv(cfg, z):
    """cdae.hpp:208-215"""
    return np.ones_like(z) if cfg.linear else (1.0 - z * z if cfg.tanh else z - z * z)


def loss_grad(cfg, y, t):
    """loss.hpp:53-55 (SQUARE = 0), loss.hpp:141-147 (CROSS_ENTROPY)"""
    if cfg.loss_type == 0:
        return -2.0 * (t - y)
    if y < -18.0:
        return np.exp(y) - t
    if y > 18.0:
        return 1.0 - t
    return 1.0 / (1.0 + np.exp(-y)) - t


def ada_row(cfg, p, acc, grad):
    """one `if (using_adagrad_) {...} p -= lr * grad` block on a row (e.g. cdae.hpp:317-331); returns the new (p, acc)"""
    if cfg.using_adagrad:
        acc = acc + grad * grad
        grad = grad / (np.sqrt(acc) + cfg.beta)
    return p - cfg.learn_rate * grad, acc


def scale_of(cfg):
    return 1.0 / (1.0 - cfg.corruption_ratio) if cfg.scaled else 1.0        # cdae.hpp:202-205


def step(cfg, P, items, kept, negatives, node):
    """ONE (epoch, corruption) step of a row.  P: dict of the frozen fp64 parameters W [I, K], b [K], bp [I], and V [I, K] when
    asymmetric; items: the row; kept / negatives: its draws; node = (wu, wu_ag, uu, uu_ag).  -> (node', z, hg)"""
    wu, wa, uu, ua = node
    W = P["W"]
    D = P["V"] if cfg.asymmetric else W
    K = W.shape[1]
    S = np.zeros(K)
    for j in kept:
        S = S + W[int(j)]
    h = S * scale_of(cfg)
    if cfg.linear_function:
        h = uu * h
    h = h + P["b"]
    if cfg.user_factor:
        h = h + wu
    z = activate(cfg, h)
    hg = np.zeros(K)
    for j in items:
        hg = hg + loss_grad(cfg, float(D[int(j)] @ z + P["bp"][int(j)]), 1.0) * D[int(j)]
    for j in negatives:                                                     # a duplicate counts once per occurrence
        hg = hg + loss_grad(cfg, float(D[int(j)] @ z + P["bp"][int(j)]), 0.0) * D[int(j)]
    delta = hg * act_deriv(cfg, z)
    new_wu, new_wa, new_uu, new_ua = wu, wa, uu, ua
    if cfg.user_factor:                                                     # both gradients from the pre-step values
        new_wu, new_wa = ada_row(cfg, wu, wa, delta + cfg.lambda_ * wu)
    if cfg.linear_function:
        new_uu, new_ua = ada_row(cfg, uu, ua, cfg.lambda_ * uu + delta * S)
    return (new_wu, new_wa, new_uu, new_ua), z, hg


def fold_in_row(o, P, r, node, seed, epoch_begin, n_epochs):
    """all epochs of row r of the oracle `o` (built over the guest rows: its draws are those of stream id r)"""
    cfg = o.cfg
    items = o.col[o.row_ptr[r]:o.row_ptr[r + 1]]
    if items.size == 0:
        return node
    for e in range(epoch_begin, epoch_begin + n_epochs):
        for c in range(cfg.num_corruptions):
            node, _, _ = step(cfg, P, items, o.draw_inputs(seed, e, r, c), o.draw_negatives(seed, e, r, c), node)
    return node


def fold_in(o, P, nodes, seed, epoch_begin, n_epochs):
    """every row of `o`; nodes = four [R, K] arrays of start nodes -> four [R, K] arrays of fitted nodes"""
    out = [np.array(a, dtype=np.float64, copy=True) for a in nodes]
    for r in range(o.U):
        res = fold_in_row(o, P, r, tuple(a[r] for a in out), seed, epoch_begin, n_epochs)
        for a, v in zip(out, res):
            a[r] = v
    return out


# ---- the exact family: models on which the definition is exact in fp32 in ANY summation order ------------------------------------------
# linear activation, SQUARE loss, plain SGD, learn_rate / lambda_ / scale powers of two, W (and a different V) with a fixed small number
# of +-1 entries per item row, b / b' / the start wu in {-1, 0, 1}, uu = 1.  Every quantity of step s is then a multiple of a power of
# two (1 in the first step; 2^-8 for z, y, g, hg and 2^-16 for the node after the second, finer under linear_function), and as long
# as every sum's absolute terms add up to less than 2^24 of those units no partial sum in any order needs more than fp32's 24 bits:
# the device must return the fp64 yardstick's bits.  Whether a (K, row, step) qualifies is NOT assumed: exact_step asserts it on the
# real draws, and tests/test_fold_in_reference.py runs it over every case below (the GPU file runs the same list and nothing else).
NO_USER = 0xFFFFFFFF
GUEST_BIT = 0x80000000
EXACT_SEED = 9
AG32 = float(np.float32(AG_INIT))     # the accumulator value as the device holds it


def exact_family(K, *, num_items=977, nnz=2, density=1.0, asymmetric=False, linear_function=False, user_factor=True, num_neg=5,
                 num_corruptions=1, corruption_ratio=0.5, scaled=True, lr_log2=-6, lambda_log2=-2, num_users=8, seed=1):
    """-> (OracleConfig, P, users): P the frozen fp64 tables W [I, K], V (asymmetric) or None, b [K], bp [I]; users = (Wu [U, K] in
    {-1, 0, 1}, Uu = 1).  density: the share of item rows that are not zero (K = 1, 2: most rows must be, or a long row's sums
    outgrow 24 bits)."""
    import oracle as orc
    cfg = orc.OracleConfig(num_dim=K, num_neg=num_neg, num_corruptions=num_corruptions, loss_type=0, using_adagrad=False,
                           asymmetric=asymmetric, user_factor=user_factor, linear=True, scaled=scaled, tanh=False,
                           linear_function=linear_function, lambda_=2.0 ** lambda_log2, learn_rate=2.0 ** lr_log2,
                           corruption_ratio=corruption_ratio, beta=1.0)
    scale = scale_of(cfg) if corruption_ratio < 1.0 or not scaled else np.inf
    assert cfg.lambda_ != 0 and np.isfinite(scale) and np.log2(scale) == int(np.log2(scale)), "scale must be a power of two"
    rng = np.random.default_rng([seed, K, num_items, int(asymmetric)])
    nz = min(nnz, K)

    def table():
        T = np.zeros((num_items, K))
        cols = np.argsort(rng.random((num_items, K)), axis=1)[:, :nz]
        T[np.arange(num_items)[:, None], cols] = rng.choice([-1.0, 1.0], (num_items, nz))
        T[rng.random(num_items) >= density] = 0.0
        return T
    W = table()
    V = table() if asymmetric else None
    assert V is None or not np.array_equal(V, W)
    tri = lambda *shape: rng.integers(-1, 2, shape).astype(np.float64)          # noqa: E731
    P = dict(W=W, V=V, b=tri(K), bp=tri(num_items))
    return cfg, P, (tri(num_users, K), np.ones((num_users, K)))


def _is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.isfinite(a).all() and np.array_equal(a.astype(np.float32).astype(np.float64), a))


def _grid_log2(*arrays):
    """log2 of the largest power of two that divides every element (None: all zero)"""
    v = np.abs(np.concatenate([np.ravel(np.asarray(a, dtype=np.float64)) for a in arrays]))
    v = v[v != 0]
    if not v.size:
        return None
    m, e = np.frexp(v)                                              # v = m 2^e, m in [0.5, 1)
    q = (m * 2.0 ** 53).astype(np.int64)                            # exact: 53 significand bits
    tz = np.log2((q & -q).astype(np.float64)).astype(np.int64)      # trailing zeros (a power of two: exact)
    return int((e.astype(np.int64) - 53 + tz).min())


def _sum_bits(abs_sum, grid):
    """bits a partial sum can need: log2(sum of |terms| / their common grid); 0 for an empty or all-zero sum"""
    top = float(np.max(abs_sum, initial=0.0))
    return 0.0 if grid is None or top == 0 else float(np.log2(top)) - grid


def exact_step(cfg, P, items, kept, negatives, node):
    """one step of the definition in fp64 for a member of the exact family, with the PROOF that fp32 takes it exactly in any order:
    asserts that every per-operation result is an fp32 value (S, S uu, h and its partial sum, y, g, hg, delta, delta S, both gradients,
    the new node) and that for each sum — S, h, every D[j].z + b'[j], hg — the absolute terms add up to less than 2^24 units of the
    terms' common grid.  -> (node', bits): bits the largest log2 of those ratios."""
    assert cfg.linear and cfg.loss_type == 0 and not cfg.using_adagrad
    wu, wa, uu, ua = (np.asarray(a, dtype=np.float64) for a in node)
    W = P["W"]
    D = P["V"] if cfg.asymmetric else W
    items, kept, negatives = (np.asarray(a, dtype=np.int64) for a in (items, kept, negatives))
    lam, lr, scale = cfg.lambda_, cfg.learn_rate, scale_of(cfg)
    val, sums = {}, {}
    S = W[kept].sum(axis=0)
    sums["S"] = (np.abs(W[kept]).sum(axis=0), _grid_log2(W[kept]))
    x = S * uu if cfg.linear_function else S
    terms = [scale * x, P["b"]] + ([wu] if cfg.user_factor else [])
    h = sum(terms)
    sums["h"] = (sum(np.abs(t) for t in terms), _grid_log2(*terms))
    z = h
    E = np.concatenate([items, negatives])
    t = np.r_[np.ones(items.size), np.zeros(negatives.size)]
    DE = D[E]
    y = DE @ z + P["bp"][E]
    sums["y"] = (np.abs(DE) @ np.abs(z) + np.abs(P["bp"][E]), _grid_log2(z, P["bp"][E]))
    g = -2.0 * (t - y)
    hg = g @ DE
    sums["hg"] = (np.abs(g) @ np.abs(DE), _grid_log2(g))
    delta = hg
    val.update(S=S, x=x, h_partial=terms[0] + terms[1], h=h, y=y, t_y=t - y, g=g, hg=hg)
    new = [wu, wa, uu, ua]
    if cfg.user_factor:
        gw = lam * wu + delta
        new[0] = wu - lr * gw
        val.update(grad_wu=gw, wu=new[0])
    if cfg.linear_function:
        dS = delta * S
        gu = lam * uu + dS
        new[2] = uu - lr * gu
        val.update(delta_S=dS, grad_uu=gu, uu=new[2])
    for name, a in val.items():
        assert _is_f32(a), f"{name} is not an fp32 value"
    bits = {name: _sum_bits(*s) for name, s in sums.items()}
    assert max(bits.values()) < 24.0, bits
    return tuple(new), max(bits.values())


def step_f32(cfg, P32, items, kept, negatives, node, order):
    """the step in float32, every operation rounded, in another order than the yardstick's.  order "reversed": kept items, examples
    and the terms of h last to first; "split4": the long role's order — the row's positions in chunks of 64, the positives and then
    the negatives in chunks of 64, chunk q (counted through all three lists) to partial q mod 4, the partials added from 0.
    P32: the tables as float32.  -> node'"""
    f = np.float32
    wu, wa, uu, ua = (np.asarray(a, dtype=f) for a in node)
    W = P32["W"]
    D = P32["V"] if cfg.asymmetric else W
    K = W.shape[1]
    items = [int(j) for j in items]
    kept_set = set(int(j) for j in kept)
    ex = [(j, f(1)) for j in items] + [(int(j), f(0)) for j in negatives]
    n = len(items)
    if order == "reversed":
        s_parts, e_parts = [[j for j in reversed(items) if j in kept_set]], [ex[::-1]]
    else:
        s_parts, e_parts, chunk = [[] for _ in range(4)], [[] for _ in range(4)], 0
        for q0 in range(0, n, 64):
            s_parts[chunk % 4] += [j for j in items[q0:q0 + 64] if j in kept_set]
            chunk += 1
        for lo, hi in ((0, n), (n, len(ex))):
            for q0 in range(lo, hi, 64):
                e_parts[chunk % 4] += ex[q0:min(q0 + 64, hi)]
                chunk += 1
    S = np.zeros(K, f)
    for part in s_parts:
        acc = np.zeros(K, f)
        for j in part:
            acc = acc + W[j]
        S = S + acc
    x = S * uu if cfg.linear_function else S
    scale, lam, lr = f(scale_of(cfg)), f(cfg.lambda_), f(cfg.learn_rate)
    if order == "reversed":
        h = (wu if cfg.user_factor else np.zeros(K, f)) + P32["b"]
        h = h + x * scale
    else:
        h = x * scale + P32["b"]
        if cfg.user_factor:
            h = h + wu
    z = h
    hg = np.zeros(K, f)
    for part in e_parts:
        acc = np.zeros(K, f)
        for j, t in part:
            y = (D[j][::-1] * z[::-1]).sum(dtype=f) if order == "reversed" else np.dot(D[j], z)
            y = f(y) + P32["bp"][j]
            acc = acc + f(-2) * (t - y) * D[j]
        hg = hg + acc
    assert S.dtype == f and h.dtype == f and hg.dtype == f
    new = [wu, wa, uu, ua]
    if cfg.user_factor:
        new[0] = wu - lr * (lam * wu + hg)
    if cfg.linear_function:
        new[2] = uu - lr * (lam * uu + hg * S)
    return tuple(new)


SWEEP = (1, 2, 3, 42, 43, 63, 64, 65, 128, 129, 300)             # the chunk seams, num_neg = 5's role seam 42 | 43, a 300-item row
LF129 = (1, 2, 42, 43, 63, 64, 65, 128, 129)
TWO_STEPS = {"2ep": dict(n_epochs=2), "nc2": dict(n_epochs=1, num_corruptions=2)}


def _exact_cases():
    """id -> dict(K, lens, family keywords, n_epochs, uids: "mixed" | "guest" | "none", check: the rows compared (None: all))"""
    cases = {}

    def add(name, K, lens, uids="mixed", check=None, **fam):
        for mode, kw in TWO_STEPS.items():
            k = dict(kw)
            n_epochs = k.pop("n_epochs")
            cases[f"{name}-K{K}-{mode}"] = dict(K=K, lens=tuple(lens), uids=uids, check=check, n_epochs=n_epochs, fam={**fam, **k})
    for K in (1, 2):
        add("sweep", K, SWEEP, density=1 / 16)
    for K in (63, 64, 65, 128, 129, 256, 257, 300, 512):
        add("sweep", K, SWEEP)
    for K in (128, 300):                                          # either side of every role seam: 256 | 257, 128 | 129, 19 | 20
        add("neg0", K, (1, 64, 65, 129, 256, 257), num_neg=0)
        add("neg1", K, (1, 64, 65, 128, 129, 257), num_neg=1)
        add("neg12", K, (1, 19, 20, 64, 65, 129), num_neg=12)
        add("asym", K, SWEEP, asymmetric=True)
    for K in (64, 129):                                           # 21 items, rows of 20: every negative is the one item left
        add("dup", K, (20, 1, 20, 19, 2), num_items=21, num_neg=12, lambda_log2=0)      # 260 examples: a workgroup
        add("dup-asym", K, (20, 1, 20, 19, 2), num_items=21, asymmetric=True, lambda_log2=0)       # 120: a wavefront
    for K in (65, 256):
        add("guest", K, SWEEP, uids="guest")
    for K, lens, lam in ((128, LF129, -2), (256, SWEEP, -2), (300, SWEEP, 0), (512, SWEEP, -2)):
        add("lf", K, lens, linear_function=True, lambda_log2=lam)
        add("lf-nouf", K, lens, linear_function=True, user_factor=False, lambda_log2=lam)
    for K in (128, 300):
        add("keep-all", K, (1, 42, 43, 65, 129), corruption_ratio=0.0)
        add("keep-none", K, (1, 42, 43, 65, 129, 300), corruption_ratio=1.0, scaled=False)
    add("keep-none-lf", 128, (1, 42, 43, 65, 129), corruption_ratio=1.0, scaled=False, linear_function=True)
    add("long-only", 257, (43, 64, 129, 300, 65, 128), uids="none")
    return cases


EXACT_CASES = _exact_cases()
# One call of 32 768 + 40 rows of 1-3 items whose second chunk holds long rows at its first, a middle and its last slot.  The first
# chunk holds long rows too, so that the second chunk's slot list does not begin the device list; their slots (5, 9, 30) are below the
# second chunk's 40 rows and none of them is a slot of its long rows: read for the wrong chunk, the list names rows that exist.
SEAM_R, SEAM_CHUNK, SEAM_K = 32768 + 40, 32768, 64
SEAM_LONG = {5: 64, 9: 43, 30: 129, SEAM_CHUNK: 43, SEAM_CHUNK + 17: 129, SEAM_R - 1: 300}
SEAM_CHECK = tuple(sorted(set(range(0, SEAM_CHUNK, 1024)) | set(range(0, 40)) | set(range(SEAM_CHUNK - 3, SEAM_R))))


def exact_rows(case):
    """the rows of a case and their uids: (ptr, col, uids)"""
    fam = dict(case["fam"])
    I = fam.get("num_items", 977)
    rng = np.random.default_rng([77, case["K"], len(case["lens"])])
    rows = [np.sort(rng.choice(I, n, replace=False)).astype(np.uint32) for n in case["lens"]]
    R = len(rows)
    if case["uids"] == "guest":
        uids = (GUEST_BIT | np.arange(R)).astype(np.uint32)
    elif case["uids"] == "none":
        uids = np.full(R, NO_USER, np.uint32)
    else:
        uids = np.array([NO_USER if r % 3 == 0 else (5 * r) % 8 for r in range(R)], np.uint32)
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    return ptr, np.concatenate(rows), uids


def seam_case():
    """the case of the host list's seams, as a dict like those of EXACT_CASES with its rows attached"""
    rng = np.random.default_rng(66)
    lens = rng.integers(1, 4, SEAM_R)
    for r, n in SEAM_LONG.items():
        lens[r] = n
    rows = [np.sort(rng.choice(977, n, replace=False)).astype(np.uint32) for n in lens]
    uids = np.where(np.arange(SEAM_R) % 3 == 0, NO_USER, (5 * np.arange(SEAM_R)) % 8).astype(np.uint32)
    ptr = np.r_[0, np.cumsum(lens)].astype(np.int64)
    return dict(K=SEAM_K, lens=tuple(int(n) for n in lens), uids="mixed", check=SEAM_CHECK, n_epochs=2, fam={},
                rows=(ptr, np.concatenate(rows), uids))


def guest_table(case):
    """the wu rows of the guest table a "guest" case starts from, in {-1, 0, 1}"""
    rng = np.random.default_rng([78, case["K"]])
    return rng.integers(-1, 2, (len(case["lens"]), case["K"])).astype(np.float64)


def exact_reference(case, prove=False):
    """-> (family, rows, start, want, bits): the four start and fitted [R, K] fp64 arrays of a case (rows outside case["check"] keep
    their start node) and, with prove, per checked row the most bits any sum of any step needs.  prove: exact_step's assertions on
    every step, the literal yardstick `step` on the same draws, and step_f32 in both other orders — all must agree exactly."""
    import oracle as orc
    family = exact_family(case["K"], **case["fam"])
    cfg, P, (Wu, Uu) = family
    ptr, col, uids = case["rows"] if "rows" in case else exact_rows(case)
    R, K = ptr.size - 1, case["K"]
    o = orc.Oracle(cfg, R, P["W"].shape[0], ptr, col)
    start = [np.zeros((R, K)), np.full((R, K), AG32), np.ones((R, K)), np.full((R, K), AG32)]
    if cfg.user_factor:
        real = (uids != NO_USER) & (uids & GUEST_BIT == 0)
        start[0][real] = Wu[uids[real]]
        if case["uids"] == "guest":
            start[0][:] = guest_table(case)
    want = [a.copy() for a in start]
    P32 = {k: None if v is None else v.astype(np.float32) for k, v in P.items()}
    bits = {}
    for r in (range(R) if case["check"] is None else case["check"]):
        items = col[ptr[r]:ptr[r + 1]]
        node = tuple(a[r] for a in start)
        worst = 0.0
        for e in range(case["n_epochs"]):
            for c in range(cfg.num_corruptions):
                kept, neg = o.draw_inputs(EXACT_SEED, e, r, c), o.draw_negatives(EXACT_SEED, e, r, c)
                assert neg.size == items.size * cfg.num_neg
                new, b = exact_step(cfg, P, items, kept, neg, node)
                worst = max(worst, b)
                if prove:
                    lit, _, _ = step(cfg, P, items, kept, neg, node)
                    for order in ("reversed", "split4"):
                        f32 = step_f32(cfg, P32, items, kept, neg, node, order)
                        for name, a, b64, l in zip(("wu", "wu_ag", "uu", "uu_ag"), f32, new, lit):
                            assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), b64), (r, e, c, order, name)
                            assert np.array_equal(l, b64), (r, e, c, "literal", name)
                node = new
        bits[r] = worst
        for a, v in zip(want, node):
            a[r] = v
    return family, (ptr, col, uids), start, want, bits
