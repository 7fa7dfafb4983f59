"""numpy fp64 restatement of the fold-in definition (include/cdae_hip.h cdae_hip_fold_in_rows): the reference step
train_one_user_corruption (cdae.hpp:198-358) with every update of a shared parameter removed.  A yardstick, not a test:
tests/test_fold_in_reference.py checks it against one literal Oracle.step_user, tests/test_gpu_fold_in.py checks the device against it.

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
