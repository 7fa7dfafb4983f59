"""CPU (-m "not gpu"): the oracle's bf16-faithful full-output mode (Oracle.train_full(..., bf16=True)).

That mode is the reference tests/test_gpu_full_exact.py holds the device's full-output decode to, bit for bit on integer data, so
it is pinned here on its own: its rounding helper against torch's CPU float32 -> bfloat16 conversion (round to nearest even), its
agreement with the plain fp64 mode where every rounded operand is already a bf16 value, its difference from it elsewhere, and one
block of it against an independent numpy restatement of the three rounded products.
"""
import numpy as np
import pytest
import torch

from cdae_amd import synth
import oracle as orc
from oracle import binding as ob


def torch_bf16(x):
    """fp64 -> fp32 (numpy, nearest even) -> bf16 (torch CPU, nearest even) -> fp64"""
    with np.errstate(over="ignore"):                      # (the huge cases: past the fp32 range is +-inf, as in the oracle)
        f = np.asarray(x, dtype=np.float64).astype(np.float32)
    return torch.from_numpy(f).to(torch.bfloat16).to(torch.float64).numpy()


@pytest.fixture(scope="module")
def tiny(built):
    return synth.generate_shape("tiny", seed=5)


def test_round_bf16_is_torch_float32_to_bfloat16(built):
    f = np.float32
    one = 1.0
    ulp1 = 2.0 ** -7                                      # bf16 spacing in [1, 2)
    ties = [one + ulp1 / 2, one + 3 * ulp1 / 2,           # halfway: even neighbour below (1.0), even neighbour above (1 + 2 ulp)
            -(one + ulp1 / 2), -(one + 3 * ulp1 / 2), 2.0 + 2.0 ** -7, 2.0 + 3 * 2.0 ** -7]
    near_ties = [one + ulp1 / 2 + 2.0 ** -23, one + ulp1 / 2 - 2.0 ** -24]
    up_to_pow2 = [2.0 - 2.0 ** -9, 4.0 - 2.0 ** -8, 0.5 - 2.0 ** -11, -(2.0 - 2.0 ** -9), float(np.nextafter(f(2.0), f(0)))]
    tiny_vals = [2.0 ** -126, 2.0 ** -133, 2.0 ** -140, 1e-40, -1e-40, 2.0 ** -149, 1e-300]     # fp32 denormals and below
    huge = [3.0e38, float(np.finfo(np.float32).max), -float(np.finfo(np.float32).max), 1e39, -1e300]
    signed_zero = [0.0, -0.0]
    rng = np.random.default_rng(0)
    random = np.concatenate([rng.standard_normal(4000), rng.standard_normal(2000) * 10.0 ** rng.integers(-30, 30, 2000),
                             rng.uniform(-1, 1, 2000) * 2.0 ** -120])
    x = np.concatenate([ties, near_ties, up_to_pow2, tiny_vals, huge, signed_zero, random]).astype(np.float64)
    got = ob.round_bf16(x)
    want = torch_bf16(x)
    np.testing.assert_array_equal(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))                  # -0 stays -0
    # the cases are what they claim to be
    assert got[0] == 1.0 and got[1] == 1.0 + 2 * ulp1 and got[2] == -1.0     # ties to even, both parities, both signs
    assert got[len(ties)] == 1.0 + ulp1                                        # a hair above the tie goes up
    assert got[len(ties) + len(near_ties)] == 2.0 and got[len(ties) + len(near_ties) + 1] == 4.0   # round up into the next binade
    assert np.isinf(ob.round_bf16(np.array([1e39])))[0]
    assert np.isnan(ob.round_bf16(np.array([np.nan])))[0]


def _one_block(tiny, bf16, cfg_kw, params=None, B=48, unrounded=False):
    cfg = orc.OracleConfig(**cfg_kw)
    o = orc.Oracle(cfg, tiny.num_users, tiny.num_items, tiny.train_ptr, tiny.train_col)
    o.init_params(3)
    for which, arr in (params or {}).items():
        o.set(which, arr)
    o.train_full(7, 0, B, 0, B, bf16=bf16, unrounded_positives=unrounded)
    return o


def _grid_params(tiny, K, rng):
    """parameters on a coarse dyadic grid: with the linear hidden layer and SQUARE, z, D, y and g are all bf16 values"""
    I, U = tiny.num_items, tiny.num_users
    g = lambda shape, lo, hi, e: rng.integers(lo, hi + 1, shape).astype(np.float64) * 2.0 ** -e
    return {ob.P_W: g((I, K), -1, 1, 2), ob.P_V: g((I, K), -1, 1, 2), ob.P_WU: g((U, K), -1, 1, 2), ob.P_B: g(K, -1, 1, 2),
            ob.P_BP: g(I, -1, 1, 1)}


@pytest.mark.parametrize("asym", [False, True])
def test_bf16_mode_equals_plain_mode_on_bf16_exact_operands(tiny, asym):
    K = 8
    kw = dict(num_dim=K, loss_type=ob.LOSS_SQUARE, linear=True, using_adagrad=False, asymmetric=asym, lambda_=0.0,
              learn_rate=2.0 ** -4, corruption_ratio=0.0, scaled=False)
    params = _grid_params(tiny, K, np.random.default_rng(1))
    # premise: every operand the bf16 mode rounds is a bf16 value already (z via the oracle's own encode, D, g = 2 (y - t))
    probe = _one_block(tiny, False, kw, params, B=0)
    uids = np.arange(48, dtype=np.uint32)
    Z = probe.encode(7, 0, 1, uids)
    D = params[ob.P_V] if asym else params[ob.P_W]
    Y = Z @ D.T + params[ob.P_BP]
    T = np.zeros_like(Y)
    for s, u in enumerate(uids):
        T[s, tiny.train_col[tiny.train_ptr[u]:tiny.train_ptr[u + 1]]] = 1.0
    G = 2.0 * (Y - T)
    for a in (Z, D, G):
        assert np.array_equal(torch_bf16(a), a)
    a, b = _one_block(tiny, False, kw, params), _one_block(tiny, True, kw, params)
    for which in range(ob.P_COUNT):
        assert np.array_equal(a.get(which), b.get(which)), which


@pytest.mark.parametrize("kw", [dict(), dict(loss_type=ob.LOSS_SQUARE, asymmetric=True), dict(using_adagrad=False, tanh=True)])
def test_bf16_mode_differs_from_plain_mode_on_general_data(tiny, kw):
    """the rounding is applied: the decoder rows, b' and the hidden layer all move.  The decoder rows and b' by about the bf16
    precision; the hidden gradient hg = sum_j g_j D[j] cancels over the whole item space (every g_j of a negative has the same sign),
    so its rounding error is a larger share of its value — there the check is only that the difference stays below the step.  (The
    99th percentile: where dD[j] + lambda D[j] cancels, an AdaGrad step takes any relative error to order one)"""
    a = _one_block(tiny, False, dict(num_dim=24, **kw))
    b = _one_block(tiny, True, dict(num_dim=24, **kw))
    dec = ob.P_V if kw.get("asymmetric") else ob.P_W
    for which in (dec, ob.P_BP, ob.P_B, ob.P_WU):
        x, y = a.get(which), b.get(which)
        step = np.abs(x - _one_block(tiny, False, dict(num_dim=24, **kw), B=0).get(which)).max()   # how far one block moves it
        d = np.quantile(np.abs(x - y), 0.99)
        assert np.abs(x - y).max() > 0, which
        assert d < (0.05 if which in (dec, ob.P_BP) else 0.5) * step, (which, d, step)


@pytest.mark.parametrize("unrounded", [False, True])
@pytest.mark.parametrize("loss", [ob.LOSS_SQUARE, ob.LOSS_CE])
def test_bf16_mode_one_block_equals_a_numpy_restatement(tiny, loss, unrounded):
    """asymmetric, SGD: after one block V[j] = V[j] - lr (G^T bf16(Z) + lambda V[j]) and b'[j] = b'[j] - lr (sum_u G[u][j] + lambda b'[j])
    with G = bf16(loss'(bf16(Z) bf16(V)^T + b', T)) — the three rounding sites of the device's products, restated with torch's rounding.
    unrounded_positives (the unfused plans' fix-up): a positive's y is Z V^T + b' from the unrounded operands."""
    K, B, lr, lam = 24, 48, 0.05, 0.01
    kw = dict(num_dim=K, loss_type=loss, asymmetric=True, using_adagrad=False, learn_rate=lr, lambda_=lam)
    o0 = _one_block(tiny, True, kw, B=0)
    V0, bp0 = o0.get(ob.P_V).reshape(tiny.num_items, K), o0.get(ob.P_BP)
    uids = np.arange(B, dtype=np.uint32)
    Zr, Vr = torch_bf16(o0.encode(7, 0, 1, uids)), torch_bf16(V0)
    Y = Zr @ Vr.T + bp0
    T = np.zeros_like(Y)
    for s, u in enumerate(uids):
        T[s, tiny.train_col[tiny.train_ptr[u]:tiny.train_ptr[u + 1]]] = 1.0
    if unrounded:
        Yu = o0.encode(7, 0, 1, uids) @ V0.T + bp0
        assert np.abs(Yu - Y)[T == 1].max() > 0       # (the option changes the positives' y)
        Y = np.where(T == 1, Yu, Y)
    G = torch_bf16(2.0 * (Y - T) if loss == ob.LOSS_SQUARE else 1.0 / (1.0 + np.exp(-Y)) - T)
    V1 = V0 - lr * (G.T @ Zr + lam * V0)
    bp1 = bp0 - lr * (G.sum(axis=0) + lam * bp0)
    o1 = _one_block(tiny, True, kw, B=B, unrounded=unrounded)
    np.testing.assert_allclose(o1.get(ob.P_V).reshape(tiny.num_items, K), V1, rtol=0, atol=1e-12)
    np.testing.assert_allclose(o1.get(ob.P_BP), bp1, rtol=0, atol=1e-12)
