"""-m gpu: the fold-in against the fp64 yardstick (tests/fold_in_ref.py) at the shapes tests/test_gpu_fold_in.py leaves out.

That file runs fold_in_rows_kernel<NI> at num_dim 40, 200 and 300 (NI = 1, 4, 8), num_neg = 5 and the default corruption.  Here, on
the same rows fixture, with the same statistic and the same bound — max|gpu - ref| / (1e-3 + max|ref|) < 2e-4 for each of wu, wu_ag,
uu, uu_ag after three epochs, the project's bound for a few fp32 AdaGrad steps against fp64:

  * CROSS_ENTROPY with AdaGrad at both edges of every tier: K = 1, 64 | 65, 128 | 129, 256 | 257, 512 (NI = 2 is launched by no
    other real-valued case);
  * the identity activation (`linear`), `scaled = False`, tanh at K = 128;
  * num_neg = 1 and 12, the fixture extended by a row either side of their role seams (128 | 129, 19 | 20 items);
  * linear_function with num_corruptions = 2 at K = 128 and 300 (UN = 4 under linear_function), and linear_function without
    user_factor: only (uu, uu_ag) move and wu / wu_ag come back as 0 / 1e-4.

The models are tests/test_gpu_rows.py's trained(K, flags): two epochs on 300 users x 977 items.  With CDAE_RECORD_MEASURED every case
appends its four errors as fold_in_tier_<case> (profiles/fold_in_tiers_measured.txt holds a run).
"""
import numpy as np
import pytest

import cdae_amd
import oracle as orc
from helpers import record_measured
from test_gpu_fold_in import AG, LF, LONG_EXAMPLES, NC2, SEED, TANH, fold_all, fold_rows, model_of, oracle_config, start_nodes
from test_gpu_rows import I_T, NO_USER, U_T, csr, gathered, rows_of

import fold_in_ref as ref

pytestmark = pytest.mark.gpu

BOUND = 2e-4
NAMES = ("wu", "wu_ag", "uu", "uu_ag")
TIERS = [1, 64, 65, 128, 129, 256, 257, 512]
# case -> (K, flags of the model, the lengths of the rows added either side of the case's role seam)
CASES = {f"ce_K{K}": (K, (), ()) for K in TIERS}
CASES.update({
    "linear_K128": (128, (("linear", True),), ()),
    "unscaled_K128": (128, (("scaled", False),), ()),
    "tanh_K128": (128, TANH, ()),
    "neg1_K128": (128, (("num_neg", 1),), (128, 129)),
    "neg12_K128": (128, (("num_neg", 12),), (19, 20)),
    "lf_nc2_K128": (128, LF + NC2, ()),
    "lf_nc2_K300": (300, LF + NC2, ()),
    "lf_without_user_factor_K128": (128, LF + (("user_factor", False),), ()),
})


def rows_with(extra):
    """the fixture of tests/test_gpu_fold_in.py, then rows of the given lengths: one with a user node, one without"""
    ptr, col, uids = fold_rows()
    if not extra:
        return ptr, col, uids
    rng = np.random.default_rng(sum(extra))
    rows = rows_of(ptr, col) + [np.sort(rng.choice(I_T, n, replace=False)).astype(np.uint32) for n in extra]
    more = np.array([NO_USER if k % 2 else int(rng.integers(0, U_T)) for k in range(len(extra))], np.uint32)
    return csr(rows) + (np.concatenate([uids, more]),)


def nodes_of(model, uids):
    """test_gpu_fold_in.start_nodes; a handle without user_factor has no Wu rows: its wu / wu_ag are 0 / 1e-4 for every row"""
    if model.cfg.user_factor:
        return start_nodes(model, uids)
    K = model.cfg.num_dim
    return (np.zeros((len(uids), K), np.float32), np.full((len(uids), K), AG, np.float32),
            gathered(model.get(cdae_amd.P_UU), uids, 1.0), gathered(model.get(cdae_amd.P_UU_AG), uids, AG))


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_fp64_yardstick_at_every_tier_and_setting(built, name):
    K, flags, extra = CASES[name]
    model, _ = model_of(K, flags)
    cfg = model.cfg
    ptr, col, uids = rows_with(extra)
    lens = np.diff(ptr)
    ex = lens * (1 + cfg.num_neg)
    assert {1, 2, 63, 64, 65, 129, 300, 976} | set(extra) <= set(lens.tolist()) and (ex > LONG_EXAMPLES).any() and (ex <= LONG_EXAMPLES).any()
    if extra:                                                        # the added pair sits either side of this num_neg's seam
        assert extra[0] * (1 + cfg.num_neg) <= LONG_EXAMPLES < extra[1] * (1 + cfg.num_neg)
    R = ptr.size - 1
    got = fold_all(model, ptr, col, uids, epoch_begin=2, n_epochs=3)
    start = nodes_of(model, uids)
    o = orc.Oracle(oracle_config(cfg), R, I_T, ptr, col)
    P = dict(W=model.get(cdae_amd.P_W).astype(np.float64), b=model.get(cdae_amd.P_B).astype(np.float64),
             bp=model.get(cdae_amd.P_BP).astype(np.float64), V=model.get(cdae_amd.P_V).astype(np.float64) if cfg.asymmetric else None)
    want = ref.fold_in(o, P, [a.astype(np.float64) for a in start], SEED, 2, 3)
    errs = {}
    for which, g, w, s0 in zip(NAMES, got, want, start):
        assert np.isfinite(g).all(), which
        errs[which] = float(np.abs(g.astype(np.float64) - w).max() / (1e-3 + np.abs(w).max()))
        print(f"fold_in_tier_{name} {which}: err {errs[which]:.3e}, max|ref| {np.abs(w).max():.4g}, moved {np.abs(w - s0).max():.3g}")
    record_measured(f"fold_in_tier_{name}", **errs)
    for which, e in errs.items():
        assert e < BOUND, (name, which, errs)
    # the fit moved what the configuration fits, and nothing else
    assert (np.abs(want[0] - start[0]).max() > 1e-3) == cfg.user_factor and (np.abs(want[2] - start[2]).max() > 1e-3) == cfg.linear_function
    if not cfg.user_factor:
        assert (got[0] == 0).all() and (got[1] == AG).all()
    if not cfg.linear_function:
        assert (got[2] == 1).all() and (got[3] == AG).all()
