"""-m gpu: fism_user_kernel and fism_pair_user_kernel at SATURATED predictions, against tests/fism_ref.py and tests/fism_pair_ref.py in fp64.

Both kernels build their own prediction (s v . Q[item] + bu + bi; s v . (Q[i] - Q[j]) + bi[i] - bi[j]), call mf_loss_grad at their own
place with their own label (0 or -1 for a FISM negative, always 1 on a difference), scale the gradient by s and step with AdaGrad without
beta.  Every other FISM / FISMauc trajectory of the suite starts from init_params' tables of 1e-3 and keeps |prediction| below 20; none
reaches +-88, where __expf overflows and rcp(inf) = 0 has to hold, and none steps a parameter on a gradient of 2000.

The fixture (fism_ref.grid_data, grid_tables; modelled on tests/test_gpu_saturation.py::test_mf_from_grid_scores) makes user u's first
prediction the u-th point of tests/golden/saturation_kat.npz's grid (53 values up to +-1000) bit for bit, and the drawn negatives among
items 0 .. 52 carry grid values too.  Each test asserts that premise on the tables the HANDLE holds, then trains two epochs and compares
every table element by element, |gpu - ref| <= GRID_BOUND (GRID_FLOOR + |ref|) with GRID_BOUND = 1e-3 and GRID_FLOOR = 1e-2: MF_BOUND and
FLOOR of test_mf_from_grid_scores, the same arithmetic (fp32 storage, __expf, 1-ulp rcp and sqrt) against fp64.  That the float32
reference stays within a quarter of the bound, that the fp64 reference meets every class of saturated instance, and that it tells five
faulty loops (three for FISMauc) from the right one are tests/test_fism_reference.py's and tests/test_fism_pair_reference.py's assertions;
the class premise is asserted here as well, on the reference the device is compared with.

Cases at K = 16 (NI = 1): FISM {SQUARE, LOG, CROSS_ENTROPY} x AdaGrad and {LOG, CROSS_ENTROPY} x plain SGD; FISMauc {SQUARE, LOG} x AdaGrad
and LOG x SGD; for each kernel LOG + AdaGrad at K = 300 (NI = 8) and without bias terms.  SQUARE with plain SGD is left out: on the full
grid the fp64 reference overflows by itself (at 2^-10 and at 2^-20), and a truncated grid would not be this test.  The rows hold five items
against eight wavefronts, so three wavefronts own no row.  Both residency settings leave the same bits on one case per kernel.
"""
import numpy as np
import pytest

import cdae_amd
import fism_pair_ref as pr
import fism_ref as fr
from helpers import record_measured

pytestmark = pytest.mark.gpu

FISM_TABLES = (("P", cdae_amd.P_W), ("Pa", cdae_amd.P_W_AG), ("Q", cdae_amd.P_V), ("Qa", cdae_amd.P_V_AG), ("bi", cdae_amd.P_BP), ("bu", cdae_amd.P_UB))
PAIR_TABLES = FISM_TABLES[:5]
FISM_CLASSES = ((True, 1), (True, -1), (False, 1), (False, -1))
PAIR_CLASSES = ((True, 1), (True, -1))
# kernel -> (handle, config, the cases, the compared tables, the reference, the classes of saturated instance it must have met)
KERNELS = {
    "fism": (cdae_amd.FISM, cdae_amd.FISMConfig, fr.GRID_CASES, FISM_TABLES, fr.grid_reference, FISM_CLASSES),
    "fismauc": (cdae_amd.FISMP, cdae_amd.FISMPConfig, fr.GRID_PAIR_CASES, PAIR_TABLES, pr.grid_reference, PAIR_CLASSES),
}


def make(kernel, name):
    """a handle that holds the grid tables (accumulators 1e-4 and biases 0 from init_params) -> (handle, the state it starts from)"""
    handle, config, cases, tables, _, _ = KERNELS[kernel]
    K, hyper = cases[name]
    h = {**fr.GRID_HYPER, **hyper}
    m = handle(config(num_dim=K, num_neg=5, lt=h["loss"], using_adagrad=h.get("adagrad", True), using_bias_term=h.get("bias", True),
                      learn_rate=h["learn_rate"], lambda_=h["lambda_"], alpha=h["alpha"]))
    m.reset(fr.grid_data(), seed=fr.PSEED)
    P, Q = fr.grid_tables(K)
    m.set(cdae_amd.P_W, P)
    m.set(cdae_amd.P_V, Q)
    got = {n: m.get(w) for n, w in tables}
    np.testing.assert_array_equal(got["P"], P); np.testing.assert_array_equal(got["Q"], Q)
    assert (got["Pa"] == np.float32(1e-4)).all() and (got["Qa"] == np.float32(1e-4)).all() and not got["bi"].any()
    return m, fr.grid_state(K, hyper, tables=(got["P"], got["Q"]))


def train(m, resident=True):
    """two epochs -> every compared table; all finite after every epoch"""
    m.set_resident(resident)
    tables = PAIR_TABLES if isinstance(m, cdae_amd.FISMP) else FISM_TABLES
    for ep in range(fr.EPOCHS):
        st = m.train_one_iteration(fr.GRID_SSEED, ep)
        d = fr.grid_data()
        per = 5 if isinstance(m, cdae_amd.FISMP) else 6
        assert (st.users, st.examples) == (d.num_users, int(d.train_ptr[-1]) * per)
        got = {n: m.get(w) for n, w in tables}
        for n, a in got.items():
            assert np.isfinite(a).all(), (n, ep)
    return got


@pytest.mark.parametrize("kernel,name", [(k, n) for k, v in KERNELS.items() for n in v[2]])
def test_two_epochs_from_grid_scores(kernel, name):
    _, _, cases, tables, reference, classes = KERNELS[kernel]
    m, start = make(kernel, name)
    # the premise, on the handle's own tables: the first predictions are the grid, in float64 and in float32
    first = fr.grid_first(start)
    np.testing.assert_array_equal(first, fr.grid().astype(np.float64))
    np.testing.assert_array_equal(fr.grid_first(start.as_float32()), fr.grid())
    assert fr.share_beyond(first, 18) > 0.4 and fr.share_beyond(first, 88.5) > 0.14          # 22 and 8 of the 53 grid points
    assert m.plan()["resident_rows"] == fr.resident_rows(cases[name][0]) and np.diff(fr.grid_data().train_ptr).max() < fr.WAVES
    ref = reference(name)
    assert all(ref.classes.get(c, 0) >= 1 for c in classes), ref.classes                    # ... and saturated instances of every class
    got = train(m)
    errs = {n: fr.grid_measure(got[n], getattr(ref, n)) for n, _ in tables}
    print(f"{kernel} {name}: max |pred| {ref.max_abs_pred:.4g}, " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    record_measured(f"saturation_{kernel}_{name}", **errs)
    worst = max(errs, key=errs.get)
    assert errs[worst] <= fr.GRID_BOUND, (worst, errs)
    if not cases[name][1].get("bias", True):
        assert not got["bi"].any() and ("bu" not in got or not got["bu"].any())
    m.close()


@pytest.mark.parametrize("kernel,name", [("fism", "ce-ada"), ("fismauc", "log-ada")])
def test_both_residency_settings_give_the_same_bits_when_saturated(kernel, name):
    outs = []
    for resident in (True, False):
        m, _ = make(kernel, name)
        assert m.plan()["resident_rows"] > 0
        m.set_resident(resident)
        assert (m.plan()["resident_rows"] > 0) == resident
        outs.append(train(m, resident))
        m.close()
    for n in outs[0]:
        np.testing.assert_array_equal(outs[0][n].view(np.uint32), outs[1][n].view(np.uint32), err_msg=n)
