"""CPU: bench.py --dump-outputs' size rule, on a stand-in model of the real shapes — float32 .npy files under 64 MB in all, small arrays
whole, larger ones as the same fixed rows on every call, a parameter and its accumulator as the same rows."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from cdae_amd import binding as b, synth  # noqa: E402


class StandIn:
    """get(which) of a CDAE handle: every row of every parameter holds its own row id (+ 0.5 for the accumulators)"""

    def __init__(self, shape, K, **cfg):
        self.num_users, self.num_items, _ = synth.SHAPES[shape]
        self.cfg = b.CDAEConfig(num_dim=K, **cfg)

    _shape = b.CDAE._shape

    def get(self, which):
        s = self._shape(which)
        rows = np.arange(s[0], dtype=np.float32).reshape((-1,) + (1,) * (len(s) - 1))
        return np.broadcast_to(rows + 0.5 * (which % 2), s).astype(np.float32)


@pytest.mark.parametrize("shape,K,cfg", [("small", 32, {}), ("ml10m", 200, {}), ("netflix", 200, {}), ("cfg5_items", 512, {}),
                                         ("ml10m", 200, dict(asymmetric=True, linear_function=True))])
def test_dump_stays_under_64_mb_and_samples_fixed_rows(tmp_path, shape, K, cfg):
    m = StandIn(shape, K, **cfg)
    bench.dump_outputs(m, str(tmp_path / "a"))
    bench.dump_outputs(m, str(tmp_path / "b"))
    files = sorted(os.listdir(tmp_path / "a"))
    want = {"W", "W_ag", "b", "b_ag", "bp", "bp_ag", "Wu", "Wu_ag"} | ({"V", "V_ag", "Uu", "Uu_ag"} if cfg else set())
    assert {f[:-4] for f in files} == want and all(f.endswith(".npy") for f in files)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64e6
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for name, a in got.items():
        assert a.dtype == np.float32 and np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy"))), name
        ids = a.reshape(a.shape[0], -1)[:, 0] - (0.5 if name.endswith("_ag") else 0.0)
        assert (np.diff(ids) > 0).all(), name                          # ascending rows of the full array
        if not name.endswith("_ag"):
            assert np.array_equal(ids, got[name + "_ag"].reshape(a.shape[0], -1)[:, 0] - 0.5), name
    assert got["b"].shape == (K,) and got["bp"].shape == (m.num_items,)    # small arrays whole
    if shape == "small":
        assert got["Wu"].shape == (m.num_users, K) and got["W"].shape == (m.num_items, K)
    if shape == "ml10m" and not cfg:
        assert got["W"].shape == (m.num_items, K) and 0 < got["Wu"].shape[0] < m.num_users
