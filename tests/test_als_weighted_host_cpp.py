"""The host C++ layer's libcf::WRMF with WRMFConfig::use_ratings, objective() and the weighted solve_rows overload
(src/model/recsys/wrmf.hpp) over cdae_hip_als_set_confidence / _objective / _solve_rows_weighted.
CPU: src/wrmf_weighted_check.cpp takes the methods' addresses with the documented signatures, compiles and links.  GPU: the same binary
fits a ratings file whose labels differ between pairs through Solver<WRMF>, prints a falling objective, and dumps its train rows,
weights and factors; the Python binding given the same rows, weights and seed must arrive at the same factors under 2e-4."""
import os
import re
import subprocess

import numpy as np
import pytest

import als_ref as ar
from cdae_amd import synth
from test_host_cpp import BUILD, ROOT, run

SEED, K, ITERS = 7, 16, 4


@pytest.fixture(scope="module")
def check(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "src"), "-s", "check"])
    return os.path.join(BUILD, "wrmf_weighted_check")


def write_rated(path, seed=5):
    """user item rating lines: the pairs of tests/test_host_cpp.py's write_ratings with play counts 1 .. 5 as labels"""
    d = synth.generate(300, 120, 9000, seed=seed)
    rng = np.random.default_rng(0)
    pairs = []
    for u in range(d.num_users):
        for ptr, col in ((d.train_ptr, d.train_col), (d.test_ptr, d.test_col)):
            pairs += [(u, int(i)) for i in col[ptr[u]:ptr[u + 1]]]
    rng.shuffle(pairs)
    labels = rng.integers(1, 6, len(pairs))
    with open(path, "w") as f:
        f.write("user item rating\n")
        for (u, i), r in zip(pairs, labels):
            f.write(f"u{u} i{i} {r}\n")


def test_the_additions_compile_and_link(check, tmp_path):
    rc, out = run([check], tmp_path)
    assert rc == 0 and "wrmf weighted check OK (compiled)" in out, out


@pytest.mark.gpu
def test_weighted_wrmf_through_the_host_layer(check, tmp_path):
    import cdae_amd
    from cdae_amd import P_W, P_WU
    write_rated(tmp_path / "ratings.txt")
    dump = tmp_path / "fit.bin"
    rc, out = run([check, "--run=true", f"--input_file={tmp_path / 'ratings.txt'}", f"--dump={dump}", f"--num_dim={K}", f"--iters={ITERS}"],
                  tmp_path, env={"CDAE_SEED": str(SEED)})
    assert rc == 0, out
    assert "wrmf weighted OK" in out and "labels 1 .. 5" in out and "{Ratings: 1}" in out
    obj = [float(x) for x in re.findall(r"objective after epoch \d+: (\S+)", out)]
    assert len(obj) == ITERS and (np.diff(obj) < 0).all(), obj
    raw = open(dump, "rb").read()
    U, I, nnz, k = (int(x) for x in np.frombuffer(raw, np.uint64, 4))
    assert k == K
    off = 32
    ptr = np.frombuffer(raw, np.int64, U + 1, off); off += 8 * (U + 1)
    col = np.frombuffer(raw, np.uint32, nnz, off); off += 4 * nnz
    w = np.frombuffer(raw, np.float32, nnz, off); off += 4 * nnz
    X = np.frombuffer(raw, np.float32, U * K, off).reshape(U, K); off += 4 * U * K
    Y = np.frombuffer(raw, np.float32, I * K, off).reshape(I, K); off += 4 * I * K
    assert off == len(raw) and ptr[-1] == nnz and set(np.unique(w)) == {1.0, 2.0, 3.0, 4.0, 5.0}
    m = cdae_amd.WRMF(cdae_amd.WRMFConfig(lambda_=1.0, scalar=5.0, num_dim=K, cg_steps=3))
    m.set_interactions(U, I, ptr, col)
    m.set_confidence(w)
    m.init_params(SEED)
    for _ in range(ITERS):
        m.train_one_iteration()
    ex, ey = ar.err(m.get(P_WU), X), ar.err(m.get(P_W), Y)
    print(f"host layer against the binding: users {ex:.3e} items {ey:.3e}")
    assert ex < ar.BOUND_GPU and ey < ar.BOUND_GPU
    total = sum(m.objective())
    assert abs(total - obj[-1]) <= 1e-9 * total
    m.close()
