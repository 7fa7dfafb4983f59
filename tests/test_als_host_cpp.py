"""The host C++ layer's libcf::WRMF (src/model/recsys/wrmf.hpp) over cdae_hip_create_als.
CPU: src/wrmf_check.cpp takes the methods' addresses with the documented signatures, compiles and links (make -C src check, as
tests/test_host_cpp.py builds src/host_check.cpp).  GPU: the same binary fits a small data set through Solver<WRMF> with TOPN and
checks the epoch, a half-step, solve_rows and the served lists."""
import os
import subprocess

import pytest

from test_host_cpp import BUILD, ROOT, run, write_ratings


@pytest.fixture(scope="module")
def wrmf_check(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "src"), "-s", "check"])
    return os.path.join(BUILD, "wrmf_check")


def test_the_class_compiles_and_links(wrmf_check, tmp_path):
    rc, out = run([wrmf_check], tmp_path)
    assert rc == 0 and "wrmf check OK (compiled)" in out, out


@pytest.mark.gpu
def test_wrmf_through_the_host_layer(wrmf_check, tmp_path):
    write_ratings(tmp_path / "ratings.txt")
    rc, out = run([wrmf_check, "--run=true", f"--input_file={tmp_path / 'ratings.txt'}"], tmp_path, env={"CDAE_SEED": "7"})
    assert rc == 0, out
    assert "wrmf OK" in out
