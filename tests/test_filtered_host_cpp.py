"""The host C++ layer's recommend_rows_filtered (src/model/recsys/cdae.hpp) over cdae_hip_recommend_rows_filtered.
CPU: src/filtered_check.cpp takes the method's address with the documented signature, compiles and links (make -C src check, as
tests/test_host_cpp.py builds src/host_check.cpp).  GPU: the same binary trains a small CDAE and checks the three serving recipes of
INTEGRATION.md — category page, hide what was shown, buy it again — against recommend_rows."""
import os
import subprocess

import pytest

from test_host_cpp import BUILD, ROOT, run, write_ratings


@pytest.fixture(scope="module")
def filtered_check(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "src"), "-s", "check"])
    return os.path.join(BUILD, "filtered_check")


def test_the_method_compiles_and_links(filtered_check, tmp_path):
    rc, out = run([filtered_check], tmp_path)
    assert rc == 0 and "filtered check OK (compiled)" in out, out


@pytest.mark.gpu
def test_the_serving_recipes_through_the_host_layer(filtered_check, tmp_path):
    write_ratings(tmp_path / "ratings.txt")
    rc, out = run([filtered_check, "--run=true", f"--input_file={tmp_path / 'ratings.txt'}"], tmp_path,
                  env={"CDAE_SEED": "7", "CDAE_BATCH_USERS": "64"})
    assert rc == 0, out
    assert "recommend_rows_filtered OK" in out
