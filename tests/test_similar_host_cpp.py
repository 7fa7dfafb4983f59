"""The host C++ layer's similar_items (src/model/recsys/cdae.hpp, imf.hpp) over cdae_hip_similar_items.
CPU: src/similar_check.cpp takes the methods' addresses with the documented signature, compiles and links (make -C src check, as
tests/test_host_cpp.py builds src/host_check.cpp).  GPU: the same binary trains a small CDAE and checks the item-page recipes of
INTEGRATION.md — an item page, hide what was shown, more like this within a category — against the whole lists."""
import os
import subprocess

import pytest

from test_host_cpp import BUILD, ROOT, run, write_ratings


@pytest.fixture(scope="module")
def similar_check(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "src"), "-s", "check"])
    return os.path.join(BUILD, "similar_check")


def test_the_methods_compile_and_link(similar_check, tmp_path):
    rc, out = run([similar_check], tmp_path)
    assert rc == 0 and "similar check OK (compiled)" in out, out


@pytest.mark.gpu
def test_the_item_page_recipes_through_the_host_layer(similar_check, tmp_path):
    write_ratings(tmp_path / "ratings.txt")
    rc, out = run([similar_check, "--run=true", f"--input_file={tmp_path / 'ratings.txt'}"], tmp_path,
                  env={"CDAE_SEED": "7", "CDAE_BATCH_USERS": "64"})
    assert rc == 0, out
    assert "similar_items OK" in out
