"""CPU: the host arithmetic of a pairwise FISM handle (cdae_amd/csrc/cdae_fism_host.h: the pair count and the launch windows in pairs)
checked by src/fism_pair_check.cpp — a stand-alone program built plain (with libcf::FISMP, which must compile and link against the
library) and, without the library, under the address and undefined-behaviour sanitizers (`make sanitize`) — and the same functions
against a Python restatement."""
import os
import re
import subprocess

import numpy as np

import fism_pair_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "src")


def test_fism_pair_check_builds_with_the_libcf_header_and_passes(built):
    subprocess.check_call(["make", "-C", SRC, "-s", os.path.join(ROOT, "build", "fism_pair_check")])
    run = subprocess.run([os.path.join(ROOT, "build", "fism_pair_check")], capture_output=True, text=True, timeout=120)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out
    assert "fism pair check OK (compiled)" in out and "fism_pair_check:" not in out, out
    hpp = open(os.path.join(SRC, "model", "recsys", "fism_pair.hpp")).read()
    assert "class FISMP : public FISM" in hpp and "struct FISMPConfig" in hpp and "cdae_hip_create_fism_pair" in hpp


def test_fism_pair_check_under_the_sanitizers():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run(["make", "-C", SRC, "-s", "sanitize"], capture_output=True, text=True, env=env, timeout=300)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out
    assert "fism pair check OK (host arithmetic)" in run.stdout, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert re.search(r"-fsanitize=address,undefined[^\n]*-DFISM_PAIR_CHECK_HOST_ONLY[^\n]*fism_pair_check\.cpp", mk)


def pair_count(ptr, a, b, num_neg):
    return int(ptr[b] - ptr[a]) * num_neg


def pair_windows(ptr, a, b, num_neg, cap):
    """users are taken while the window's pairs stay within cap, and always at least one"""
    cuts, u = [a], a
    while u < b:
        e = u + 1
        while e < b and pair_count(ptr, u, e + 1, num_neg) <= cap:
            e += 1
        cuts.append(e)
        u = e
    return cuts


def test_the_restatement_gives_what_the_program_pins():
    """the figures src/fism_pair_check.cpp expects of the header, from the Python restatement; and the windows of the GPU test's data"""
    ptr = np.array([0, 3, 3, 10, 11, 411, 412])
    assert pair_count(ptr, 0, 6, 5) == 2060 and pair_count(ptr, 1, 2, 5) == 0 and pair_count(ptr, 2, 4, 12) == 96
    assert pair_windows(ptr, 0, 6, 5, 55) == [0, 4, 5, 6]
    assert pair_windows(ptr, 0, 6, 5, 54) == [0, 3, 4, 5, 6]
    assert pair_windows(ptr, 0, 6, 5, 2005) == [0, 4, 6]
    assert pair_windows(ptr, 2, 2, 5, 55) == [2]
    src = open(os.path.join(SRC, "fism_pair_check.cpp")).read()
    for text in ("412u * 5u", "8u * 12u", "w[1] == 4 && w[2] == 5 && w[3] == 6", "w2[1] == 3 && w2[2] == 4 && w2[3] == 5 && w2[4] == 6",
                 "w3[1] == 4 && w3[2] == 6"):
        assert text in src, text
    win = pr.fixture_data("win")
    c = pr.case("win")
    cuts = pair_windows(win.train_ptr, 0, win.num_users, c[3], pr.WINDOW_INSTANCES)
    assert cuts == [0, 22, 24] and pair_count(win.train_ptr, 0, win.num_users, c[3]) == 429 * 5 > pr.WINDOW_INSTANCES    # two launches for "win"
    d40 = pr.fixture_data("d40")
    assert pair_windows(d40.train_ptr, 0, d40.num_users, 5, pr.WINDOW_INSTANCES) == [0, d40.num_users]
