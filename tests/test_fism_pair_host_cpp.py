"""CPU: the host arithmetic of a pairwise FISM handle (cdae_amd/csrc/cdae_fism_host.h: the pair count and the launch windows in pairs)
against a Python restatement of them.  src/fism_check.cpp pins the same figures; tests/test_fism_host_cpp.py builds and runs it, plain
(with libcf::FISMP) and under the sanitizers."""
import os

import numpy as np

import fism_pair_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "src")


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
    """the figures src/fism_check.cpp expects of the header in pairs, from the Python restatement; and the windows of the GPU test's data"""
    ptr = np.array([0, 3, 3, 10, 11, 411, 412])
    assert pair_count(ptr, 0, 6, 5) == 2060 and pair_count(ptr, 1, 2, 5) == 0 and pair_count(ptr, 2, 4, 12) == 96
    assert pair_windows(ptr, 0, 6, 5, 55) == [0, 4, 5, 6]
    assert pair_windows(ptr, 0, 6, 5, 54) == [0, 3, 4, 5, 6]
    assert pair_windows(ptr, 0, 6, 5, 2005) == [0, 4, 6]
    assert pair_windows(ptr, 2, 2, 5, 55) == [2]
    src = open(os.path.join(SRC, "fism_check.cpp")).read()
    for text in ("412u * 5u", "8u * 12u", "w[1] == 4 && w[2] == 5 && w[3] == 6", "w2[1] == 3 && w2[2] == 4 && w2[3] == 5 && w2[4] == 6",
                 "w3[1] == 4 && w3[2] == 6"):
        assert text in src, text
    win = pr.fixture_data("win")
    c = pr.case("win")
    cuts = pair_windows(win.train_ptr, 0, win.num_users, c[3], pr.WINDOW_INSTANCES)
    assert cuts == [0, 22, 24] and pair_count(win.train_ptr, 0, win.num_users, c[3]) == 429 * 5 > pr.WINDOW_INSTANCES    # two launches for "win"
    d40 = pr.fixture_data("d40")
    assert pair_windows(d40.train_ptr, 0, d40.num_users, 5, pr.WINDOW_INSTANCES) == [0, d40.num_users]
