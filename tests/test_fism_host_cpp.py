"""CPU: the host arithmetic of a FISM handle of either kind (cdae_amd/csrc/cdae_fism_host.h: the scale table against pow, the residency
plan, the step counts and launch windows in instances and in pairs) checked by src/fism_check.cpp — a stand-alone program built plain
(with libcf::FISM and libcf::FISMP, which must compile and link against the library) and, without the library, under the address and
undefined-behaviour sanitizers (`make sanitize`) — and the same functions against tests/fism_ref.py's constants."""
import os
import re
import subprocess

import numpy as np

import fism_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "src")


def test_fism_check_builds_with_the_libcf_header_and_passes(built):
    subprocess.check_call(["make", "-C", SRC, "-s", os.path.join(ROOT, "build", "fism_check")])
    run = subprocess.run([os.path.join(ROOT, "build", "fism_check")], capture_output=True, text=True, timeout=120)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out
    assert "fism check OK (compiled)" in out and "fism pair check OK (compiled)" in out and "fism_check:" not in out, out
    hpp = open(os.path.join(SRC, "model", "recsys", "fism_pair.hpp")).read()
    assert "class FISMP : public FISM" in hpp and "struct FISMPConfig" in hpp and "cdae_hip_create_fism_pair" in hpp


def test_fism_check_under_the_sanitizers():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run(["make", "-C", SRC, "-s", "sanitize"], capture_output=True, text=True, env=env, timeout=300)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out
    assert "fism check OK (host arithmetic)" in run.stdout and "warp check OK (host arithmetic)" in run.stdout, out
    assert "fism pair check OK (host arithmetic)" in run.stdout, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert re.search(r"-fsanitize=address,undefined[^\n]*-DFISM_CHECK_HOST_ONLY[^\n]*fism_check\.cpp", mk)


def test_the_reference_states_the_same_plan():
    """fism_ref's scale table is the header's (fp64 pow rounded once), its resident_rows the plan fism_check pins"""
    for alpha in (0.0, 0.5, 1.0):
        s = fr.scale_table(1500, alpha)
        assert s[0] == 0.0 and s[1] == 1.0
        n = np.arange(1, 1501, dtype=np.float64)
        np.testing.assert_array_equal(s[1:], np.power(n, -alpha).astype(np.float32).astype(np.float64))
    assert [fr.resident_rows(K) for K in (1, 64, 65, 128, 129, 256, 257, 512)] == [256, 256, 256, 256, 128, 128, 64, 64]
