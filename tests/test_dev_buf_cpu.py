"""CPU: DevBuf, the owner of every device allocation of a handle (cdae_amd/csrc/cdae_dev_buf.h), over malloc / free.
tests/native/dev_buf_cpu.cpp defines the header's memory seam with a live-block counter and failure switches and asserts what the
library relies on: ensure is grow-only, alloc is exact and never null, a failed acquire or release leaves the buffer empty, moves
and std::swap of arrays move ownership, destruction releases, nothing is live at the end.  Compiled with the address and
undefined-behaviour sanitizers and run as a child process: it passes only if the program exits 0 and neither sanitizer speaks.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_buf_under_the_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "dev_buf_cpu.cpp")
    exe = str(tmp_path / "dev_buf_cpu")
    # (the runtimes are linked statically: the program then runs wherever a library is preloaded into every process)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", src, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out
    assert "dev_buf check OK" in run.stdout, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
