"""CPU: the WRMF confidence-weight and objective entry points are additions under ABI 12 — declared in include/cdae_hip.h, exported by
the built library, bound by cdae_amd.binding, wrapped by cdae_amd.WRMF.  No compute is attempted."""
import inspect
import os
import re

import cdae_amd
from cdae_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cdae_hip_als_set_confidence": ["h", "w", "count"],
       "cdae_hip_als_solve_rows_weighted": ["h", "n_rows", "row_ptr", "col", "w", "x0", "cg_steps", "out_x"],
       "cdae_hip_als_objective": ["h", "out2"]}


def header():
    return open(os.path.join(ROOT, "include", "cdae_hip.h")).read()


def test_the_library_exports_the_symbols(built):
    lib = cdae_amd.load_library()
    for name, args in NEW.items():
        assert hasattr(lib, name) and name in binding.EXPORTS, name
        assert getattr(lib, name).argtypes == binding.EXPORTS[name][1]
        assert len(binding.EXPORTS[name][1]) == len(args)


def test_the_header_declares_them_under_abi_12(built):
    hdr = header()
    assert "#define CDAE_HIP_ABI_VERSION 12" in hdr and cdae_amd.load_library().cdae_hip_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    version_comment = hdr[:hdr.index("#define CDAE_HIP_ABI_VERSION")]
    for name, args in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, name
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == args
        assert name in version_comment
    assert version_comment.count("also under 12, the version unchanged") >= 2
    # the binary entry point and the config struct are the ones they were
    assert re.search(r"int cdae_hip_als_solve_rows\(cdae_hip_t\* h, uint64_t n_rows, const int64_t\* row_ptr, const uint32_t\* col, const float\* x0,", code)


def test_the_python_methods():
    assert list(inspect.signature(binding.WRMF.set_confidence).parameters)[1:] == ["w"]
    assert list(inspect.signature(binding.WRMF.objective).parameters)[1:] == []
    sig = inspect.signature(binding.WRMF.solve_rows_weighted)
    assert list(sig.parameters)[1:] == ["row_ptr", "col", "weights", "x0", "cg_steps"] and sig.parameters["weights"].default is None
    assert list(inspect.signature(binding.WRMF.solve_rows).parameters)[1:] == ["row_ptr", "col", "x0", "cg_steps"]      # unchanged
