"""CPU: cdae_hip_score_rows (get_output_values for many rows: scores and ranks of caller-supplied candidate sets) is an addition
under ABI 12 — declared in include/cdae_hip.h, exported by the built library, bound by cdae_amd.binding.  No compute is attempted here."""
import ctypes as C
import inspect
import os
import re

import cdae_amd
from cdae_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "cdae_hip_score_rows"


def header():
    return open(os.path.join(ROOT, "include", "cdae_hip.h")).read()


def test_the_library_exports_the_symbol(built):
    lib = cdae_amd.load_library()
    assert hasattr(lib, NEW) and NEW in binding.EXPORTS
    restype, argtypes = binding.EXPORTS[NEW]
    assert restype is C.c_int and len(argtypes) == 9
    assert argtypes == [C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
    assert getattr(lib, NEW).argtypes == argtypes


def test_the_header_declares_it_under_abi_12(built):
    hdr = header()
    assert "#define CDAE_HIP_ABI_VERSION 12" in hdr and cdae_amd.load_library().cdae_hip_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + NEW + r"\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 9
    for name in ("uids", "row_ptr", "col", "cand_row_ptr", "cand_col", "out_scores", "out_ranks"):
        assert re.search(r"\b" + name + r"\b", m.group(1)), name
    version_comment = hdr[:hdr.index("#define CDAE_HIP_ABI_VERSION")]
    added = [line for line in version_comment.splitlines() if "added under 12" in line]
    assert len(added) == 2 and NEW in added[1] and NEW not in added[0]
    assert re.search(r"CDAE::get_output_values\s+cdae\.hpp:418-426\s+" + NEW, version_comment)


def test_the_rank_cap_is_4096_in_the_header_and_in_the_binding():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"#define\s+CDAE_RANK_CANDIDATES_MAX\s+4096u\b", code)
    assert binding.RANK_CANDIDATES_MAX == cdae_amd.RANK_CANDIDATES_MAX == 4096


def test_the_python_class_has_the_method():
    sig = inspect.signature(binding.CDAE.score_rows)
    assert list(sig.parameters)[1:] == ["row_ptr", "col", "cand_ptr", "cand_col", "uids", "with_ranks"]
    assert sig.parameters["uids"].default is None and sig.parameters["with_ranks"].default is False
    assert binding.MF.score_rows is binding.CDAE.score_rows           # (inherited: the library refuses an IMF / BPR handle)
