"""CPU: cdae_hip_full_rank_rows (the exact rank of named items among ALL unrated items of a row) is an addition under ABI 12 —
declared in include/cdae_hip.h, exported by the built library, bound by cdae_amd.binding.  No compute is attempted here."""
import ctypes as C
import inspect
import os
import re

import cdae_amd
from cdae_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "cdae_hip_full_rank_rows"


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
    assert m
    params = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["h", "n_rows", "uids", "row_ptr", "col", "target_row_ptr", "target_col", "out_ranks", "out_scores"]
    version_comment = hdr[:hdr.index("#define CDAE_HIP_ABI_VERSION")]
    assert len([line for line in version_comment.splitlines() if "added under 12" in line]) == 2      # (what the earlier additions pin)
    assert any("also under 12, the version unchanged" in line and NEW in line for line in version_comment.splitlines())
    assert re.search(r"CDAE::recommend[^\n]*\n[^\n]*cdae\.hpp:162-196\s+" + NEW, version_comment)
    assert re.search(r"CDAE::get_output_values\s+cdae\.hpp:418-426\s+cdae_hip_score_rows", version_comment)


def test_the_python_class_has_the_methods():
    sig = inspect.signature(binding.CDAE.full_rank_rows)
    assert list(sig.parameters)[1:] == ["row_ptr", "col", "target_ptr", "target_col", "uids", "with_scores"]
    assert sig.parameters["uids"].default is None and sig.parameters["with_scores"].default is False
    sig = inspect.signature(binding.CDAE.eval_ranking_rows)
    assert list(sig.parameters)[1:] == ["row_ptr", "col", "target_ptr", "target_col", "uids", "ks"]
    assert sig.parameters["ks"].default == (1, 5, 10, 20, 50, 100)
    assert binding.MF.full_rank_rows is binding.CDAE.full_rank_rows   # (inherited: the library refuses an IMF / BPR handle)
    assert cdae_amd.ranking_metrics is cdae_amd.metrics.ranking_metrics
    sig = inspect.signature(cdae_amd.ranking_metrics)
    assert list(sig.parameters) == ["target_ptr", "ranks", "n_unrated", "ks"] and sig.parameters["ks"].default == (1, 5, 10, 20, 50, 100)
