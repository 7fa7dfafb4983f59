"""CPU: the batched rated-set entry points (cdae_hip_recommend_rows, cdae_hip_eval_topn_rows) are additions under ABI 12 — declared
in include/cdae_hip.h, exported by the built library, bound by cdae_amd.binding.  No compute is attempted here."""
import inspect
import os
import re

import cdae_amd
from cdae_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cdae_hip_recommend_rows", "cdae_hip_eval_topn_rows")


def header():
    return open(os.path.join(ROOT, "include", "cdae_hip.h")).read()


def test_the_library_exports_both_symbols(built):
    lib = cdae_amd.load_library()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in binding.EXPORTS
        assert getattr(lib, s).argtypes == binding.EXPORTS[s][1]
    assert len(binding.EXPORTS["cdae_hip_recommend_rows"][1]) == 8 and len(binding.EXPORTS["cdae_hip_eval_topn_rows"][1]) == 11


def test_the_header_declares_them_under_abi_12(built):
    hdr = header()
    assert "#define CDAE_HIP_ABI_VERSION 12" in hdr and cdae_amd.load_library().cdae_hip_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
    assert re.search(r"#define\s+CDAE_NO_USER\s+0xFFFFFFFFu", code)
    assert binding.NO_USER == cdae_amd.NO_USER == 0xFFFFFFFF
    version_comment = hdr[:hdr.index("#define CDAE_HIP_ABI_VERSION")]
    assert "added under 12" in version_comment and all(s in version_comment for s in NEW)


def test_the_python_class_has_the_two_methods():
    rec = inspect.signature(binding.CDAE.recommend_rows)
    assert list(rec.parameters)[1:] == ["row_ptr", "col", "uids", "topk", "with_scores"]
    assert rec.parameters["uids"].default is None and rec.parameters["topk"].default == 10 and rec.parameters["with_scores"].default is False
    ev = inspect.signature(binding.CDAE.eval_topn_rows)
    assert list(ev.parameters)[1:6] == ["row_ptr", "col", "target_ptr", "target_col", "uids"] and ev.parameters["topk"].default == 10
