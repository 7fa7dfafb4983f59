"""CPU: cdae_hip_similar_items (batched top-k item neighbours by dot product or cosine) is an addition under ABI 12 — declared in
include/cdae_hip.h, exported by the built library, bound by cdae_amd.binding.  No compute is attempted."""
import inspect
import os
import re

import cdae_amd
from cdae_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "cdae_hip_similar_items"


def header():
    return open(os.path.join(ROOT, "include", "cdae_hip.h")).read()


def test_the_library_exports_the_symbol(built):
    lib = cdae_amd.load_library()
    assert hasattr(lib, NEW) and NEW in binding.EXPORTS
    assert getattr(lib, NEW).argtypes == binding.EXPORTS[NEW][1]
    assert len(binding.EXPORTS[NEW][1]) == 13


def test_the_header_declares_it_under_abi_12(built):
    hdr = header()
    assert "#define CDAE_HIP_ABI_VERSION 12" in hdr and cdae_amd.load_library().cdae_hip_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + NEW + r"\s*\(([^)]*)\)", code)
    assert m, NEW
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["h", "n_queries", "query_items", "table", "metric", "exclude_self", "excl_row_ptr", "excl_col", "allow_items", "n_allow",
                     "topk", "out_ids", "out_scores"]
    version_comment = hdr[:hdr.index("#define CDAE_HIP_ABI_VERSION")]
    assert "the version unchanged" in version_comment and NEW in version_comment


def test_the_constants_are_the_headers():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name, value in (("ITEMS_OUTPUT", 0), ("ITEMS_INPUT", 1), ("SIM_DOT", 0), ("SIM_COSINE", 1)):
        assert re.search(rf"#define\s+CDAE_{name}\s+{value}u\b", code), name
        assert getattr(cdae_amd, name) == value


def test_the_python_class_has_the_method():
    sig = inspect.signature(binding.CDAE.similar_items)
    assert list(sig.parameters)[1:] == ["items", "topk", "metric", "table", "exclude_self", "exclude", "allow", "with_scores"]
    p = sig.parameters
    assert p["items"].default is inspect.Parameter.empty and p["topk"].default == 10 and p["metric"].default == "cosine"
    assert p["table"].default == "output" and p["exclude_self"].default is True and p["exclude"].default is None
    assert p["allow"].default is None and p["with_scores"].default is False
    assert binding.MF.similar_items is binding.CDAE.similar_items            # IMF / BPR handles inherit it
