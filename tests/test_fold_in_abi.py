"""CPU: the fold-in entry points (cdae_hip_fold_in_rows, cdae_hip_set_guest_nodes, cdae_hip_guest_nodes) and CDAE_GUEST_USER are
additions under ABI 12 (the version unchanged) — declared in include/cdae_hip.h, exported by the built library, bound by cdae_amd.binding.  No compute is
attempted here."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cdae_amd
from cdae_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cdae_hip_fold_in_rows", "cdae_hip_set_guest_nodes", "cdae_hip_guest_nodes")


def header():
    return open(os.path.join(ROOT, "include", "cdae_hip.h")).read()


def test_the_library_exports_the_three_symbols(built):
    lib = cdae_amd.load_library()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in binding.EXPORTS
        assert getattr(lib, s).argtypes == binding.EXPORTS[s][1]
    assert len(binding.EXPORTS["cdae_hip_fold_in_rows"][1]) == 14 and len(binding.EXPORTS["cdae_hip_set_guest_nodes"][1]) == 6
    assert binding.EXPORTS["cdae_hip_guest_nodes"] == (C.c_uint64, [C.c_void_p])
    assert lib.cdae_hip_guest_nodes(None) == 0


def test_the_header_declares_them_under_abi_12(built):
    hdr = header()
    assert "#define CDAE_HIP_ABI_VERSION 12" in hdr and cdae_amd.load_library().cdae_hip_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW[:2]:
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
    assert re.search(r"\buint64_t\s+cdae_hip_guest_nodes\s*\(\s*const\s+cdae_hip_t\s*\*", code)
    assert re.search(r"#define\s+CDAE_GUEST_USER\(i\)\s+\(0x80000000u\s*\|\s*\(uint32_t\)\(i\)\)", code)
    version_comment = hdr[:hdr.index("#define CDAE_HIP_ABI_VERSION")]
    assert any("also under 12, the version unchanged" in line and NEW[0] in line for line in version_comment.splitlines())
    assert all(s in version_comment for s in NEW) and "CDAE_GUEST_USER" in version_comment
    # the mapping table's row
    table = hdr[:hdr.index("Conventions:")]
    assert re.search(r"train_one_user_corruption with the shared parameters frozen\s*\n\s*\*\s+cdae\.hpp:198-358\s+cdae_hip_fold_in_rows", table)


def test_guest_user_sets_the_top_bit():
    assert cdae_amd.GUEST_USER(0) == 0x80000000 and cdae_amd.GUEST_USER(5) == 0x80000005
    g = cdae_amd.GUEST_USER(np.arange(3))
    assert g.dtype == np.uint32 and g.tolist() == [0x80000000, 0x80000001, 0x80000002]
    assert cdae_amd.GUEST_USER(0x7FFFFFFE) != cdae_amd.NO_USER
    for bad in (-1, 0x7FFFFFFF):                                      # 0x7FFFFFFF would be NO_USER
        with pytest.raises(ValueError):
            cdae_amd.GUEST_USER(bad)


def test_the_python_class_has_the_methods():
    f = inspect.signature(binding.CDAE.fold_in_rows)
    assert list(f.parameters)[1:] == ["row_ptr", "col", "uids", "seed", "epoch_begin", "n_epochs", "stream_id_base", "install",
                                      "with_accumulators"]
    assert f.parameters["uids"].default is None and f.parameters["n_epochs"].default == 10
    assert all(f.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(f.parameters)[4:])
    assert [f.parameters[k].default for k in ("seed", "epoch_begin", "stream_id_base", "install", "with_accumulators")] == [0, 0, 0, False, False]
    g = inspect.signature(binding.CDAE.set_guest_nodes)
    assert list(g.parameters)[1:] == ["wu", "wu_ag", "uu", "uu_ag"] and all(g.parameters[k].default is None for k in ("wu_ag", "uu", "uu_ag"))
    assert isinstance(binding.CDAE.num_guest_nodes, property)
