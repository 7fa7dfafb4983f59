"""CPU: the WRMF / ALS entry points are additions under ABI 12 — declared in include/cdae_hip.h, exported by the built library, bound
by cdae_amd.binding, wrapped by cdae_amd.WRMF.  No compute is attempted."""
import ctypes as C
import inspect
import os
import re

import cdae_amd
from cdae_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cdae_hip_create_als": ["cfg", "device_id", "out"],
       "cdae_hip_als_half_step": ["h", "side"],
       "cdae_hip_als_solve_rows": ["h", "n_rows", "row_ptr", "col", "x0", "cg_steps", "out_x"],
       "cdae_hip_als_gram": ["h", "side", "out", "count"]}


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
    assert "the version unchanged" in version_comment


def test_the_config_struct_is_the_headers():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"typedef struct cdae_als_config \{(.*?)\} cdae_als_config;", code, flags=re.S)
    assert m
    fields = [tuple(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == [("uint32_t", "struct_size"), ("uint32_t", "num_dim"), ("uint32_t", "cg_steps"), ("uint32_t", "reserved"),
                      ("double", "lambda"), ("double", "alpha")]
    assert [n for n, _ in binding._AlsConfig._fields_] == ["struct_size", "num_dim", "cg_steps", "reserved", "lambda_", "alpha"]
    assert C.sizeof(binding._AlsConfig) == 32
    for name, value in (("ALS_USERS", 0), ("ALS_ITEMS", 1)):
        assert re.search(rf"#define\s+CDAE_{name}\s+{value}u\b", code), name
        assert getattr(cdae_amd, name) == value
    assert re.search(r"#define\s+CDAE_ALS_DEFAULT_CG_STEPS\s+3u\b", code)


def test_the_python_class():
    assert issubclass(cdae_amd.WRMF, cdae_amd.MF)
    cfg = cdae_amd.WRMFConfig()
    assert (cfg.lambda_, cfg.scalar, cfg.num_dim, cfg.cg_steps) == (0.01, 40.0, 10, 3)
    assert list(inspect.signature(binding.WRMF.half_step).parameters)[1:] == ["side"]
    assert list(inspect.signature(binding.WRMF.solve_rows).parameters)[1:] == ["row_ptr", "col", "x0", "cg_steps"]
    assert list(inspect.signature(binding.WRMF.train_one_iteration).parameters)[1:] == ["seed", "epoch"]
    for inherited in ("recommend_all", "eval_topn", "similar_items"):
        assert getattr(binding.WRMF, inherited) is getattr(binding.CDAE, inherited)
