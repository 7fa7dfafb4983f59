"""CPU: the WARP entry points are additions under ABI 12 — declared in include/cdae_hip.h, exported by the built library, bound by
cdae_amd.binding, wrapped by cdae_amd.WARP — and the refusals that are decided before a device is looked for.  No compute is attempted."""
import ctypes as C
import inspect
import os
import re

import cdae_amd
from cdae_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cdae_hip_create_warp": ["cfg", "device_id", "out"],
       "cdae_hip_warp_search": ["h", "seed", "epoch", "pos_begin", "pos_end", "out_item", "out_cnt", "out_margin", "count"],
       "cdae_hip_warp_record_choices": ["h", "on"],
       "cdae_hip_warp_choices": ["h", "out_item", "out_cnt", "count"]}


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
    m = re.search(r"typedef struct cdae_warp_config \{(.*?)\} cdae_warp_config;", code, flags=re.S)
    assert m
    fields = [tuple(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == [("uint32_t", "struct_size"), ("uint32_t", "num_dim"), ("uint32_t", "num_neg"), ("uint32_t", "loss_type"),
                      ("uint32_t", "using_adagrad"), ("uint32_t", "batch_users"), ("double", "lambda"), ("double", "learn_rate")]
    assert [n for n, _ in binding._WarpConfig._fields_] == ["struct_size", "num_dim", "num_neg", "loss_type", "using_adagrad", "batch_users",
                                                            "lambda_", "learn_rate"]
    assert C.sizeof(binding._WarpConfig) == 40
    assert re.search(r"#define\s+CDAE_WARP_MAX_TRY\s+500u\b", code) and cdae_amd.WARP_MAX_TRY == 500 and cdae_amd.WARP_NONE == 0xFFFFFFFF
    kernels = open(os.path.join(ROOT, "cdae_amd", "csrc", "cdae_warp_host.h")).read()
    assert re.search(r"WARP_MAX_TRY\s*=\s*500u\b", kernels)


def test_the_python_class():
    assert issubclass(cdae_amd.WARP, cdae_amd.MF)
    cfg = cdae_amd.WARPConfig()                        # the reference's defaults (warp.hpp:12-23)
    assert (cfg.learn_rate, cfg.lambda_, cfg.lt, cfg.num_dim, cfg.num_neg, cfg.using_adagrad, cfg.batch_users) == (0.1, 0.1, cdae_amd.HINGE, 10, 5, True, 1)
    sig = inspect.signature(binding.WARP.search)
    assert list(sig.parameters)[1:] == ["seed", "epoch", "pos_begin", "pos_end", "with_margin"]
    assert sig.parameters["pos_begin"].default == 0 and sig.parameters["pos_end"].default is None and sig.parameters["with_margin"].default is False
    assert list(inspect.signature(binding.WARP.record_choices).parameters)[1:] == ["on"]
    assert list(inspect.signature(binding.WARP.choices).parameters)[1:] == []
    for inherited in ("recommend_all", "eval_topn", "similar_items"):
        assert getattr(binding.WARP, inherited) is getattr(binding.CDAE, inherited)


def test_refusals_that_need_no_device(built):
    lib = cdae_amd.load_library()

    def refused(rc, *words):
        msg = lib.cdae_hip_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), msg

    h = C.c_void_p()
    refused(lib.cdae_hip_create_warp(None, 0, C.byref(h)), "null argument")
    good = dict(struct_size=C.sizeof(binding._WarpConfig), num_dim=10, num_neg=5, loss_type=3, using_adagrad=1, batch_users=1, lambda_=0.1, learn_rate=0.1)
    refused(lib.cdae_hip_create_warp(C.byref(binding._WarpConfig(**good)), 0, None), "null argument")
    refused(lib.cdae_hip_create_warp(C.byref(binding._WarpConfig(**{**good, "struct_size": 32})), 0, C.byref(h)), "cdae_warp_config size mismatch")
    for lt in (4, 6, 7):                               # SQUARED_HINGE, LOGM, nothing: not among mf_loss_grad's five
        refused(lib.cdae_hip_create_warp(C.byref(binding._WarpConfig(**{**good, "loss_type": lt})), 0, C.byref(h)), "loss_type", "unsupported")
    refused(lib.cdae_hip_create_warp(C.byref(binding._WarpConfig(**{**good, "num_neg": 0})), 0, C.byref(h)), "num_neg")
    refused(lib.cdae_hip_create_warp(C.byref(binding._WarpConfig(**{**good, "num_dim": 513})), 0, C.byref(h)), "num_dim")
    assert not h.value
    refused(lib.cdae_hip_warp_search(None, 0, 0, 0, 0, None, None, None, 0), "set_interactions")
    refused(lib.cdae_hip_warp_record_choices(None, 1), "set_interactions")
    refused(lib.cdae_hip_warp_choices(None, None, None, 0), "set_interactions")
