"""CPU: the FISM entry points are additions under ABI 12 — declared in include/cdae_hip.h, exported by the built library, bound by
cdae_amd.binding, wrapped by cdae_amd.FISM — and the refusals that are decided before a device is looked for.  No compute is attempted."""
import ctypes as C
import inspect
import os
import re

import cdae_amd
from cdae_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cdae_hip_create_fism": ["cfg", "device_id", "out"],
       "cdae_hip_fism_plan": ["h", "resident_rows", "window_instances"],
       "cdae_hip_fism_set_resident": ["h", "allow"]}


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
    assert "cdae_fism_config" in version_comment and "the version unchanged" in version_comment


def test_the_config_struct_is_the_headers():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"typedef struct cdae_fism_config \{(.*?)\} cdae_fism_config;", code, flags=re.S)
    assert m
    fields = [tuple(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == [("uint32_t", "struct_size"), ("uint32_t", "num_dim"), ("uint32_t", "num_neg"), ("uint32_t", "loss_type"),
                      ("uint32_t", "using_adagrad"), ("uint32_t", "using_bias_term"), ("uint32_t", "batch_users"), ("uint32_t", "reserved"),
                      ("double", "lambda"), ("double", "learn_rate"), ("double", "alpha")]
    assert [n for n, _ in binding._FismConfig._fields_] == ["struct_size", "num_dim", "num_neg", "loss_type", "using_adagrad", "using_bias_term",
                                                            "batch_users", "reserved", "lambda_", "learn_rate", "alpha"]
    assert C.sizeof(binding._FismConfig) == 56 and binding._FismConfig.lambda_.offset == 32 and binding._FismConfig.alpha.offset == 48
    host = open(os.path.join(ROOT, "cdae_amd", "csrc", "cdae_fism_host.h")).read()
    import fism_ref
    for name, value in (("FISM_WAVES", fism_ref.WAVES), ("FISM_RESIDENT_FLOATS", fism_ref.RESIDENT_FLOATS), ("FISM_RESIDENT_SLOTS", fism_ref.RESIDENT_SLOTS), ("FISM_WINDOW_INSTANCES", fism_ref.WINDOW_INSTANCES)):
        assert re.search(name + r"\s*=\s*" + str(value) + r"u\b", host), name


def test_the_python_class():
    assert issubclass(cdae_amd.FISM, cdae_amd.MF)
    cfg = cdae_amd.FISMConfig()                        # the reference's defaults (fism.hpp:8-20), SGDConfig's learn rate
    assert (cfg.learn_rate, cfg.lambda_, cfg.lt, cfg.num_dim, cfg.num_neg, cfg.alpha, cfg.using_bias_term, cfg.using_adagrad, cfg.batch_users) == (
        0.1, 0.01, cdae_amd.SQUARE, 10, 5, 1.0, True, True, 1)
    assert list(inspect.signature(binding.FISM.plan).parameters)[1:] == []
    assert list(inspect.signature(binding.FISM.set_resident).parameters)[1:] == ["allow"]
    for served in ("recommend_all", "eval_topn", "recommend_rows", "eval_topn_rows", "score_rows", "full_rank_rows", "recommend_rows_filtered",
                   "similar_items"):
        assert getattr(binding.FISM, served) is getattr(binding.CDAE, served)
    assert "FISM" in cdae_amd.__doc__


def test_refusals_that_need_no_device(built):
    lib = cdae_amd.load_library()

    def refused(rc, *words):
        msg = lib.cdae_hip_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), msg

    h = C.c_void_p()
    refused(lib.cdae_hip_create_fism(None, 0, C.byref(h)), "null argument")
    good = dict(struct_size=C.sizeof(binding._FismConfig), num_dim=10, num_neg=5, loss_type=0, using_adagrad=1, using_bias_term=1, batch_users=1,
                reserved=0, lambda_=0.01, learn_rate=0.1, alpha=1.0)

    def create(**change):
        return lib.cdae_hip_create_fism(C.byref(binding._FismConfig(**{**good, **change})), 0, C.byref(h))

    refused(lib.cdae_hip_create_fism(C.byref(binding._FismConfig(**good)), 0, None), "null argument")
    refused(create(struct_size=48), "cdae_fism_config size mismatch")
    refused(create(batch_users=2), "batch_users 2", "block schedule", "not built")
    refused(create(loss_type=3), "HINGE", "refused", "jumps")
    refused(create(loss_type=1), "LOGISTIC", "refused", "CHECK-aborts")
    for lt in (4, 6, 7):
        refused(create(loss_type=lt), "loss_type", "unsupported")
    refused(create(num_dim=0), "num_dim")
    refused(create(num_dim=513), "num_dim")
    refused(create(num_neg=0), "num_neg")
    refused(create(alpha=-1.0), "alpha")
    assert not h.value
    refused(lib.cdae_hip_fism_plan(None, None, None), "null handle")
    refused(lib.cdae_hip_fism_set_resident(None, 1), "null handle")
