"""CPU: cdae_hip_create_fism_pair is an addition under ABI 12 — declared in include/cdae_hip.h, exported by the built library, bound by
cdae_amd.binding, wrapped by cdae_amd.FISMP — on the unchanged cdae_fism_config, and the refusals that are decided before a device is
looked for.  No compute is attempted."""
import ctypes as C
import dataclasses
import os
import re

import cdae_amd
from cdae_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARGS = "cdae_hip_create_fism_pair", ["cfg", "device_id", "out"]


def header():
    return open(os.path.join(ROOT, "include", "cdae_hip.h")).read()


def test_the_library_exports_the_symbol(built):
    lib = cdae_amd.load_library()
    assert hasattr(lib, NAME) and NAME in binding.EXPORTS
    assert getattr(lib, NAME).argtypes == binding.EXPORTS[NAME][1] == binding.EXPORTS["cdae_hip_create_fism"][1]
    assert len(binding.EXPORTS[NAME][1]) == len(ARGS)


def test_the_header_declares_it_under_abi_12(built):
    hdr = header()
    assert "#define CDAE_HIP_ABI_VERSION 12" in hdr and cdae_amd.load_library().cdae_hip_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", code)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ARGS
    assert "const cdae_fism_config*" in m.group(1)
    version_comment = hdr[:hdr.index("#define CDAE_HIP_ABI_VERSION")]
    line = next(part for part in version_comment.split("also under 12") if NAME in part)
    assert "the version unchanged" in line and "nothing existing changed" in line


def test_the_config_struct_is_unchanged():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"typedef struct cdae_fism_config \{(.*?)\} cdae_fism_config;", code, flags=re.S)
    fields = [tuple(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == [("uint32_t", "struct_size"), ("uint32_t", "num_dim"), ("uint32_t", "num_neg"), ("uint32_t", "loss_type"),
                      ("uint32_t", "using_adagrad"), ("uint32_t", "using_bias_term"), ("uint32_t", "batch_users"), ("uint32_t", "reserved"),
                      ("double", "lambda"), ("double", "learn_rate"), ("double", "alpha")]
    assert C.sizeof(binding._FismConfig) == 56 and binding._FismConfig.lambda_.offset == 32 and binding._FismConfig.alpha.offset == 48
    assert "cdae_fism_pair_config" not in code                 # no second struct


def test_the_python_classes():
    assert issubclass(cdae_amd.FISMP, cdae_amd.FISM) and issubclass(cdae_amd.FISMPConfig, cdae_amd.FISMConfig)
    cfg = cdae_amd.FISMPConfig()                       # the reference's defaults (fism_pair.hpp), SGDConfig's learn rate
    assert (cfg.learn_rate, cfg.lambda_, cfg.lt, cfg.num_dim, cfg.num_neg, cfg.alpha, cfg.using_bias_term, cfg.using_adagrad, cfg.batch_users) == (
        0.1, 0.01, cdae_amd.SQUARE, 10, 5, 1.0, True, True, 1)
    assert [f.name for f in dataclasses.fields(cfg)] == [f.name for f in dataclasses.fields(cdae_amd.FISMConfig())]
    assert binding.FISMP._create == NAME and binding.FISM._create == "cdae_hip_create_fism"
    for same in ("plan", "set_resident", "recommend_all", "eval_topn", "recommend_rows", "eval_topn_rows", "score_rows", "full_rank_rows",
                 "recommend_rows_filtered", "similar_items", "train_users", "train_one_iteration"):
        assert getattr(binding.FISMP, same) is getattr(binding.FISM, same), same
    assert "FISMP" in cdae_amd.__doc__

    class Rows:                                            # _batch_examples counts pairs
        _row_ptr = [0, 3, 3, 10]
        cfg = cdae_amd.FISMPConfig(num_neg=7)
    assert binding.FISMP._batch_examples(Rows, 0, 3) == 70 and binding.FISMP._batch_examples(Rows, 1, 1) == 0
    assert binding.FISM._batch_examples(Rows, 0, 3) == 80


def test_refusals_that_need_no_device(built):
    lib = cdae_amd.load_library()

    def refused(rc, *words):
        msg = lib.cdae_hip_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), msg

    h = C.c_void_p()
    create_pair = getattr(lib, NAME)
    refused(create_pair(None, 0, C.byref(h)), "null argument")
    good = dict(struct_size=C.sizeof(binding._FismConfig), num_dim=10, num_neg=5, loss_type=0, using_adagrad=1, using_bias_term=1, batch_users=1,
                reserved=0, lambda_=0.01, learn_rate=0.1, alpha=1.0)

    def create(**change):
        return create_pair(C.byref(binding._FismConfig(**{**good, **change})), 0, C.byref(h))

    refused(create_pair(C.byref(binding._FismConfig(**good)), 0, None), "null argument")
    refused(create(struct_size=48), "cdae_fism_config size mismatch")
    refused(create(batch_users=2), "batch_users 2", "block schedule", "not built")
    refused(create(loss_type=5), "CROSS_ENTROPY", "refused", "LOG's")
    refused(create(loss_type=3), "HINGE", "refused", "jumps")
    refused(create(loss_type=1), "LOGISTIC", "refused", "CHECK-aborts")
    for lt in (4, 6, 7):
        refused(create(loss_type=lt), "loss_type", "unsupported")
    refused(create(num_dim=0), "num_dim")
    refused(create(num_dim=513), "num_dim")
    refused(create(num_neg=0), "num_neg")
    refused(create(alpha=-1.0), "alpha")
    assert not h.value
