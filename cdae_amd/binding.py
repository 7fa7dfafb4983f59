"""ctypes binding of libcdae_hip.so (include/cdae_hip.h) and a host-side mirror of libcf::CDAE.

`CDAEConfig` / `CDAE` keep the field and method names of the reference's model class
(/root/reference/src/model/recsys/cdae.hpp:13-31, 36-196) so that parity tests read like the reference's
call sites (apps/yelp/yelp.cpp:168-199, src/solver/solver-inl.hpp:19,53,55).  There is NO CPU fallback:
constructing a CDAE without the HIP library or without a GPU raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CDAE_HIP_LIBRARY") or os.path.join(_HERE, "lib", "libcdae_hip.so")   # (developer builds: another .so of the same ABI)
# the -DCDAE_DEVELOPER build of the same sources (made by __graft_entry__.build()): the only library that reads the developer
# environment switches; loaded by the tests that flip one (developer_library() below), never by the product path
DEV_LIB_PATH = os.path.join(os.path.dirname(_HERE), "build", "libcdae_hip_dev.so")

# libcf::LossType values (/root/reference/src/model/loss.hpp:10-18)
SQUARE, LOGISTIC, LOG, HINGE, SQUARED_HINGE, CROSS_ENTROPY, LOGM = range(7)

P_W, P_W_AG, P_V, P_V_AG, P_WU, P_WU_AG, P_B, P_B_AG, P_BP, P_BP_AG, P_UU, P_UU_AG = range(12)
P_UB, P_UB_AG = 12, 13
P_COUNT = 14

PLAN_FUSED_DECODE, PLAN_GEMM2_TN, PLAN_ROWS_FUSED = 1, 2, 4     # cdae_hip_full_output_plan bits (include/cdae_hip.h)
IMF_DEFAULT_BATCH_USERS = 16   # CDAE_IMF_DEFAULT_BATCH_USERS / CDAE_BPR_DEFAULT_BATCH_USERS (include/cdae_hip.h): what an IMF / BPR handle created
BPR_DEFAULT_BATCH_USERS = 8    # with batch_users = 0 trains on a BASELINE-sized data set (cdae_hip_mf_default_batch_users); 1 on smaller ones
RANK_CANDIDATES_MAX = 4096     # CDAE_RANK_CANDIDATES_MAX (include/cdae_hip.h): candidates per row that score_rows ranks
NO_USER = 0xFFFFFFFF           # CDAE_NO_USER (include/cdae_hip.h): a row of recommend_rows / eval_topn_rows without a user node
ALS_USERS, ALS_ITEMS = 0, 1         # CDAE_ALS_USERS / CDAE_ALS_ITEMS: the side a WRMF half-step solves
WARP_MAX_TRY = 500                  # CDAE_WARP_MAX_TRY (include/cdae_hip.h): draws of one WARP search; cnt == WARP_MAX_TRY: exhausted
WARP_NONE = 0xFFFFFFFF              # the item of an exhausted search
ITEMS_OUTPUT, ITEMS_INPUT = 0, 1   # CDAE_ITEMS_OUTPUT / CDAE_ITEMS_INPUT (include/cdae_hip.h): the item table similar_items compares rows of
SIM_DOT, SIM_COSINE = 0, 1         # CDAE_SIM_DOT / CDAE_SIM_COSINE (include/cdae_hip.h): its score
DEFAULT_BATCH_USERS = 0        # 0 = the library's default (cdae_hip_default_batch_users: num_users / 160, within [32, 256])


def GUEST_USER(i):
    """CDAE_GUEST_USER(i) (include/cdae_hip.h): the uid of node i of a handle's guest table; scalars and arrays alike -> uint32"""
    i = np.asarray(i)
    if i.size and (i.min() < 0 or i.max() > 0x7FFFFFFE):
        raise ValueError("guest index out of range")
    g = (i.astype(np.uint32) | np.uint32(0x80000000)).astype(np.uint32)
    return g if g.ndim else np.uint32(g)


class _Config(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "struct_size", "num_dim", "num_neg", "num_corruptions", "loss_type", "using_adagrad",
        "asymmetric", "user_factor", "linear", "scaled", "tanh_act", "batch_users", "full_output", "linear_function")] + [
            (n, C.c_double) for n in ("lambda_", "learn_rate", "corruption_ratio", "beta")]


class _MfConfig(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "num_dim", "num_neg", "loss_type", "using_adagrad", "using_bias_term",
                                          "pairwise", "batch_users")] + [(n, C.c_double) for n in ("lambda_", "learn_rate", "beta")]


class _AlsConfig(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "num_dim", "cg_steps", "reserved")] + [(n, C.c_double) for n in ("lambda_", "alpha")]


class _WarpConfig(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "num_dim", "num_neg", "loss_type", "using_adagrad", "batch_users")] + [
        (n, C.c_double) for n in ("lambda_", "learn_rate")]


class _FismConfig(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "num_dim", "num_neg", "loss_type", "using_adagrad", "using_bias_term", "batch_users",
                                          "reserved")] + [(n, C.c_double) for n in ("lambda_", "learn_rate", "alpha")]


class Stats(C.Structure):
    _fields_ = [("wall_seconds", C.c_double), ("users", C.c_uint64), ("examples", C.c_uint64),
                ("batches", C.c_uint64), ("ms_sample", C.c_double), ("ms_sort", C.c_double),
                ("ms_encode", C.c_double), ("ms_decode", C.c_double), ("ms_hidden", C.c_double),
                ("ms_input", C.c_double), ("launches_decode", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


EXPORTS = {
    # name: (restype, argtypes) — every symbol include/cdae_hip.h declares
    "cdae_hip_last_error": (C.c_char_p, []),
    "cdae_hip_abi_version": (C.c_int, []),
    "cdae_hip_create": (C.c_int, [C.POINTER(_Config), C.c_int, C.POINTER(C.c_void_p)]),
    "cdae_hip_create_mf": (C.c_int, [C.POINTER(_MfConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "cdae_hip_create_als": (C.c_int, [C.POINTER(_AlsConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "cdae_hip_als_half_step": (C.c_int, [C.c_void_p, C.c_uint32]),
    "cdae_hip_als_solve_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cdae_hip_als_gram": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "cdae_hip_als_set_confidence": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "cdae_hip_als_solve_rows_weighted": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                  C.c_void_p]),
    "cdae_hip_als_objective": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cdae_hip_create_warp": (C.c_int, [C.POINTER(_WarpConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "cdae_hip_warp_search": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "cdae_hip_warp_record_choices": (C.c_int, [C.c_void_p, C.c_uint32]),
    "cdae_hip_warp_choices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "cdae_hip_create_fism": (C.c_int, [C.POINTER(_FismConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "cdae_hip_create_fism_pair": (C.c_int, [C.POINTER(_FismConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "cdae_hip_fism_plan": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "cdae_hip_fism_set_resident": (C.c_int, [C.c_void_p, C.c_int]),
    "cdae_hip_destroy": (C.c_int, [C.c_void_p]),
    "cdae_hip_set_interactions": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cdae_hip_row_stride": (C.c_uint32, [C.c_void_p]),
    "cdae_hip_default_batch_users": (C.c_uint32, [C.c_uint64]),
    "cdae_hip_mf_default_batch_users": (C.c_uint32, [C.c_uint64, C.c_uint32]),
    "cdae_hip_batch_users": (C.c_uint32, [C.c_void_p]),
    "cdae_hip_full_output_plan": (C.c_uint32, [C.c_void_p]),
    "cdae_hip_set_decode_fused": (C.c_int, [C.c_void_p, C.c_int]),
    "cdae_hip_decode_plan": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "cdae_hip_user_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "cdae_hip_set_user_id_offset": (C.c_int, [C.c_void_p, C.c_uint64]),
    "cdae_hip_init_params": (C.c_int, [C.c_void_p, C.c_uint64]),
    "cdae_hip_set_param": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "cdae_hip_get_param": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "cdae_hip_param_device_ptr": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "cdae_hip_train_epoch": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(Stats)]),
    "cdae_hip_train_users": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(Stats)]),
    "cdae_hip_enqueue_users": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64]),
    "cdae_hip_prefetch_users": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64]),
    "cdae_hip_collect_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "cdae_hip_train_one_user_corruption": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "cdae_hip_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "cdae_hip_set_profiling_families": (C.c_int, [C.c_void_p, C.c_uint32]),
    "cdae_hip_synchronize": (C.c_int, [C.c_void_p]),
    "cdae_hip_debug_row_pack": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cdae_hip_debug_sample_batch": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8
                                    + [C.POINTER(C.c_uint64)]),
    "cdae_hip_encode": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cdae_hip_data_loss": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
    "cdae_hip_penalty_loss": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cdae_hip_recommend_all": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]),
    "cdae_hip_recommend_user": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
    "cdae_hip_recommend_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "cdae_hip_recommend_rows_filtered": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                   C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "cdae_hip_similar_items": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "cdae_hip_score_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cdae_hip_full_rank_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cdae_hip_eval_topn_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "cdae_hip_fold_in_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cdae_hip_set_guest_nodes": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cdae_hip_guest_nodes": (C.c_uint64, [C.c_void_p]),
    "cdae_hip_set_test_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cdae_hip_eval_topn": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cdae_hip_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "cdae_hip_delta_begin": (C.c_int, [C.c_void_p]),
    "cdae_hip_delta_compute": (C.c_int, [C.c_void_p]),
    "cdae_hip_delta_device_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "cdae_hip_delta_apply": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "cdae_hip_delta_stage": (C.c_int, [C.c_void_p]),
    "cdae_hip_delta_set_combine": (C.c_int, [C.c_void_p, C.c_uint32]),
    "cdae_hip_delta_recv_device_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "cdae_hip_delta_merge": (C.c_int, [C.c_void_p]),
    "cdae_hip_delta_merge_stage": (C.c_int, [C.c_void_p]),
    "cdae_hip_comm_unique_id": (C.c_int, [C.c_void_p, C.c_size_t]),
    "cdae_hip_comm_init_rank": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "cdae_hip_exchange_configure": (C.c_int, [C.c_void_p, C.c_int]),
    "cdae_hip_exchange_step": (C.c_int, [C.c_void_p]),
    "cdae_hip_exchange_flush": (C.c_int, [C.c_void_p]),
    "cdae_hip_exchange_time_all_reduce": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "cdae_hip_multi_create": (C.c_int, [C.POINTER(_Config), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "cdae_hip_multi_destroy": (C.c_int, [C.c_void_p]),
    "cdae_hip_multi_set_layout": (C.c_int, [C.c_void_p, C.c_uint32]),
    "cdae_hip_multi_num_shards": (C.c_int, [C.c_void_p]),
    "cdae_hip_multi_shard": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cdae_hip_multi_set_interactions": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cdae_hip_multi_init_params": (C.c_int, [C.c_void_p, C.c_uint64]),
    "cdae_hip_multi_set_exchange": (C.c_int, [C.c_void_p, C.c_int]),
    "cdae_hip_multi_set_schedule": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cdae_hip_multi_train_epoch": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(Stats)]),
    "cdae_hip_multi_steps_per_epoch": (C.c_uint64, [C.c_void_p]),
    "cdae_hip_multi_train_steps": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(Stats)]),
    "cdae_hip_multi_train_users": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(Stats)]),
    "cdae_hip_multi_data_loss": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
    "cdae_hip_multi_penalty_loss": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "cdae_hip_multi_recommend_all": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]),
    "cdae_hip_multi_eval_topn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cdae_hip_multi_get_param": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "cdae_hip_multi_set_param": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
}
COMM_ID_BYTES = 128

_libs = {}                 # path -> loaded library
_default_path = LIB_PATH   # what load_library() without a path returns (developer_library swaps it for the length of a test)


def load_library(path: str | None = None):
    """dlopen the C-ABI library and bind every declared export.  Raises if it is missing."""
    path = path or _default_path
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the CDAE hot path.")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64 (ROCm 7.0) next
    # to the system's (7.2).  If this library pulled the system copies in first, a later `import torch` (needed
    # only for torch.distributed) finds a foreign runtime already loaded and reports "No HIP GPUs are available".
    # Loading torch first makes both share torch's copy, which the kernels run on unchanged.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)       # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _libs[path] = lib
    return lib



@contextlib.contextmanager
def developer_library():
    """Inside the block every new CDAE / MultiCDAE / MF object is created on the DEVELOPER build (environment switches compiled in).
    Handles of the two libraries are not interchangeable; a comparison of a switched path with the default one runs both sides here."""
    global _default_path
    load_library(DEV_LIB_PATH)
    prev, _default_path = _default_path, DEV_LIB_PATH
    try:
        yield _libs[DEV_LIB_PATH]
    finally:
        _default_path = prev


class CDAEError(RuntimeError):
    pass


def _chk(lib, rc):
    if rc != 0:
        raise CDAEError(lib.cdae_hip_last_error().decode())


@dataclass
class CDAEConfig:
    """libcf::CDAEConfig (/root/reference/src/model/recsys/cdae.hpp:13-31); defaults are the struct's."""
    lambda_: float = 0.01
    learn_rate: float = 0.1
    lt: int = LOGISTIC
    num_dim: int = 10
    using_adagrad: bool = True
    corruption_ratio: float = 0.5
    num_corruptions: int = 1
    asymmetric: bool = False
    user_factor: bool = True
    linear: bool = False
    num_neg: int = 5
    scaled: bool = True
    beta: float = 0.0
    linear_function: bool = False
    tanh: bool = False
    # not in the reference: users per parameter snapshot (1 == the reference's sequential schedule)
    batch_users: int = DEFAULT_BATCH_USERS
    # not in the reference: full-output decode — every unrated item is a negative once (MFMA path)
    full_output: bool = False


class CDAE:
    """Host mirror of libcf::CDAE over the C ABI.

    reset(train) ~ cdae.hpp:109-134, train_one_iteration ~ :136-146, current_loss ~ model_base.hpp:29-32,
    pre_recommend/recommend ~ :162-196 (all users at once on the GPU, then table lookups).
    """

    def __init__(self, mcfg: CDAEConfig, device: int = 0):
        self.lib = load_library()
        self.cfg = mcfg
        c = _Config(C.sizeof(_Config), mcfg.num_dim, mcfg.num_neg, mcfg.num_corruptions, mcfg.lt,
                    int(mcfg.using_adagrad), int(mcfg.asymmetric), int(mcfg.user_factor), int(mcfg.linear),
                    int(mcfg.scaled), int(mcfg.tanh), mcfg.batch_users, int(mcfg.full_output), int(mcfg.linear_function),
                    mcfg.lambda_, mcfg.learn_rate,
                    mcfg.corruption_ratio, mcfg.beta)
        self.h = C.c_void_p()
        _chk(self.lib, self.lib.cdae_hip_create(C.byref(c), device, C.byref(self.h)))
        self.num_users = self.num_items = 0
        self._rec = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.cdae_hip_destroy(self.h)
            self.h = None

    __del__ = close

    # ---- reset -------------------------------------------------------------------------------------
    def set_interactions(self, num_users, num_items, row_ptr, col_idx, user_id_offset: int = 0):
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ci = np.ascontiguousarray(col_idx, dtype=np.uint32)
        if rp.size != num_users + 1 or ci.size != rp[-1]:
            raise CDAEError("row_ptr / col_idx sizes do not match num_users")
        _chk(self.lib, self.lib.cdae_hip_set_interactions(self.h, num_users, num_items, rp.ctypes.data, ci.ctypes.data))
        _chk(self.lib, self.lib.cdae_hip_set_user_id_offset(self.h, user_id_offset))
        self.num_users, self.num_items = int(num_users), int(num_items)
        self._row_ptr = rp

    def reset(self, train, seed: int = 0):
        """train: object with num_users, num_items, train_ptr, train_col (cdae_amd.synth.Interactions)."""
        self.set_interactions(train.num_users, train.num_items, train.train_ptr, train.train_col)
        self.init_params(seed)

    def init_params(self, seed: int):
        _chk(self.lib, self.lib.cdae_hip_init_params(self.h, seed))

    def user_order(self) -> np.ndarray:
        """out[position] = user id of the handle's training order (the identity except for IMF / BPR block schedules)"""
        out = np.empty(self.num_users, dtype=np.uint32)
        _chk(self.lib, self.lib.cdae_hip_user_order(self.h, out.ctypes.data, out.size))
        return out

    @property
    def batch_users(self) -> int:
        """users per parameter snapshot the handle is using (the library's choice when the config asked for 0)"""
        return int(self.lib.cdae_hip_batch_users(self.h))

    def set_decode_fused(self, allow: bool):
        """cdae_hip_set_decode_fused: off for handles trained side by side with another handle on the same device"""
        _chk(self.lib, self.lib.cdae_hip_set_decode_fused(self.h, int(bool(allow))))

    @property
    def decode_plan(self) -> dict:
        """{hot_rows, late_rows, fused} of the sampled step (include/cdae_hip.h cdae_hip_decode_plan)"""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _chk(self.lib, self.lib.cdae_hip_decode_plan(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(hot_rows=int(a.value), late_rows=int(b.value), fused=bool(c.value))

    @property
    def full_output_plan(self) -> int:
        """CDAE_PLAN_* bits (include/cdae_hip.h): which launches this handle's full-output decode is made of"""
        return int(self.lib.cdae_hip_full_output_plan(self.h))

    # ---- parameters --------------------------------------------------------------------------------
    def _shape(self, which):
        K = self.cfg.num_dim
        if which in (P_BP, P_BP_AG):
            return (self.num_items,)
        if which in (P_B, P_B_AG):
            return (K,)
        if which in (P_WU, P_WU_AG, P_UU, P_UU_AG):
            return (self.num_users, K)
        return (self.num_items, K)

    def get(self, which) -> np.ndarray:
        out = np.empty(self._shape(which), dtype=np.float32)
        _chk(self.lib, self.lib.cdae_hip_get_param(self.h, which, out.ctypes.data, out.size))
        return out

    def set(self, which, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(self._shape(which))
        _chk(self.lib, self.lib.cdae_hip_set_param(self.h, which, a.ctypes.data, a.size))

    def param_device_ptr(self, which):
        p, n = C.c_void_p(), C.c_size_t()
        _chk(self.lib, self.lib.cdae_hip_param_device_ptr(self.h, which, C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- training ----------------------------------------------------------------------------------
    def set_profiling(self, period, families=None):
        """0/False: off; k >= 1 (True = 1): HIP-event kernel timing on every k-th batch, of the families named (e.g. ("decode",))
        or of all of them."""
        names = ("sample", "sort", "encode", "decode", "hidden", "input")
        mask = 0xFFFFFFFF if families is None else sum(1 << names.index(f) for f in families)
        _chk(self.lib, self.lib.cdae_hip_set_profiling_families(self.h, mask))
        _chk(self.lib, self.lib.cdae_hip_set_profiling(self.h, int(period)))

    def train_one_iteration(self, seed: int, epoch: int) -> Stats:
        st = Stats()
        _chk(self.lib, self.lib.cdae_hip_train_epoch(self.h, seed, epoch, C.byref(st)))
        return st

    def train_users(self, seed: int, epoch: int, u_begin: int, u_end: int) -> Stats:
        st = Stats()
        _chk(self.lib, self.lib.cdae_hip_train_users(self.h, seed, epoch, u_begin, u_end, C.byref(st)))
        return st

    def enqueue_users(self, seed: int, epoch: int, u_begin: int, u_end: int):
        _chk(self.lib, self.lib.cdae_hip_enqueue_users(self.h, seed, epoch, u_begin, u_end))

    def prefetch_users(self, seed: int, epoch: int, u_begin: int, u_end: int):
        _chk(self.lib, self.lib.cdae_hip_prefetch_users(self.h, seed, epoch, u_begin, u_end))

    def collect_stats(self) -> Stats:
        st = Stats()
        _chk(self.lib, self.lib.cdae_hip_collect_stats(self.h, C.byref(st)))
        return st

    def synchronize(self):
        _chk(self.lib, self.lib.cdae_hip_synchronize(self.h))

    def _batch_examples(self, u_begin: int, n_users: int) -> int:
        """examples in the item-sorted list of the batch of users [u_begin, u_begin + n_users)"""
        nnz = int(self._row_ptr[u_begin + n_users] - self._row_ptr[u_begin])
        return nnz * (1 if self.cfg.full_output else 1 + self.cfg.num_neg)

    def debug_sample_batch(self, seed: int, epoch: int, u_begin: int, n_users: int, cidx: int = 0) -> dict:
        """Integer work of one batch (masks, negatives, item sort, segments, duplicate numbering) copied back from the
        device (cdae_hip_debug_sample_batch) — the bit-exact parity tests compare it with the oracle's draws."""
        E = self._batch_examples(u_begin, n_users)
        out = {"ex_item": np.empty(E, np.uint32), "ex_val": np.empty(E, np.uint64), "sorted_item": np.empty(E, np.uint32),
               "sorted_val": np.empty(E, np.uint64), "seg_begin": np.empty(self.num_items, np.uint32),
               "seg_end": np.empty(self.num_items, np.uint32), "dup_of_pos": np.empty(E, np.uint32),
               "dup_of_ex": np.empty(E, np.uint32)}
        n = C.c_uint64(E)
        _chk(self.lib, self.lib.cdae_hip_debug_sample_batch(
            self.h, seed, epoch, u_begin, n_users, cidx, *[a.ctypes.data for a in out.values()], C.byref(n)))
        assert n.value == E
        return out

    def debug_row_pack(self, seed: int, epoch: int, u_begin: int, n_users: int, cidx: int = 0) -> np.ndarray:
        """The row pack of one batch prepared as training would (cdae_hip_debug_row_pack): uint32 [records, 4] of
        (item, sorted begin, sorted end, popularity rank); no rows for a handle or batch without a pack."""
        rec = np.empty(((self.num_items + 3) // 4 * 4, 4), np.uint32)
        n = C.c_uint64(rec.shape[0])
        _chk(self.lib, self.lib.cdae_hip_debug_row_pack(self.h, seed, epoch, u_begin, n_users, cidx, rec.ctypes.data, C.byref(n)))
        return rec[:n.value].copy()

    def train_one_user_corruption(self, uid: int, input_items, negative_items):
        """cdae.hpp:198-200 with explicit input set; negatives as the reference would have drawn them."""
        i = np.ascontiguousarray(input_items, dtype=np.uint32)
        n = np.ascontiguousarray(negative_items, dtype=np.uint32)
        _chk(self.lib, self.lib.cdae_hip_train_one_user_corruption(self.h, uid, i.ctypes.data, i.size, n.ctypes.data, n.size))

    def get_hidden_values(self, uids, seed: int = 0, epoch: int = 0, mode: int = 0) -> np.ndarray:
        u = np.ascontiguousarray(uids, dtype=np.uint32)
        Z = np.empty((u.size, self.cfg.num_dim), dtype=np.float32)
        _chk(self.lib, self.lib.cdae_hip_encode(self.h, seed, epoch, mode, u.ctypes.data, u.size, Z.ctypes.data))
        return Z

    def data_loss(self, seed: int, epoch: int) -> float:
        v = C.c_double()
        _chk(self.lib, self.lib.cdae_hip_data_loss(self.h, seed, epoch, C.byref(v)))
        return v.value

    def penalty_loss(self) -> float:
        v = C.c_double()
        _chk(self.lib, self.lib.cdae_hip_penalty_loss(self.h, C.byref(v)))
        return v.value

    def current_loss(self, seed: int, epoch: int) -> float:
        return self.data_loss(seed, epoch) + self.penalty_loss()      # model_base.hpp:29-32

    # ---- evaluation --------------------------------------------------------------------------------
    def recommend_all(self, topk: int = 10, u_begin: int = 0, u_end: int | None = None) -> np.ndarray:
        u_end = self.num_users if u_end is None else u_end
        out = np.empty((u_end - u_begin, topk), dtype=np.uint32)
        _chk(self.lib, self.lib.cdae_hip_recommend_all(self.h, u_begin, u_end, topk, out.ctypes.data))
        return out

    def recommend_user(self, uid: int, rated_items, topk: int = 10) -> np.ndarray:
        """recommend(uid, topk, rated_item_set) for a set that is not the train row (cdae.hpp:162-196)."""
        r = np.ascontiguousarray(rated_items, dtype=np.uint32)
        out = np.empty(topk, dtype=np.uint32)
        _chk(self.lib, self.lib.cdae_hip_recommend_user(self.h, uid, r.ctypes.data, r.size, topk, out.ctypes.data))
        return out

    @staticmethod
    def _rows(row_ptr, col, uids):
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        rc = np.ascontiguousarray(col, dtype=np.uint32)
        if rp.ndim != 1 or rp.size < 1 or (rp.size > 1 and rc.size < rp[-1]):
            raise ValueError("row_ptr / col are not a CSR")
        ru = None if uids is None else np.ascontiguousarray(uids, dtype=np.uint32)
        if ru is not None and ru.size != rp.size - 1:
            raise ValueError("one uid per row")
        return rp, rc, ru

    def recommend_rows(self, row_ptr, col, uids=None, topk: int = 10, with_scores: bool = False):
        """recommend(uid, topk, rated_item_set) for many caller-supplied rated sets at once (cdae_hip_recommend_rows): CSR rows
        with ascending unique items, uids[r] the user whose private rows row r takes (NO_USER: none; None: none anywhere).
        -> ids [n_rows, topk] uint32 (0xFFFFFFFF beyond a row's unrated items), or (ids, scores) with the fp32 scores."""
        rp, rc, ru = self._rows(row_ptr, col, uids)
        n = rp.size - 1
        ids = np.empty((n, topk), dtype=np.uint32)
        scores = np.empty((n, topk), dtype=np.float32) if with_scores else None
        _chk(self.lib, self.lib.cdae_hip_recommend_rows(self.h, n, None if ru is None else ru.ctypes.data, rp.ctypes.data, rc.ctypes.data,
                                                        topk, ids.ctypes.data, scores.ctypes.data if with_scores else None))
        return (ids, scores) if with_scores else ids

    def recommend_rows_filtered(self, row_ptr, col, uids=None, topk: int = 10, exclude=None, allow=None, exclude_rated: bool = True,
                                with_scores: bool = False):
        """recommend_rows with the excluded set cut loose from the input set (cdae_hip_recommend_rows_filtered).  exclude: a
        (ptr, col) CSR over the same rows of items that must not be listed but do not enter z (None: none); allow: ONE ascending
        unique item list for the whole call, the only items that may be listed (None: the whole catalogue); exclude_rated=False:
        a row's own items are candidates too.  Row r's list is recommend_rows' unbounded list with the items outside
        allow minus exclude[r] (minus rated[r]) deleted, the same fp32 scores -> ids [n_rows, topk] uint32 of original item ids
        (0xFFFFFFFF beyond a row's candidates), or (ids, scores)."""
        rp, rc, ru = self._rows(row_ptr, col, uids)
        n = rp.size - 1
        ep = ec = None
        if exclude is not None:
            ep, ec, _ = self._rows(exclude[0], exclude[1], None)
            if ep.size != rp.size:
                raise ValueError("the exclude CSR covers the same rows")
        al = None if allow is None else np.ascontiguousarray(allow, dtype=np.uint32).reshape(-1)
        al_buf = al if al is None or al.size else np.zeros(1, dtype=np.uint32)      # an empty list is still a list: the library refuses it
        ids = np.empty((n, topk), dtype=np.uint32)
        scores = np.empty((n, topk), dtype=np.float32) if with_scores else None
        _chk(self.lib, self.lib.cdae_hip_recommend_rows_filtered(
            self.h, n, None if ru is None else ru.ctypes.data, rp.ctypes.data, rc.ctypes.data,
            None if ep is None else ep.ctypes.data, None if ep is None else ec.ctypes.data, 1 if exclude_rated else 0,
            None if al is None else al_buf.ctypes.data, 0 if al is None else al.size, topk, ids.ctypes.data,
            scores.ctypes.data if with_scores else None))
        return (ids, scores) if with_scores else ids

    def similar_items(self, items, topk: int = 10, metric: str = "cosine", table: str = "output", exclude_self: bool = True, exclude=None,
                      allow=None, with_scores: bool = False):
        """The topk items closest to each of `items` (cdae_hip_similar_items).  metric: "cosine" or "dot"; table: "output" (the rows
        the scores are made of: V when asymmetric, else W) or "input" (W, the rows the encoder sums; an IMF / BPR model has one item
        table and both name it); exclude_self=False: a query may list itself; exclude: a (ptr, col) CSR over the queries of items
        that must not be listed (None: none); allow: ONE ascending unique item list for the whole call, the only items that may be
        listed (None: the whole catalogue; the queries need not be in it) -> ids [n_queries, topk] uint32 (0xFFFFFFFF beyond a
        query's candidates), or (ids, scores) with the fp32 scores."""
        metrics = {"dot": SIM_DOT, "cosine": SIM_COSINE}
        tables = {"output": ITEMS_OUTPUT, "input": ITEMS_INPUT}
        if metric not in metrics or table not in tables:
            raise ValueError('metric is "dot" or "cosine", table is "output" or "input"')
        q = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1)
        n = q.size
        ep = ec = None
        if exclude is not None:
            ep, ec, _ = self._rows(exclude[0], exclude[1], None)
            if ep.size != n + 1:
                raise ValueError("the exclude CSR covers the queries")
        al = None if allow is None else np.ascontiguousarray(allow, dtype=np.uint32).reshape(-1)
        al_buf = al if al is None or al.size else np.zeros(1, dtype=np.uint32)      # an empty list is still a list: the library refuses it
        ids = np.empty((n, topk), dtype=np.uint32)
        scores = np.empty((n, topk), dtype=np.float32) if with_scores else None
        _chk(self.lib, self.lib.cdae_hip_similar_items(
            self.h, n, q.ctypes.data, tables[table], metrics[metric], 1 if exclude_self else 0,
            None if ep is None else ep.ctypes.data, None if ep is None else ec.ctypes.data,
            None if al is None else al_buf.ctypes.data, 0 if al is None else al.size, topk, ids.ctypes.data,
            scores.ctypes.data if with_scores else None))
        return (ids, scores) if with_scores else ids

    def eval_topn_rows(self, row_ptr, col, target_ptr, target_col, uids=None, topk: int = 10, with_ids: bool = False):
        """The lists of recommend_rows scored on the device against per-row target sets by the rules of eval_topn
        (cdae_hip_eval_topn_rows): (rets[8], hits[3]) or (rets, hits, ids)."""
        rp, rc, ru = self._rows(row_ptr, col, uids)
        tp, tc, _ = self._rows(target_ptr, target_col, None)
        if tp.size != rp.size:
            raise ValueError("the target CSR covers the same rows")
        n = rp.size - 1
        rets, hits = np.empty(8, dtype=np.float64), np.empty(3, dtype=np.uint64)
        ids = np.empty((n, topk), dtype=np.uint32) if with_ids else None
        _chk(self.lib, self.lib.cdae_hip_eval_topn_rows(self.h, n, None if ru is None else ru.ctypes.data, rp.ctypes.data, rc.ctypes.data,
                                                        tp.ctypes.data, tc.ctypes.data, topk, rets.ctypes.data, hits.ctypes.data,
                                                        ids.ctypes.data if with_ids else None))
        return (rets, hits, ids) if with_ids else (rets, hits)

    def score_rows(self, row_ptr, col, cand_ptr, cand_col, uids=None, with_ranks: bool = False):
        """get_output_values for many rows at once (cdae_hip_score_rows): the fp32 scores of the candidates a second CSR over the
        same rows names (ascending unique items; a row's own rated items allowed), in CSR order -> scores float32 [nnz_cand], or
        (scores, ranks uint32 [nnz_cand]): a candidate's place among its row's candidates in recommend_all's order, 0 the best
        (rows of at most RANK_CANDIDATES_MAX candidates)."""
        rp, rc, ru = self._rows(row_ptr, col, uids)
        cp, cc, _ = self._rows(cand_ptr, cand_col, None)
        if cp.size != rp.size:
            raise ValueError("the candidate CSR covers the same rows")
        n = rp.size - 1
        total = max(int(cp[-1]), 0) if n else 0
        scores = np.empty(total, dtype=np.float32)
        ranks = np.empty(total, dtype=np.uint32) if with_ranks else None
        _chk(self.lib, self.lib.cdae_hip_score_rows(self.h, n, None if ru is None else ru.ctypes.data, rp.ctypes.data, rc.ctypes.data,
                                                    cp.ctypes.data, cc.ctypes.data, scores.ctypes.data, ranks.ctypes.data if with_ranks else None))
        return (scores, ranks) if with_ranks else scores

    def full_rank_rows(self, row_ptr, col, target_ptr, target_col, uids=None, with_scores: bool = False):
        """The exact place of named items in each row's WHOLE list (cdae_hip_full_rank_rows): for every target of a second CSR over
        the same rows (ascending unique items, none of them rated by its row; no cap per row), the number of items outside the row's
        rated set that precede it in recommend_all's order, 0 the head of the list -> ranks uint32 [nnz_targets] in CSR order, or
        (ranks, scores) with the fp32 scores the counting used."""
        rp, rc, ru = self._rows(row_ptr, col, uids)
        tp, tc, _ = self._rows(target_ptr, target_col, None)
        if tp.size != rp.size:
            raise ValueError("the target CSR covers the same rows")
        n = rp.size - 1
        total = max(int(tp[-1]), 0) if n else 0
        ranks = np.empty(total, dtype=np.uint32)
        scores = np.empty(total, dtype=np.float32) if with_scores else None
        _chk(self.lib, self.lib.cdae_hip_full_rank_rows(self.h, n, None if ru is None else ru.ctypes.data, rp.ctypes.data, rc.ctypes.data,
                                                        tp.ctypes.data, tc.ctypes.data, ranks.ctypes.data, scores.ctypes.data if with_scores else None))
        return (ranks, scores) if with_scores else ranks

    def eval_ranking_rows(self, row_ptr, col, target_ptr, target_col, uids=None, ks=(1, 5, 10, 20, 50, 100)):
        """Full-catalogue ranking metrics of per-row target sets: full_rank_rows, then metrics.ranking_metrics over the ranks
        (recall@k, precision@k, ndcg@k, map@k for every k of ks, mrr, auc: means over the rows with targets)."""
        from .metrics import ranking_metrics
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ranks = self.full_rank_rows(rp, col, target_ptr, target_col, uids)
        return ranking_metrics(target_ptr, ranks, self.num_items - np.diff(rp), ks)

    def fold_in_rows(self, row_ptr, col, uids=None, *, seed: int = 0, epoch_begin: int = 0, n_epochs: int = 10, stream_id_base: int = 0,
                     install: bool = False, with_accumulators: bool = False):
        """Fit the user node of many rows that are no train rows, everything shared frozen (cdae_hip_fold_in_rows): CSR rows with
        ascending unique items; uids[r] the node row r starts from (a user: a copy of its rows; NO_USER / None: zeros and ones;
        GUEST_USER(i): guest i).  Row r draws the masks and negatives of user id stream_id_base + r in epochs [epoch_begin,
        epoch_begin + n_epochs).  install: the fitted nodes become the handle's guest table, row r as GUEST_USER(r).
        -> wu [n_rows, num_dim] float32, or (wu, uu) under linear_function; with_accumulators: (wu, wu_ag), or (wu, wu_ag, uu, uu_ag)."""
        rp, rc, ru = self._rows(row_ptr, col, uids)
        n, K = rp.size - 1, self.cfg.num_dim
        lf = bool(getattr(self.cfg, "linear_function", False))
        wu = np.empty((n, K), dtype=np.float32)
        wa = np.empty((n, K), dtype=np.float32) if with_accumulators else None
        uu = np.empty((n, K), dtype=np.float32) if lf else None
        ua = np.empty((n, K), dtype=np.float32) if lf and with_accumulators else None
        _chk(self.lib, self.lib.cdae_hip_fold_in_rows(self.h, n, None if ru is None else ru.ctypes.data, rp.ctypes.data, rc.ctypes.data, seed,
                                                      epoch_begin, n_epochs, stream_id_base, int(bool(install)),
                                                      *[None if a is None else a.ctypes.data for a in (wu, wa, uu, ua)]))
        out = tuple(a for a in (wu, wa, uu, ua) if a is not None)
        return out[0] if len(out) == 1 else out

    def set_guest_nodes(self, wu, wu_ag=None, uu=None, uu_ag=None):
        """Replace the handle's guest table by host rows (cdae_hip_set_guest_nodes): wu [n, num_dim]; an array left None stands for
        its "no node" value (accumulators 1e-4, uu ones).  n == 0 clears the table."""
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (wu, wu_ag, uu, uu_ag)]
        given = [a for a in arrs if a is not None]
        if not given:
            raise ValueError("set_guest_nodes needs at least one array (its rows are the table's size)")
        n = given[0].shape[0] if given[0].ndim == 2 else 0
        if any(a.shape != (n, self.cfg.num_dim) for a in given):
            raise ValueError("guest node arrays are [n_guests, num_dim]")
        _chk(self.lib, self.lib.cdae_hip_set_guest_nodes(self.h, n, *[None if a is None else a.ctypes.data for a in arrs]))

    @property
    def num_guest_nodes(self) -> int:
        """rows of the handle's guest table (cdae_hip_guest_nodes)"""
        return int(self.lib.cdae_hip_guest_nodes(self.h))

    def set_test_rows(self, test_ptr, test_col):
        """the validation rows TOPN_Evaluation scores against (evaluation.hpp:118-120), CSR over this handle's users"""
        tp = np.ascontiguousarray(test_ptr, dtype=np.int64)
        tc = np.ascontiguousarray(test_col, dtype=np.uint32)
        _chk(self.lib, self.lib.cdae_hip_set_test_rows(self.h, tp.ctypes.data, tc.ctypes.data))

    def eval_topn(self, topk: int = 10, with_ids: bool = False):
        """TOPN_Evaluation::evaluate on the device (evaluation.hpp:113-219): (rets[8], hits[3]) or (rets, hits, ids)."""
        rets, hits = np.empty(8, dtype=np.float64), np.empty(3, dtype=np.uint64)
        ids = np.empty((self.num_users, topk), dtype=np.uint32) if with_ids else None
        _chk(self.lib, self.lib.cdae_hip_eval_topn(self.h, topk, rets.ctypes.data, hits.ctypes.data, ids.ctypes.data if with_ids else None))
        return (rets, hits, ids) if with_ids else (rets, hits)

    def pre_recommend(self, topk: int = 10):
        self._rec = self.recommend_all(topk)

    def recommend(self, uid: int, topk: int = 10):
        if self._rec is None or self._rec.shape[1] != topk:
            self.pre_recommend(topk)
        return self._rec[uid]

    # ---- data-parallel exchange --------------------------------------------------------------------
    def stream_handle(self) -> int:
        p = C.c_void_p()
        _chk(self.lib, self.lib.cdae_hip_stream(self.h, C.byref(p)))
        return p.value

    def delta_begin(self):
        _chk(self.lib, self.lib.cdae_hip_delta_begin(self.h))

    def delta_compute(self):
        _chk(self.lib, self.lib.cdae_hip_delta_compute(self.h))

    def delta_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        _chk(self.lib, self.lib.cdae_hip_delta_device_ptr(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def delta_apply(self, world_size: int, rule: int = 0):
        _chk(self.lib, self.lib.cdae_hip_delta_apply(self.h, world_size, rule))

    def delta_set_combine(self, combine: int):
        _chk(self.lib, self.lib.cdae_hip_delta_set_combine(self.h, combine))

    def delta_stage(self):
        _chk(self.lib, self.lib.cdae_hip_delta_stage(self.h))

    def delta_recv_device_ptr(self):
        p, n = C.c_void_p(), C.c_size_t()
        _chk(self.lib, self.lib.cdae_hip_delta_recv_device_ptr(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def delta_merge(self):
        _chk(self.lib, self.lib.cdae_hip_delta_merge(self.h))

    def delta_merge_stage(self):
        _chk(self.lib, self.lib.cdae_hip_delta_merge_stage(self.h))

    # ---- library-owned communicator + exchange schedule (one process per GPU) ---------------------------------------
    def comm_init_rank(self, world_size: int, rank: int, unique_id: bytes):
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        _chk(self.lib, self.lib.cdae_hip_comm_init_rank(self.h, world_size, rank, buf, COMM_ID_BYTES))

    def exchange_configure(self, period: int):
        _chk(self.lib, self.lib.cdae_hip_exchange_configure(self.h, period))

    def exchange_step(self):
        _chk(self.lib, self.lib.cdae_hip_exchange_step(self.h))

    def exchange_flush(self):
        _chk(self.lib, self.lib.cdae_hip_exchange_flush(self.h))

    def exchange_time_all_reduce(self, repeats: int = 5) -> float:
        v = C.c_double()
        _chk(self.lib, self.lib.cdae_hip_exchange_time_all_reduce(self.h, repeats, C.byref(v)))
        return v.value


@dataclass
class MFConfig:
    """libcf::IMFConfig / BPRConfig (/root/reference/src/model/recsys/imf.hpp:12-23, bpr.hpp:12-24); pairwise=True is BPR."""
    learn_rate: float = 0.1
    beta: float = 1.0
    lambda_: float = 0.01
    lt: int = SQUARE
    num_dim: int = 10
    num_neg: int = 5
    using_bias_term: bool = True
    using_adagrad: bool = True
    pairwise: bool = False
    batch_users: int = DEFAULT_BATCH_USERS


class MF(CDAE):
    """Host mirror of libcf::IMF / libcf::BPR over the same C ABI handle (cdae_hip_create_mf).  get / set use P_WU = uv_,
    P_W = iv_, P_UB = ub_, P_BP = ib_ (and their *_AG accumulators)."""

    def __init__(self, mcfg: MFConfig, device: int = 0):
        self.lib = load_library()
        self.cfg = mcfg
        c = _MfConfig(C.sizeof(_MfConfig), mcfg.num_dim, mcfg.num_neg, mcfg.lt, int(mcfg.using_adagrad), int(mcfg.using_bias_term),
                      int(mcfg.pairwise), mcfg.batch_users, mcfg.lambda_, mcfg.learn_rate, mcfg.beta)
        self.h = C.c_void_p()
        _chk(self.lib, self.lib.cdae_hip_create_mf(C.byref(c), device, C.byref(self.h)))
        self.num_users = self.num_items = 0
        self._rec = None

    def _shape(self, which):
        if which in (P_UB, P_UB_AG):
            return (self.num_users,)
        return CDAE._shape(self, which)

    def _batch_examples(self, u_begin: int, n_users: int) -> int:
        """debug_sample_batch of an IMF / BPR handle: the window is in TRAINING POSITIONS (user_order), an IMF positive gives
        1 + num_neg examples (one per instance), a BPR positive 2 * num_neg (two per pair) — cdae_mf_kernels.hpp mf_sample_kernel"""
        lens = np.diff(self._row_ptr)[self.user_order().astype(np.int64)]
        nnz = int(lens[u_begin:u_begin + n_users].sum())
        return nnz * (2 * self.cfg.num_neg if self.cfg.pairwise else 1 + self.cfg.num_neg)


@dataclass
class WRMFConfig:
    """libcf::WRMFConfig (the reference's src/model/recsys/wrmf.hpp:9-16): lambda, scalar (the confidence weight alpha), num_dim; cg_steps is
    not in the reference (conjugate-gradient iterations per row and half-step; 0 = the library's 3)."""
    lambda_: float = 0.01
    scalar: float = 40.0
    num_dim: int = 10
    cg_steps: int = 3


class WRMF(MF):
    """Weighted-regularised matrix factorisation fitted by alternating least squares (cdae_hip_create_als; include/cdae_hip.h has
    the definition).  The factors are P_WU (users) and P_W (items); recommend_all, eval_topn and similar_items are MF's."""

    def __init__(self, mcfg: WRMFConfig, device: int = 0):
        self.lib = load_library()
        self.cfg = mcfg
        c = _AlsConfig(C.sizeof(_AlsConfig), mcfg.num_dim, mcfg.cg_steps, 0, mcfg.lambda_, mcfg.scalar)
        self.h = C.c_void_p()
        _chk(self.lib, self.lib.cdae_hip_create_als(C.byref(c), device, C.byref(self.h)))
        self.num_users = self.num_items = 0
        self._rec = None

    def half_step(self, side: int):
        """One half-step: ALS_USERS solves every user's row against the frozen item table, ALS_ITEMS the reverse."""
        _chk(self.lib, self.lib.cdae_hip_als_half_step(self.h, side))

    def train_one_iteration(self, seed: int = 0, epoch: int = 0) -> Stats:
        """The user half-step, then the item half-step (seed and epoch are ignored: nothing is drawn)."""
        return MF.train_one_iteration(self, seed, epoch)

    def gram(self, side: int) -> np.ndarray:
        """T^T T of the user (ALS_USERS) or item (ALS_ITEMS) table as the half-steps compute it, [num_dim, num_dim]"""
        K = self.cfg.num_dim
        out = np.empty((K, K), dtype=np.float32)
        _chk(self.lib, self.lib.cdae_hip_als_gram(self.h, side, out.ctypes.data, out.size))
        return out

    def solve_rows(self, row_ptr, col, x0=None, cg_steps: int = 0) -> np.ndarray:
        """Factors of caller-supplied rows (users outside the training set) against the frozen item table: CSR rows with ascending
        unique items, x0 None (zeros) or [n_rows, num_dim] start vectors -> [n_rows, num_dim].  The handle is not written."""
        return self._solve_rows(row_ptr, col, x0, cg_steps, None, False)

    def solve_rows_weighted(self, row_ptr, col, weights=None, x0=None, cg_steps: int = 0) -> np.ndarray:
        """solve_rows with one confidence weight per entry of col — the caller's, not the handle's; None: the bits of solve_rows
        (cdae_hip_als_solve_rows_weighted with w = NULL)."""
        return self._solve_rows(row_ptr, col, x0, cg_steps, weights, True)

    def _solve_rows(self, row_ptr, col, x0, cg_steps, weights, weighted_entry):
        rp, rc, _ = self._rows(row_ptr, col, None)
        n, K = rp.size - 1, self.cfg.num_dim
        a = None
        if x0 is not None:
            a = np.ascontiguousarray(x0, dtype=np.float32)
            if a.shape != (n, K):
                raise ValueError("x0 must be [n_rows, num_dim]")
        out = np.empty((n, K), dtype=np.float32)
        if not weighted_entry:
            _chk(self.lib, self.lib.cdae_hip_als_solve_rows(self.h, n, rp.ctypes.data, rc.ctypes.data, None if a is None else a.ctypes.data,
                                                            cg_steps, out.ctypes.data))
            return out
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.shape != rc.shape:
                raise ValueError("weights must hold one value per entry of col")
        _chk(self.lib, self.lib.cdae_hip_als_solve_rows_weighted(self.h, n, rp.ctypes.data, rc.ctypes.data, None if w is None else w.ctypes.data,
                                                                 None if a is None else a.ctypes.data, cg_steps, out.ctypes.data))
        return out

    def set_confidence(self, w):
        """Per-pair confidence weights: one finite value >= 0 per stored pair in the order of the train CSR's col (confidence
        1 + scalar * w); None returns the handle to binary.  set_interactions drops them."""
        if w is None:
            _chk(self.lib, self.lib.cdae_hip_als_set_confidence(self.h, None, 0))
            return
        a = np.ascontiguousarray(w, dtype=np.float32).ravel()
        _chk(self.lib, self.lib.cdae_hip_als_set_confidence(self.h, a.ctypes.data, a.size))

    def objective(self):
        """-> (data, penalty): sum over ALL pairs of c (p - x . y)^2 under the current confidences, and lambda (|X|^2 + |Y|^2)"""
        out = np.zeros(2, dtype=np.float64)
        _chk(self.lib, self.lib.cdae_hip_als_objective(self.h, out.ctypes.data))
        return float(out[0]), float(out[1])


@dataclass
class WARPConfig:
    """libcf::WARPConfig (the reference's src/model/recsys/warp.hpp:12-23) with its defaults; beta and using_bias_term are accepted as the
    reference accepts them and change nothing (warp.hpp never reads beta; the bias steps are comments).  batch_users is not in the
    reference: 1 (and 0) is its loop, above 1 the block schedule — no block size has been measured for accuracy."""
    learn_rate: float = 0.1
    beta: float = 0.0
    lambda_: float = 0.1
    lt: int = HINGE
    num_dim: int = 10
    num_neg: int = 5
    using_bias_term: bool = True
    using_adagrad: bool = True
    batch_users: int = 1


class WARP(MF):
    """Rank-weighted pairwise matrix factorisation whose negatives are searched for on the device (cdae_hip_create_warp; include/cdae_hip.h
    has the definition).  The factors and biases live where IMF's do; recommend_all, eval_topn and similar_items are MF's."""

    def __init__(self, mcfg: WARPConfig, device: int = 0):
        self.lib = load_library()
        self.cfg = mcfg
        c = _WarpConfig(C.sizeof(_WarpConfig), mcfg.num_dim, mcfg.num_neg, mcfg.lt, int(mcfg.using_adagrad), mcfg.batch_users,
                        mcfg.lambda_, mcfg.learn_rate)
        self.h = C.c_void_p()
        _chk(self.lib, self.lib.cdae_hip_create_warp(C.byref(c), device, C.byref(self.h)))
        self.num_users = self.num_items = 0
        self._rec = None

    def _pairs(self, pos_begin: int, pos_end: int) -> int:
        lens = np.diff(self._row_ptr)[self.user_order().astype(np.int64)]
        return int(lens[pos_begin:pos_end].sum()) * self.cfg.num_neg

    def search(self, seed: int, epoch: int, pos_begin: int = 0, pos_end: int | None = None, with_margin: bool = False):
        """The search of every (position, positive, k) of training positions [pos_begin, pos_end) against the current parameters; nothing
        is trained.  -> (item, cnt[, margin]) indexed by (row offset of the positive in the range) * num_neg + k; cnt == WARP_MAX_TRY
        and item == WARP_NONE: exhausted."""
        pos_end = self.num_users if pos_end is None else pos_end
        n = self._pairs(pos_begin, pos_end) if 0 <= pos_begin <= pos_end <= self.num_users else 0
        item, cnt = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        margin = np.empty(n, dtype=np.float32) if with_margin else None
        _chk(self.lib, self.lib.cdae_hip_warp_search(self.h, seed, epoch, pos_begin, pos_end, item.ctypes.data, cnt.ctypes.data,
                                                     None if margin is None else margin.ctypes.data, n))
        return (item, cnt, margin) if with_margin else (item, cnt)

    def record_choices(self, on):
        """on: every training call leaves the (item, cnt) of every pair of the users it trained (choices())"""
        _chk(self.lib, self.lib.cdae_hip_warp_record_choices(self.h, int(bool(on))))

    def choices(self):
        """-> (item, cnt) of every pair, [nnz * num_neg] in position order, as the last training calls left them"""
        n = self._pairs(0, self.num_users)
        item, cnt = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        _chk(self.lib, self.lib.cdae_hip_warp_choices(self.h, item.ctypes.data, cnt.ctypes.data, n))
        return item, cnt

    def _batch_examples(self, u_begin: int, n_users: int) -> int:
        return 2 * self._pairs(u_begin, u_begin + n_users)


@dataclass
class FISMConfig:
    """libcf::FISMConfig (the reference's src/model/recsys/fism.hpp:8-20) with its defaults and SGDConfig's learn rate; alpha is a real
    number here (the reference's is an int).  using_factor_term = False and using_global_mean are not taken over.  batch_users is not in
    the reference: 1 (and 0) is its loop; a block schedule is not built."""
    learn_rate: float = 0.1
    lambda_: float = 0.01
    lt: int = SQUARE
    num_dim: int = 10
    num_neg: int = 5
    alpha: float = 1.0
    using_bias_term: bool = True
    using_adagrad: bool = True
    batch_users: int = 1


class FISM(MF):
    """Factored item similarity (cdae_hip_create_fism; include/cdae_hip.h has the definition).  P = P_W, Q = P_V, bi = P_BP, bu = P_UB (and
    their *_AG accumulators); there is no user table.  A user is the sum of the rows of P of a rated set, so recommend_rows, eval_topn_rows,
    score_rows, full_rank_rows, recommend_rows_filtered (any rated sets) and similar_items (table "input" = P, "output" = Q) serve the handle
    as CDAE's methods do, beside recommend_all and eval_topn over the train rows."""

    _create = "cdae_hip_create_fism"

    def __init__(self, mcfg: FISMConfig, device: int = 0):
        self.lib = load_library()
        self.cfg = mcfg
        c = _FismConfig(C.sizeof(_FismConfig), mcfg.num_dim, mcfg.num_neg, mcfg.lt, int(mcfg.using_adagrad), int(mcfg.using_bias_term),
                        mcfg.batch_users, 0, mcfg.lambda_, mcfg.learn_rate, mcfg.alpha)
        self.h = C.c_void_p()
        _chk(self.lib, getattr(self.lib, self._create)(C.byref(c), device, C.byref(self.h)))
        self.num_users = self.num_items = 0
        self._rec = None

    def plan(self) -> dict:
        """{resident_rows, window_instances}: rows of a user the training kernel keeps on chip for a visit (0: all stream; 0 before
        set_interactions), and the instances one launch holds at most"""
        r, w = C.c_uint32(0), C.c_uint64(0)
        _chk(self.lib, self.lib.cdae_hip_fism_plan(self.h, C.byref(r), C.byref(w)))
        return dict(resident_rows=int(r.value), window_instances=int(w.value))

    def set_resident(self, allow: bool):
        """allow = False: every row streams through memory; both settings give the same bits"""
        _chk(self.lib, self.lib.cdae_hip_fism_set_resident(self.h, int(bool(allow))))

    def _batch_examples(self, u_begin: int, n_users: int) -> int:
        return int(self._row_ptr[u_begin + n_users] - self._row_ptr[u_begin]) * (1 + self.cfg.num_neg)


@dataclass
class FISMPConfig(FISMConfig):
    """libcf::FISMPConfig (the reference's src/model/recsys/fism_pair.hpp) with its defaults: lambda 0.01, SQUARE, 10 dimensions, 5 negatives,
    alpha 1, AdaGrad, bias terms.  lt is SQUARE (the paper's (1 - d)^2) or LOG (the BPR criterion on the difference); CROSS_ENTROPY is
    refused, its gradient at label 1 being LOG's."""


class FISMP(FISM):
    """FISMauc, the pairwise form of FISM (cdae_hip_create_fism_pair; include/cdae_hip.h has the definition): a FISM handle in everything
    but its training loop, which steps on pairs (rated item, drawn negative) of one shared neighbourhood vector.  There is no user bias:
    P_UB / P_UB_AG are not allocated.  stats.examples counts pairs, num_neg per stored interaction."""
    _create = "cdae_hip_create_fism_pair"

    def __init__(self, mcfg: FISMPConfig, device: int = 0):
        super().__init__(mcfg, device)

    def _batch_examples(self, u_begin: int, n_users: int) -> int:
        return int(self._row_ptr[u_begin + n_users] - self._row_ptr[u_begin]) * self.cfg.num_neg


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library: rank 0 makes it, every rank passes it to CDAE.comm_init_rank."""
    lib = load_library()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _chk(lib, lib.cdae_hip_comm_unique_id(buf, COMM_ID_BYTES))
    return buf.raw


COMBINE_SUM, COMBINE_GLOBAL_ACC = 0, 1


class _MultiSchedule(C.Structure):
    _fields_ = [("period", C.c_int32), ("combine", C.c_uint32), ("sync_batch_users", C.c_uint32), ("reserved", C.c_uint32),
                ("relay_epochs", C.c_double)]


class MultiCDAE:
    """Several user shards behind one handle (cdae_hip_multi_*): the data-parallel form of libcf::CDAE in one process.

    devices = [0, 1, ..., N-1]: one shard per GPU (RCCL); devices = [0] * N: N logical shards of GPU 0 (tests, accuracy
    envelope).  exchange_every: 0 = synchronous exchange of the shared-parameter deltas at every step, k >= 1 = pipelined."""

    def __init__(self, mcfg: CDAEConfig, devices, exchange_every: int = 0, item_rows: bool = False):
        """item_rows=True: CDAE_LAYOUT_ITEM_ROWS — the shards cut the item rows (exact single-GPU schedule, sampled or full-output decode; the user node sharded by user)."""
        self.lib = load_library()
        self.cfg = mcfg
        c = _Config(C.sizeof(_Config), mcfg.num_dim, mcfg.num_neg, mcfg.num_corruptions, mcfg.lt,
                    int(mcfg.using_adagrad), int(mcfg.asymmetric), int(mcfg.user_factor), int(mcfg.linear),
                    int(mcfg.scaled), int(mcfg.tanh), mcfg.batch_users, int(mcfg.full_output), int(mcfg.linear_function),
                    mcfg.lambda_, mcfg.learn_rate, mcfg.corruption_ratio, mcfg.beta)
        devs = (C.c_int * len(devices))(*devices)
        self.h = C.c_void_p()
        _chk(self.lib, self.lib.cdae_hip_multi_create(C.byref(c), len(devices), devs, C.byref(self.h)))
        _chk(self.lib, self.lib.cdae_hip_multi_set_exchange(self.h, exchange_every))
        if item_rows:
            _chk(self.lib, self.lib.cdae_hip_multi_set_layout(self.h, 1))
        self.num_users = self.num_items = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.cdae_hip_multi_destroy(self.h)
            self.h = None

    __del__ = close

    def set_exchange(self, period: int):
        _chk(self.lib, self.lib.cdae_hip_multi_set_exchange(self.h, period))

    def set_schedule(self, period: int = 0, combine: int = COMBINE_SUM, sync_batch_users: int = 0, relay_epochs: float = 0.0):
        """cdae_hip_multi_set_schedule (user-sharded layout): the first `relay_epochs` epochs (fractions allowed) on the single-GPU
        schedule handed from shard to shard, the rest as exchanged steps of `sync_batch_users` users per shard folded in by `combine`"""
        sc = _MultiSchedule(period, combine, sync_batch_users, 0, relay_epochs)
        _chk(self.lib, self.lib.cdae_hip_multi_set_schedule(self.h, C.byref(sc)))

    def set_interactions(self, num_users, num_items, row_ptr, col_idx):
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ci = np.ascontiguousarray(col_idx, dtype=np.uint32)
        _chk(self.lib, self.lib.cdae_hip_multi_set_interactions(self.h, num_users, num_items, rp.ctypes.data, ci.ctypes.data))
        self.num_users, self.num_items = int(num_users), int(num_items)

    def reset(self, train, seed: int = 0):
        self.set_interactions(train.num_users, train.num_items, train.train_ptr, train.train_col)
        self.init_params(seed)

    def init_params(self, seed: int):
        _chk(self.lib, self.lib.cdae_hip_multi_init_params(self.h, seed))

    def shard_profiling(self, shard: int, period: int, families=None):
        """cdae_hip_set_profiling (+ _families) on ONE shard's handle: HIP events around that shard's decode / row launches"""
        h = C.c_void_p()
        _chk(self.lib, self.lib.cdae_hip_multi_shard(self.h, shard, C.byref(h), None, None))
        _chk(self.lib, self.lib.cdae_hip_set_profiling(h, period))
        if families is not None:
            _chk(self.lib, self.lib.cdae_hip_set_profiling_families(h, sum(1 << f for f in families)))

    def shard_stats(self, shard: int) -> Stats:
        """the counters and HIP-event kernel times ONE shard's handle accumulated since they were last collected"""
        h = C.c_void_p()
        _chk(self.lib, self.lib.cdae_hip_multi_shard(self.h, shard, C.byref(h), None, None))
        st = Stats()
        _chk(self.lib, self.lib.cdae_hip_collect_stats(h, C.byref(st)))
        return st

    def shards(self):
        """[(u_begin, u_end)] of every shard"""
        out = []
        for s in range(self.lib.cdae_hip_multi_num_shards(self.h)):
            a, b = C.c_uint64(), C.c_uint64()
            _chk(self.lib, self.lib.cdae_hip_multi_shard(self.h, s, None, C.byref(a), C.byref(b)))
            out.append((a.value, b.value))
        return out

    def train_one_iteration(self, seed: int, epoch: int) -> Stats:
        st = Stats()
        _chk(self.lib, self.lib.cdae_hip_multi_train_epoch(self.h, seed, epoch, C.byref(st)))
        return st

    def train_users(self, seed: int, epoch: int, u_begin: int, u_end: int) -> Stats:
        st = Stats()
        _chk(self.lib, self.lib.cdae_hip_multi_train_users(self.h, seed, epoch, u_begin, u_end, C.byref(st)))
        return st

    @property
    def steps_per_epoch(self) -> int:
        """user-sharded layout: exchanged steps of one epoch (cdae_hip_multi_steps_per_epoch)"""
        return int(self.lib.cdae_hip_multi_steps_per_epoch(self.h))

    def train_steps(self, seed: int, epoch: int, step_begin: int, step_end: int) -> Stats:
        """steps [step_begin, step_end) of the epoch's exchanged part, no relay, flushed at the end (measurement hook)"""
        st = Stats()
        _chk(self.lib, self.lib.cdae_hip_multi_train_steps(self.h, seed, epoch, step_begin, step_end, C.byref(st)))
        return st

    def current_loss(self, seed: int, epoch: int) -> float:
        a, b = C.c_double(), C.c_double()
        _chk(self.lib, self.lib.cdae_hip_multi_data_loss(self.h, seed, epoch, C.byref(a)))
        _chk(self.lib, self.lib.cdae_hip_multi_penalty_loss(self.h, C.byref(b)))
        return a.value + b.value

    def recommend_all(self, topk: int = 10, u_begin: int = 0, u_end=None) -> np.ndarray:
        u_end = self.num_users if u_end is None else u_end
        out = np.empty((u_end - u_begin, topk), dtype=np.uint32)
        _chk(self.lib, self.lib.cdae_hip_multi_recommend_all(self.h, u_begin, u_end, topk, out.ctypes.data))
        return out

    def eval_topn(self, test_ptr, test_col, topk: int = 10):
        tp = np.ascontiguousarray(test_ptr, dtype=np.int64)
        tc = np.ascontiguousarray(test_col, dtype=np.uint32)
        rets, hits = np.empty(8, dtype=np.float64), np.empty(3, dtype=np.uint64)
        _chk(self.lib, self.lib.cdae_hip_multi_eval_topn(self.h, tp.ctypes.data, tc.ctypes.data, topk, rets.ctypes.data, hits.ctypes.data, None))
        return rets, hits

    _shape = CDAE._shape

    def shard_get(self, shard: int, which) -> np.ndarray:
        """a SHARED parameter (item-side matrices, biases) as ONE shard's replica holds it (user-sharded layout: the replicas must agree)"""
        h = C.c_void_p()
        _chk(self.lib, self.lib.cdae_hip_multi_shard(self.h, shard, C.byref(h), None, None))
        out = np.empty(self._shape(which), dtype=np.float32)
        _chk(self.lib, self.lib.cdae_hip_get_param(h, which, out.ctypes.data, out.size))
        return out

    def get(self, which) -> np.ndarray:
        out = np.empty(self._shape(which), dtype=np.float32)
        _chk(self.lib, self.lib.cdae_hip_multi_get_param(self.h, which, out.ctypes.data, out.size))
        return out

    def set(self, which, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(self._shape(which))
        _chk(self.lib, self.lib.cdae_hip_multi_set_param(self.h, which, a.ctypes.data, a.size))
