"""The C-ABI of ``include/fleet_codec.h`` as ctypes: constants, errors, the signature table,
``lib()``, and the small helpers every wrapper module shares. Imports nothing of the package."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
# FLEET_CODEC_LIB: load another build of the same C-ABI (A/B experiments on one box)
LIB_PATH = os.environ.get("FLEET_CODEC_LIB") or os.path.join(PKG, "libfleetcodec.so")
HEADER_PATH = os.path.join(ROOT, "include", "fleet_codec.h")

FLEET_OK = 0
FLEET_ERR_ARG = -1
FLEET_ERR_BASE64 = -2
FLEET_ERR_LAYOUT = -3
FLEET_ERR_HIP = -4
FLEET_ERR_NOMEM = -5
FLEET_ERR_CAPACITY = -6
FLEET_MAX_HEADERS = 4096


# new_solver's names (commonLib/cppNN/solver.h:198-208) in FLEET_SOLVER_* order
SOLVERS = ("sgd", "adagrad", "rmsprop", "adam")


class FleetError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class Base64Error(FleetError):
    pass


class LayoutError(FleetError):
    pass


_lib = None

# argument and result types of every entry point lib() binds, by name
sz, vp, i32, i64 = C.c_size_t, C.c_void_p, C.c_int, C.c_int64
szp = C.POINTER(C.c_size_t)
SIGNATURES = {
    "fleet_version": (C.c_char_p, []),
    "fleet_create": (i32, [i32, C.POINTER(vp)]),
    "fleet_destroy": (None, [vp]),
    "fleet_last_error": (C.c_char_p, [vp]),
    "fleet_sync": (i32, [vp, vp]),
    "fleet_check": (i32, [vp, vp]),
    "fleet_b64_len": (sz, [sz]),
    "fleet_b64_count": (sz, [sz]),
    "fleet_layout_from_sizes": (i32, [vp, i32, vp, i32, vp, i32, C.POINTER(i32), szp]),
    "fleet_layout_parse": (i32, [vp, vp, sz, vp, i32, C.POINTER(i32), szp]),
    "fleet_encode_f32": (i32, [vp, vp, sz, vp, sz, szp]),
    "fleet_encode_i32": (i32, [vp, vp, sz, vp, sz, szp]),
    "fleet_decode_f32": (i32, [vp, vp, sz, vp, sz, szp]),
    "fleet_decode_i32": (i32, [vp, vp, sz, vp, sz, szp]),
    "fleet_flat_gradient": (i32, [vp, vp, sz, vp, sz, szp]),
    "fleet_merge_flat_gradient": (i32, [vp, vp, sz, vp, sz, vp, sz, szp]),
    "fleet_scalar_mul": (i32, [vp, vp, sz, C.c_double, vp, sz, szp]),
    "fleet_add": (i32, [vp, vp, sz, vp, sz, vp, sz, szp]),
    "fleet_subtract": (i32, [vp, vp, sz, vp, sz, vp, sz, szp]),
    "fleet_norm": (i32, [vp, vp, sz, C.POINTER(C.c_double)]),
    "fleet_update": (i32, [vp, vp, vp, i32, vp, vp, sz, szp, vp]),
    "fleet_update_multi": (i32, [vp, i32, vp, vp, i32, vp, vp, sz, szp, vp]),
    "fleet_update_rows": (i32, [vp, vp, sz, sz, i32, vp, vp, sz, szp, vp]),
    "fleet_update_rows_multi": (i32, [vp, i32, vp, sz, sz, i32, vp, vp, sz, szp, vp]),
    "fleet_host_register": (i32, [vp, vp, sz]),
    "fleet_host_unregister": (i32, [vp, vp]),
    "fleet_update_device": (i32, [vp, vp, sz, sz, i32, vp, vp, i32, sz, sz, vp, vp, vp]),
    "fleet_update_encode_device": (i32, [vp, vp, sz, sz, i32, vp, vp, i32, vp, vp, vp, sz, vp, vp]),
    "fleet_update_kardam_device": (i32, [vp, vp, sz, sz, i32, vp, vp, i32, C.c_double, vp, vp, vp, sz, vp, vp,
                                         vp, vp, vp]),
    "fleet_acc_create": (i32, [vp, sz, vp, i32, sz, sz, C.POINTER(vp)]),
    "fleet_acc_destroy": (None, [vp]),
    "fleet_acc_push": (i32, [vp, vp, sz, C.c_double]),
    "fleet_acc_push_device": (i32, [vp, vp, C.c_double, vp]),
    "fleet_acc_count": (i32, [vp]),
    "fleet_acc_finish": (i32, [vp, vp, sz, szp, vp]),
    "fleet_acc_finish_device": (i32, [vp, vp, vp, vp]),
    "fleet_acc_reset": (i32, [vp]),
    "fleet_acc_push_many": (i32, [vp, vp, vp, i32, vp]),
    "fleet_acc_push_many_device": (i32, [vp, vp, sz, i32, vp, vp]),
    "fleet_acc_push_finish": (i32, [vp, vp, vp, i32, vp, vp, sz, szp, vp]),
    "fleet_acc_push_finish_device": (i32, [vp, vp, sz, i32, vp, vp, vp, vp]),
    "fleet_acc_burst": (i32, []),
    "fleet_pool_create": (i32, [vp, sz, vp, i32, sz, sz, i32, C.POINTER(vp)]),
    "fleet_pool_destroy": (None, [vp]),
    "fleet_pool_slots": (i32, [vp]),
    "fleet_pool_occupied": (i32, [vp, i32]),
    "fleet_pool_put": (i32, [vp, i32, vp, sz]),
    "fleet_pool_put_device": (i32, [vp, i32, vp, vp]),
    "fleet_pool_drop": (i32, [vp, i32]),
    "fleet_pool_update": (i32, [vp, vp, i32, vp, vp, sz, szp, vp]),
    "fleet_pool_update_device": (i32, [vp, vp, i32, vp, vp, vp, vp]),
    "fleet_pool_slot_status": (i32, [vp, i32]),
    "fleet_gate_header_codes": (i32, [vp, i32, vp]),
    "fleet_gate_create": (i32, [vp, vp, i32, C.POINTER(vp)]),
    "fleet_gate_destroy": (None, [vp]),
    "fleet_gate_vet": (i32, [vp, vp, i32, vp, vp, vp]),
    "fleet_gate_vet_device": (i32, [vp, vp, i32, vp, vp, vp, vp]),
    "fleet_gate_put": (i32, [vp, i32, vp, sz, vp, vp, vp]),
    "fleet_kledger_create": (i32, [vp, i32, i32, C.POINTER(vp)]),
    "fleet_kledger_destroy": (None, [vp]),
    "fleet_kledger_workers": (i32, [vp]),
    "fleet_kledger_has": (i32, [vp, i32]),
    "fleet_kledger_epoch": (i32, [vp, i32, C.POINTER(i32)]),
    "fleet_kledger_forget": (i32, [vp, i32]),
    "fleet_kledger_read": (i32, [vp, i32, vp, sz]),
    "fleet_kledger_update": (i32, [vp, vp, i32, vp, vp, vp, C.c_double, vp, sz, szp, vp, vp, vp, vp]),
    "fleet_kledger_update_device": (i32, [vp, vp, i32, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp]),
    "fleet_kfilter_create": (i32, [vp, sz, sz, i32, C.POINTER(vp)]),
    "fleet_kfilter_destroy": (None, [vp]),
    "fleet_kfilter_has_last": (i32, [vp]),
    "fleet_kfilter_set_model": (i32, [vp, vp, vp, vp, vp]),
    "fleet_kfilter_set_model_device": (i32, [vp, vp, vp, vp, vp, vp]),
    "fleet_kfilter_update": (i32, [vp, vp, i32, vp, vp, vp, C.c_double, vp, sz, szp, vp, vp, vp, vp, vp, vp]),
    "fleet_kfilter_update_device": (i32, [vp, vp, i32, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]),
    "fleet_kfilter_resolve": (i32, [vp, vp, i32, vp, sz, szp, vp]),
    "fleet_kfilter_resolve_device": (i32, [vp, vp, i32, vp, vp, szp, vp]),
    "fleet_mledger_create": (i32, [vp, sz, sz, i32, i32, i32, C.POINTER(vp)]),
    "fleet_mledger_destroy": (None, [vp]),
    "fleet_mledger_shape": (i32, [vp, szp, szp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "fleet_mledger_launch_shape": (i32, [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "fleet_mledger_stage": (i32, [vp, i64, vp, vp]),
    "fleet_mledger_stage_device": (i32, [vp, i64, vp, vp, vp]),
    "fleet_mledger_resident": (i32, [vp, i64]),
    "fleet_mledger_update": (i32, [vp, vp, vp, i32, vp, vp, vp]),
    "fleet_mledger_has": (i32, [vp, i32]),
    "fleet_mledger_version": (i32, [vp, i32, C.POINTER(i64)]),
    "fleet_mledger_forget": (i32, [vp, i32]),
    "fleet_mledger_read": (i32, [vp, i32, vp, sz]),
    "fleet_mledger_read_version": (i32, [vp, i64, vp, sz]),
    "fleet_mledger_stage_model": (i32, [vp, vp, i32, C.POINTER(i64)]),
    "fleet_model_version_id": (i32, [vp, i32, C.POINTER(i64)]),
    "fleet_update_kernel": (C.c_char_p, [sz]),
    "fleet_update_plan_grid": (i32, [sz, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "fleet_update_encode_kernel": (C.c_char_p, [sz]),
    "fleet_set_plan": (i32, [C.c_char_p, vp, sz]),
    "fleet_plan": (C.c_char_p, []),
    "fleet_model_quantize_index": (i32, [vp, vp, vp, i32, vp, vp, vp, vp]),
    "fleet_model_weights_text": (i32, [vp, vp, vp, i32, vp, sz, szp]),
    "fleet_model_read_weights": (i32, [vp, vp, sz, vp, i32, vp]),
    "fleet_values_text": (i32, [vp, vp, sz, vp, i32, vp, sz, szp]),
    "fleet_values_text_device": (i32, [vp, vp, sz, vp, i32, vp, sz, szp, vp]),
    "fleet_encode_device": (i32, [vp, vp, sz, sz, i32, vp, sz, vp]),
    "fleet_decode_device": (i32, [vp, vp, sz, sz, i32, vp, sz, vp]),
    "fleet_synth_device": (i32, [vp, C.c_uint64, i32, i32, vp, vp, i32, sz, vp, sz, vp]),
    "fleet_synth_window_device": (i32, [vp, C.c_uint64, i32, i32, sz, vp, vp, i32, sz, vp, sz, vp]),
    "fleet_selftest_digest": (i32, [vp, i32, C.POINTER(C.c_uint64)]),
    "fleet_descent_device": (i32, [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, C.c_float, vp]),
    "fleet_descent": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, vp, i32, vp, vp, i32, C.c_float]),
    "fleet_solver_from_name": (i32, [C.c_char_p]),
    "fleet_descent_solver_device": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, C.c_float, vp]),
    "fleet_descent_solver": (i32, [vp, i32, vp, sz, vp, vp, vp, sz, vp, sz, vp, vp, i32, vp, vp, i32, C.c_float]),
    "fleet_model_set_solver": (i32, [vp, C.c_char_p]),
    "fleet_model_solver": (i32, [vp]),
    "fleet_model_solver_state": (i32, [vp, i32, vp, sz]),
    "fleet_rmodel_set_solver": (i32, [vp, C.c_char_p]),
    "fleet_rmodel_solver": (i32, [vp]),
    "fleet_rmodel_solver_state": (i32, [vp, i32, vp, sz]),
    "fleet_model_params": (i32, [vp, vp, sz, vp, sz, i32, vp, sz, szp]),
    "fleet_model_version": (i32, [vp, vp, vp, i32, vp, sz, vp, vp]),
    "fleet_model_params_device": (i32, [vp, vp, sz, vp, sz, i32, vp, vp]),
    "fleet_minibatch_len": (sz, [i32, i32, i32, i32]),
    "fleet_test_kardam_skew": (i32, [vp, C.c_uint]),
    "fleet_kardam_grads": (i32, [vp, vp, vp, i32, vp, C.c_double, vp, vp, sz, szp, vp, vp]),
    "fleet_descent_window_device": (i32, [vp, vp, vp, vp, sz, sz, vp, vp, i32, vp, vp, i32, C.c_float, vp]),
    "fleet_minibatch_device": (i32, [vp, vp, sz, i32, vp, vp, i32, vp, i32, vp, vp, vp]),
    "fleet_minibatch": (i32, [vp, vp, sz, i32, vp, vp, i32, vp, i32, vp, vp, sz, szp]),
    "fleet_teacher_weight_count": (sz, []),
    "fleet_teacher_bias_count": (sz, []),
    "fleet_teacher_forward_device": (i32, [vp, vp, vp, vp, sz, i32, vp, i32, C.c_float, vp, vp]),
    "fleet_teacher_forward": (i32, [vp, vp, sz, vp, sz, vp, sz, i32, vp, i32, C.c_float, vp]),
    "fleet_evaluate_block_images": (sz, []),
    "fleet_evaluate_set_grid": (i32, [i32]),
    "fleet_evaluate_device": (i32, [vp, vp, vp, vp, sz, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
    "fleet_evaluate": (i32, [vp, vp, sz, vp, sz, vp, sz, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
    "fleet_model_evaluate": (i32, [vp, i32, vp, sz, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
    "fleet_rmodel_evaluate": (i32, [vp, i32, vp, sz, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
    "fleet_rmodel_evaluate_device": (i32, [vp, i32, vp, sz, i32, vp, vp, i32, vp, vp, vp, vp]),
    "fleet_cifar_weight_count": (sz, [i32]),
    "fleet_cifar_bias_count": (sz, [i32]),
    "fleet_cifar_block_images": (sz, []),
    "fleet_cifar_set_grid": (i32, [i32]),
    "fleet_cifar_test_device": (i32, [vp, i32, vp, vp, vp, sz, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
    "fleet_cifar_test": (i32, [vp, i32, vp, sz, vp, sz, vp, sz, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "fleet_model_cifar_test": (i32, [vp, i32, vp, sz, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
    "fleet_rmodel_cifar_test": (i32, [vp, i32, vp, sz, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
    "fleet_rmodel_cifar_test_device": (i32, [vp, i32, vp, sz, i32, vp, vp, i32, vp, vp, vp, vp]),
    "fleet_client_grad_len": (sz, []),
    "fleet_client_grad_set_chunk": (i32, [i32]),
    "fleet_client_grads_device": (i32, [vp, vp, sz, i32, vp, vp, sz, i32, vp, vp, vp, i32, i32, C.c_float, vp, sz, vp,
                                        sz, vp]),
    "fleet_client_grads": (i32, [vp, vp, sz, vp, sz, vp, sz, i32, vp, vp, vp, i32, i32, C.c_float, vp, vp, sz]),
    "fleet_rmodel_client_grads_device": (i32, [vp, vp, vp, sz, i32, vp, vp, vp, i32, i32, C.c_float, vp, sz, vp, sz,
                                               vp]),
    "fleet_client_ex_grads_device": (i32, [vp, vp, sz, i32, vp, vp, sz, i32, vp, vp, vp, i32, i32, C.c_float, i32, vp, vp,
                                           vp, sz, vp, sz, vp]),
    "fleet_client_ex_grads": (i32, [vp, vp, sz, vp, sz, vp, sz, i32, vp, vp, vp, i32, i32, C.c_float, i32, vp, vp, vp,
                                    vp, sz]),
    "fleet_rmodel_client_ex_grads_device": (i32, [vp, vp, vp, sz, i32, vp, vp, vp, i32, i32, C.c_float, i32, vp, vp, vp,
                                                  sz, vp, sz, vp]),
    "fleet_client_dp_noise": (i32, [vp, sz]),
    "fleet_model_load": (i32, [vp, vp, sz, i32, C.POINTER(vp)]),
    "fleet_model_destroy": (None, [vp]),
    "fleet_model_last_error": (C.c_char_p, [vp]),
    "fleet_model_init_updater": (i32, [vp, vp, i32]),
    "fleet_model_descent": (i32, [vp, vp, sz, i32, i32]),
    "fleet_model_count": (i32, [vp]),
    "fleet_model_get_params": (i32, [vp, i32, vp, sz, szp]),
    "fleet_model_get_model_params": (i32, [vp, i32, vp, sz, szp]),
    "fleet_model_get_epoch": (i32, [vp]),
    "fleet_model_set_epoch": (None, [vp, i32]),
    "fleet_model_get_priority": (i32, [vp]),
    "fleet_model_set_priority": (None, [vp, i32]),
    "fleet_model_get_lrate": (C.c_double, [vp]),
    "fleet_model_shape": (i32, [vp, szp, szp, C.POINTER(i32), C.POINTER(i32)]),
    "fleet_model_export": (i32, [vp, i32, vp, sz, vp, sz]),
    "fleet_ctx_device": (i32, [vp]),
    "fleet_ctx_of_mledger": (vp, [vp]),
    "fleet_rmodel_load": (i32, [vp, vp, sz, i32, i32, C.POINTER(vp)]),
    "fleet_rmodel_destroy": (None, [vp]),
    "fleet_rmodel_last_error": (C.c_char_p, [vp]),
    "fleet_rmodel_init_updater": (i32, [vp, vp, i32]),
    "fleet_rmodel_descent": (i32, [vp, vp, sz, i32, i32]),
    "fleet_rmodel_descent_device": (i32, [vp, vp, sz, i32, vp]),
    "fleet_rmodel_count": (i32, [vp]),
    "fleet_rmodel_params_cap": (sz, [vp]),
    "fleet_rmodel_get_params": (i32, [vp, i32, vp, sz, szp]),
    "fleet_rmodel_get_model_params": (i32, [vp, i32, vp, sz, szp]),
    "fleet_rmodel_get_model_params_device": (i32, [vp, i32, vp, vp]),
    "fleet_rmodel_get_epoch": (i32, [vp]),
    "fleet_rmodel_set_epoch": (None, [vp, i32]),
    "fleet_rmodel_get_priority": (i32, [vp]),
    "fleet_rmodel_set_priority": (None, [vp, i32]),
    "fleet_rmodel_get_lrate": (C.c_double, [vp]),
    "fleet_rmodel_shape": (i32, [vp, szp, szp, C.POINTER(i32), C.POINTER(i32)]),
    "fleet_rmodel_export": (i32, [vp, i32, vp, sz, vp, sz]),
    "fleet_rmodel_version_id": (i32, [vp, i32, C.POINTER(i64)]),
    "fleet_rmodel_version_device": (i32, [vp, i32, C.POINTER(vp), C.POINTER(vp)]),
    "fleet_rmodel_stage_mledger": (i32, [vp, vp, i32, C.POINTER(i64)]),
    "fleet_rmodel_stats": (i32, [vp, szp, C.POINTER(i32)]),
    "fleet_rmodel_workspace_bytes": (sz, [vp]),
    "fleet_sampler_create": (i32, [vp, C.c_char_p, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    "fleet_sampler_create_from": (i32, [vp, vp, vp, sz, i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    "fleet_sampler_destroy": (None, [vp]),
    "fleet_sampler_last_error": (C.c_char_p, [vp]),
    "fleet_last_ingress": (i32, [vp]),
    "fleet_updater_reseed_ex": (None, [i32, i32]),
    "fleet_updater_reseed": (None, [i32]),
    "fleet_sampler_set_hyper": (i32, [vp, i32, C.c_double, C.c_double]),
    "fleet_sampler_set_teacher": (i32, [vp, vp, sz, vp, sz]),
    "fleet_sampler_minibatch": (i32, [vp, i32, C.c_float, vp, sz, szp]),
    "fleet_sampler_minibatch_len": (sz, [vp, i32]),
    "fleet_sampler_num_labels": (i32, [vp]),
    "fleet_sampler_has_outlier": (i32, [vp]),
    "fleet_sampler_num_samples": (sz, [vp]),
    "fleet_sampler_bucket": (i32, [vp, i32, vp, sz, szp]),
    "fleet_sampler_sorted_index": (i32, [vp, vp, sz, szp]),
    "fleet_sampler_last_indices": (i32, [vp, vp, sz, szp]),
}


def lib() -> C.CDLL:
    """Load libfleetcodec.so (build it with ``python -m fleet_amd.build``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -m fleet_amd.build` (HIP extension not built)")
    # One HIP runtime per process: when torch (ROCm build) is present, load it first so
    # libfleetcodec.so binds to the libamdhip64 torch already mapped (two runtimes in
    # one process cannot share streams/pointers and the second fails to initialise).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    ab_build = bool(os.environ.get("FLEET_CODEC_LIB"))
    for name, (res, args) in SIGNATURES.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            if ab_build:  # an A/B build from an older commit: entry points it predates stay unbound
                continue
            raise
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def exported_symbols_from_header(path: str = HEADER_PATH):
    """Function names declared in include/fleet_codec.h."""
    import re
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fleet_[a-z0-9_]+)\s*\(", text)))


def b64_len(n_values: int) -> int:
    """Base64 length of n int32 values: 4*ceil(4n/3) (Base64.cpp:129-136)."""
    return 4 * ((4 * n_values + 2) // 3)


def b64_count(length: int) -> int:
    return 3 * length // 16


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(stream):
    """Device calls default to torch's current stream so they order with torch ops
    (NULL = the null stream, which is torch's default stream)."""
    if stream is not None:
        return C.c_void_p(int(stream)) if int(stream) else None
    try:
        import torch
        if torch.cuda.is_available():
            h = torch.cuda.current_stream().cuda_stream
            return C.c_void_p(h) if h else None
    except ImportError:
        pass
    return None


def _as_bytes(x) -> bytes:
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, str):
        return x.encode("ascii")
    raise TypeError(f"expected Base64 bytes, got {type(x)}")


def raise_for(rc: int, msg: str):
    """The exception of a failed call's return code."""
    if rc == FLEET_ERR_BASE64:
        raise Base64Error(rc, msg)
    if rc == FLEET_ERR_LAYOUT:
        raise LayoutError(rc, msg)
    raise FleetError(rc, msg)


class Handle:
    """Lifecycle of one C handle ``_h`` of the library ``_L``. A subclass names its destroy
    function, the owners up the chain (attribute paths from ``self``; destroy is called only
    while each of them still has its own ``_h``, since the library frees a handle's parts with
    its owner) and the message ``_live`` raises."""

    _destroy = ""
    _owners = ()
    _closed = "the handle is closed"

    def _open(self) -> bool:
        if not getattr(self, "_h", None):  # closed, or __init__ raised before there was a handle
            return False
        for path in self._owners:
            o = self
            for name in path.split("."):
                o = getattr(o, name)
            if not getattr(o, "_h", None):
                return False
        return True

    def close(self):
        if self._open():
            getattr(self._L, self._destroy)(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _live(self):
        if not self._open():
            raise ValueError(self._closed)
        return self._h


def upload_args(uploads, dampens):
    """Host uploads and their dampening factors as a C call takes them:
    (the byte strings, char* array, lengths, dampens)."""
    ups = [_as_bytes(u) for u in uploads]
    if not ups:
        raise ValueError("no uploads")
    if len(dampens) != len(ups):
        raise ValueError("one dampening factor per upload")
    arr = (C.c_char_p * len(ups))(*ups)
    lens = np.array([len(u) for u in ups], dtype=np.uint64)
    d = np.ascontiguousarray(dampens, dtype=np.float64)
    return ups, arr, lens, d


def merged_out(length: int, want_f32: bool):
    """Host out-buffers of a merged gradient of ``length`` Base64 bytes: (out, n, f32 or None).
    Zeroed: a windowed form writes only its window of them."""
    return (np.zeros(length + 16, np.uint8), C.c_size_t(0),
            np.zeros(b64_count(length) + 1, np.float32) if want_f32 else None)


def merged_pair(length: int, out, n, f32):
    """:func:`merged_out`'s buffers after the call as (merged bytes, f32 values or None)."""
    return out[: n.value].tobytes(), None if f32 is None else f32[: b64_count(length)].copy()


def merged_result(length: int, out, n, f32, empty_is_none: bool = False):
    """What the host forms return: the merged bytes, or ``(bytes, f32)`` where f32 was asked
    for; None for an empty result if so asked."""
    if empty_is_none and n.value == 0:
        return None
    merged, values = merged_pair(length, out, n, f32)
    return merged if values is None else (merged, values)


def merged_ptrs(merged_u8, merged_f32, groups: int, length: int):
    """The two pointers of the device tensors a merged gradient of ``groups`` 16-byte groups
    is written to (merged_f32 may be None), after checking their sizes."""
    if merged_u8.numel() < 16 * groups or (
            merged_f32 is not None and merged_f32.numel() < b64_count(length)):
        raise ValueError("merged tensors smaller than the upload's groups")
    return merged_u8.data_ptr(), merged_f32.data_ptr() if merged_f32 is not None else None
