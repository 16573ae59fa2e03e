"""fleet_amd -- MI355X-native FLeet gradient codec + server-side aggregation.

Python host layer over the C-ABI of ``include/fleet_codec.h`` (libfleetcodec.so,
gfx950 HIP kernels). It mirrors the reference's native surface:

* :class:`Codec` -- one device context; the JNI natives of the reference's
  server backend (Server/src/main/c++/cppNN_backend.cpp) as methods with the
  same names and argument meaning (``getFlatGradient``, ``mergeFlatGradient``,
  ``scalarMulNative``, ``addNative``, ``subtractNative``, ``getNorm``) plus the
  fused batched ``update`` and the device-resident entry points.
* :class:`ByteVec` -- mirror of Server/src/main/java/utils/ByteVec.java.
* :mod:`fleet_amd.updater` -- mirror of CppNNUpdater's aggregation logic.

There is no CPU compute path: if the HIP library is missing or no GPU is
visible, constructing a :class:`Codec` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from .layouts import LAYOUTS, Layout  # noqa: F401

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
    sz, vp, i32, i64 = C.c_size_t, C.c_void_p, C.c_int, C.c_int64
    szp = C.POINTER(C.c_size_t)
    sig = {
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
    ab_build = bool(os.environ.get("FLEET_CODEC_LIB"))
    for name, (res, args) in sig.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            if ab_build:  # an A/B build from an older commit: entry points it predates stay unbound
                continue
            raise
        f.restype = res
        f.argtypes = args
    _ = i64
    _lib = L
    return L


def __getattr__(name):
    # ACC_BURST: uploads one k_acc_push_many launch folds (fleet_acc_burst), read from the
    # library when first asked for, so importing the package does not load it
    if name == "ACC_BURST":
        v = globals()["ACC_BURST"] = int(lib().fleet_acc_burst())
        return v
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


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


def update_kernel(length: int) -> str:
    """Aggregation kernel the library launches for uploads of `length` bytes."""
    return lib().fleet_update_kernel(length).decode()


def update_plan_grid(length: int) -> dict:
    """The aggregation's launch grid for uploads of `length` bytes (fleet_update_plan_grid):
    kind ("stream" / "tiled" / "pipe" / "weave" / "flat"), blocks, and n_a / n_w / n_n (see fleet_codec.h)."""
    k = C.c_int()
    b, a, w, n = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib().fleet_update_plan_grid(length, C.byref(k), C.byref(b), C.byref(a), C.byref(w), C.byref(n))
    if rc != 0:
        raise FleetError(f"fleet_update_plan_grid: {rc}")
    return {"kind": ("stream", "tiled", "pipe", "weave", "flat")[k.value], "blocks": b.value, "n_a": a.value, "n_w": w.value,
            "n_n": n.value}


def update_encode_kernel(length: int) -> str:
    """What fleet_update_encode_device launches for uploads of `length` bytes: the fused
    k_update_encode on the stream grid, k_update_tiled_encode on the wide tiles,
    k_update_pipe with the encode's blocks appended on the pipelined tiles."""
    return lib().fleet_update_encode_kernel(length).decode()


def set_plan(spec: str = "") -> None:
    """Launch-plan overrides (fleet_set_plan; process-wide): "update=auto|stream|tiled|pipe",
    "grid=auto|plain|balanced|lanes", "tile=auto|classic|flat|weave6|weave8", "flat_w2=auto|N",
    "tile_enc_prio=auto|0..3", "tile_enc_rows=N", "fused=on|off", "stage_threads=N",
    "stage_pieces=N", comma-separated; "" restores the measured default. Results are
    identical under every plan; an invalid spec raises and changes nothing."""
    err = C.create_string_buffer(256)
    rc = lib().fleet_set_plan(spec.encode(), err, 256)
    if rc != FLEET_OK:
        raise FleetError(rc, err.value.decode())


def plan() -> str:
    """The active launch-plan overrides ("" = the measured default)."""
    return lib().fleet_plan().decode()


class plan_override:
    """Context manager: `with plan_override("update=tiled"): ...` restores the previous plan."""

    def __init__(self, spec: str):
        self.spec = spec

    def __enter__(self):
        self.prev = plan()
        set_plan(self.spec)
        return self

    def __exit__(self, *exc):
        set_plan(self.prev)
        return False


class Evaluation:
    """What the Driver's ``test()`` returns for a model (Driver/src/main/c++/cppNN_backend.cpp:53-75)
    -- ``error`` and ``accuracy``, the ``valE, valA`` of FLeet's CSV lines -- with the count of
    correct images and, per image, the predicted class and its probability. Unpacks as
    ``error, accuracy``, the tuple the reference returns."""

    __slots__ = ("error", "accuracy", "correct", "predictions", "probabilities")

    def __init__(self, error, accuracy, correct, predictions, probabilities):
        self.error, self.accuracy, self.correct = error, accuracy, correct
        self.predictions, self.probabilities = predictions, probabilities

    def __iter__(self):
        return iter((self.error, self.accuracy))

    def __repr__(self):
        return f"Evaluation(error={self.error!r}, accuracy={self.accuracy!r}, correct={self.correct!r})"


def evaluate_block_images() -> int:
    """Images a block of the evaluation's forward kernel takes at a time."""
    return int(lib().fleet_evaluate_block_images())


class evaluate_grid_override:
    """``with evaluate_grid_override(2): ...`` caps the evaluation kernel's grid at that many
    blocks, so that a small set walks more than one grid-stride pass (tests; process-wide, as
    :class:`plan_override`)."""

    def __init__(self, max_blocks: int):
        self.max_blocks = int(max_blocks)

    def __enter__(self):
        self.prev = lib().fleet_evaluate_set_grid(self.max_blocks)
        return self

    def __exit__(self, *exc):
        lib().fleet_evaluate_set_grid(self.prev)
        return False


def _eval_host_args(images, labels, idx):
    x = np.ascontiguousarray(images, dtype=np.float32)
    if x.ndim == 1:
        x = x.reshape(1, -1)
    lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    if x.ndim != 2 or len(lab) != x.shape[0]:
        raise ValueError("images [N, F] and one label per image")
    ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
    return x, lab, ix, (x.shape[0] if ix is None else len(ix))


def _eval_host_call(fn, head, images, labels, idx):
    """one of the host-buffer evaluate entry points: fn(*head, images .., outputs ..) -> (rc, Evaluation)"""
    x, lab, ix, B = _eval_host_args(images, labels, idx)
    err, acc, cor = C.c_float(0), C.c_float(0), C.c_int32(0)
    pred, prob = np.empty(max(B, 1), np.int32), np.empty(max(B, 1), np.float32)
    rc = fn(*head, x.ctypes.data, x.shape[0], x.shape[1], lab.ctypes.data, None if ix is None else ix.ctypes.data, B,
            C.byref(err), C.byref(acc), C.byref(cor), pred.ctypes.data, prob.ctypes.data)
    return rc, Evaluation(np.float32(err.value), np.float32(acc.value), int(cor.value), pred[:B], prob[:B])


def _eval_device_out(images_f32, labels_i32, idx, out):
    """shapes and output tensors of a device evaluation: (n_images, F, B, out dict)"""
    import torch
    if images_f32.dim() != 2 or labels_i32.numel() != images_f32.shape[0]:
        raise ValueError("images [N, F] and one label per image")
    for t, dt, name in ((images_f32, torch.float32, "images"), (labels_i32, torch.int32, "labels"), (idx, torch.int32, "idx")):
        if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous()):
            raise ValueError(f"{name}: a contiguous {dt} CUDA tensor")
    B = images_f32.shape[0] if idx is None else idx.numel()
    dev = images_f32.device
    o = dict(out) if out else {}
    o.setdefault("predictions", torch.empty(B, dtype=torch.int32, device=dev))
    o.setdefault("probabilities", torch.empty(B, dtype=torch.float32, device=dev))
    o.setdefault("result", torch.empty(3, dtype=torch.float32, device=dev))
    for k, n, dt in (("predictions", B, torch.int32), ("probabilities", B, torch.float32), ("result", 3, torch.float32),
                     ("costs", B, torch.float32), ("probs10", 10 * B, torch.float32)):
        t = o.get(k)
        if t is not None and (t.dtype != dt or t.numel() < n or not t.is_cuda or not t.is_contiguous()):
            raise ValueError(f"out[{k!r}]: a contiguous {dt} CUDA tensor of at least {n} elements")
    return images_f32.shape[0], images_f32.shape[1], B, o


def _ptr(t):
    return None if t is None else t.data_ptr()


def evaluation_from_device(out) -> Evaluation:
    """The :class:`Evaluation` of a device evaluation's output tensors (synchronises on the copy)."""
    r = out["result"].cpu().numpy()
    pred, prob = out.get("predictions"), out.get("probabilities")
    return Evaluation(r[0], r[1], int(r[2:3].view(np.int32)[0]),
                      None if pred is None else pred.cpu().numpy(), None if prob is None else prob.cpu().numpy())


def layout_from_sizes(w_sizes: Sequence[int], b_sizes: Sequence[int]):
    """Header slot positions + n_up of the gradients() layout (network.h:1038-1056)."""
    w = np.ascontiguousarray(w_sizes, dtype=np.int32)
    b = np.ascontiguousarray(b_sizes, dtype=np.int32)
    cap = len(w) + len(b) + 2
    pos = np.empty(cap, np.int32)
    nh = C.c_int(0)
    n_up = C.c_size_t(0)
    rc = lib().fleet_layout_from_sizes(w.ctypes.data, len(w), b.ctypes.data, len(b), pos.ctypes.data, cap,
                                       C.byref(nh), C.byref(n_up))
    if rc != FLEET_OK:
        raise FleetError(rc, "bad layout sizes")
    return pos[: nh.value].copy(), int(n_up.value)


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


class Codec:
    """One HIP device context (``fleet_ctx``). Raises if no GPU / library."""

    def __init__(self, device: int = 0):
        L = lib()
        h = C.c_void_p()
        rc = L.fleet_create(device, C.byref(h))
        if rc != FLEET_OK:
            raise FleetError(rc, f"fleet_create(device={device}) failed: no usable MI355X/HIP device")
        self._h = h
        self._L = L
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.fleet_destroy(self._h)
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

    # -- error plumbing -------------------------------------------------------
    def _check(self, rc: int):
        if rc == FLEET_OK:
            return
        msg = self._L.fleet_last_error(self._h).decode(errors="replace")
        if rc == FLEET_ERR_BASE64:
            raise Base64Error(rc, msg)
        if rc == FLEET_ERR_LAYOUT:
            raise LayoutError(rc, msg)
        raise FleetError(rc, msg)

    def _text_call(self, fn, args, cap):
        out = np.empty(max(cap, 1), np.uint8)
        n = C.c_size_t(0)
        rc = fn(self._h, *args, out.ctypes.data, cap, C.byref(n))
        self._check(rc)
        return out[: n.value].tobytes()

    # -- Base64.cpp -------------------------------------------------------------
    def encode_floats(self, v) -> bytes:
        """Base64::encode(std::vector<float>) (Base64.cpp:104-106)."""
        v = np.ascontiguousarray(v, dtype=np.float32)
        return self._text_call(self._L.fleet_encode_f32, (v.ctypes.data, len(v)), b64_len(len(v)))

    def encode_ints(self, v) -> bytes:
        """Base64::encode(std::vector<int>) (Base64.cpp:109-115)."""
        v = np.ascontiguousarray(v, dtype=np.int32)
        return self._text_call(self._L.fleet_encode_i32, (v.ctypes.data, len(v)), b64_len(len(v)))

    def decode_floats(self, text) -> np.ndarray:
        """Base64::decodeFloat (Base64.cpp:171-173)."""
        s = _as_bytes(text)
        out = np.empty(b64_count(len(s)) + 1, np.float32)
        n = C.c_size_t(0)
        self._check(self._L.fleet_decode_f32(self._h, s, len(s), out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    def decode_ints(self, text) -> np.ndarray:
        """Base64::decodeInt (Base64.cpp:175-183)."""
        s = _as_bytes(text)
        out = np.empty(b64_count(len(s)) + 1, np.int32)
        n = C.c_size_t(0)
        self._check(self._L.fleet_decode_i32(self._h, s, len(s), out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    # -- cppNN_backend.cpp natives (same names as the Java declarations) -------
    def getFlatGradient(self, grad) -> bytes:  # noqa: N802  (CppNNUpdater.java:159)
        s = _as_bytes(grad)
        return self._text_call(self._L.fleet_flat_gradient, (s, len(s)), len(s) + 16)

    def mergeFlatGradient(self, grad, flat) -> bytes:  # noqa: N802  (CppNNUpdater.java:160)
        g, f = _as_bytes(grad), _as_bytes(flat)
        return self._text_call(self._L.fleet_merge_flat_gradient, (g, len(g), f, len(f)), len(g) + 16)

    def scalarMulNative(self, v, a: float) -> bytes:  # noqa: N802  (ByteVec.java:26)
        s = _as_bytes(v)
        return self._text_call(self._L.fleet_scalar_mul, (s, len(s), float(a)), len(s) + 16)

    def addNative(self, a, b) -> bytes:  # noqa: N802  (ByteVec.java:25)
        x, y = _as_bytes(a), _as_bytes(b)
        return self._text_call(self._L.fleet_add, (x, len(x), y, len(y)), len(x) + 16)

    def subtractNative(self, a, b) -> bytes:  # noqa: N802  (ByteVec.java:24)
        x, y = _as_bytes(a), _as_bytes(b)
        return self._text_call(self._L.fleet_subtract, (x, len(x), y, len(y)), len(x) + 16)

    def getNorm(self, v) -> float:  # noqa: N802  (ByteVec.java:23)
        s = _as_bytes(v)
        out = C.c_double(0)
        self._check(self._L.fleet_norm(self._h, s, len(s), C.byref(out)))
        return out.value

    def layout_parse(self, upload):
        s = _as_bytes(upload)
        pos = np.empty(FLEET_MAX_HEADERS, np.int32)
        nh = C.c_int(0)
        n_up = C.c_size_t(0)
        self._check(self._L.fleet_layout_parse(self._h, s, len(s), pos.ctypes.data, FLEET_MAX_HEADERS,
                                               C.byref(nh), C.byref(n_up)))
        return pos[: nh.value].copy(), int(n_up.value)

    # -- fused update ------------------------------------------------------------
    def update(self, uploads: Sequence, dampen: Sequence[float], want_f32: bool = False):
        """Aggregation of CppNNUpdater.update (CppNNUpdater.java:420-509) in one call.

        Returns the merged Base64 (what mergeFlatGradient returns) and, with
        ``want_f32``, Base64::decodeFloat of it (what descentNative decodes).
        """
        ups = [_as_bytes(u) for u in uploads]
        M = len(ups)
        if M == 0:
            raise ValueError("no uploads")
        if len(dampen) != M:
            raise ValueError("one dampening factor per upload")
        arr = (C.c_char_p * M)(*ups)
        lens = np.array([len(u) for u in ups], dtype=np.uint64)
        d = np.ascontiguousarray(dampen, dtype=np.float64)
        L = len(ups[0])
        out = np.empty(L + 16, np.uint8)
        n = C.c_size_t(0)
        f32 = np.empty(b64_count(L) + 1, np.float32) if want_f32 else None
        rc = self._L.fleet_update(self._h, C.cast(arr, C.c_void_p), lens.ctypes.data, M, d.ctypes.data,
                                  out.ctypes.data, len(out), C.byref(n), f32.ctypes.data if want_f32 else None)
        self._check(rc)
        merged = out[: n.value].tobytes()
        if want_f32:
            return merged, f32[: b64_count(L)].copy()
        return merged

    def accumulator(self, length: int, header_pos, group_begin: int = 0, group_end: Optional[int] = None):
        """A streaming accumulator (fleet_acc) for uploads of `length` Base64 bytes with the
        given layout header positions: each upload is folded into a resident sum when it
        arrives, and ``finish`` returns what ``update`` returns for the same uploads."""
        return Accumulator(self, length, header_pos, group_begin, group_end)

    def pool(self, length: int, header_pos, slots: int, group_begin: int = 0, group_end: Optional[int] = None):
        """An upload pool (fleet_pool) of `slots` resident uploads of `length` Base64 bytes:
        uploads are put into slots when they arrive, and ``update`` over any subset of the
        slots, in any order, returns what ``update`` returns for those uploads in that order."""
        return Pool(self, length, header_pos, slots, group_begin, group_end)

    def model_ledger(self, n_weights: int, n_biases: int, graph_edges: int, workers: int,
                     max_versions: Optional[int] = None):
        """A Kardam model ledger (fleet_mledger) for models of ``n_weights`` non-null W floats
        and ``n_biases`` use_bias() biases over ``graph_edges`` layer-graph edges: ``workers``
        worker ids, at most ``max_versions`` (default: ``workers``) resident versions that no
        worker holds."""
        return ModelLedger(self, n_weights, n_biases, graph_edges, workers, max_versions)

    def update_rows(self, rows: np.ndarray, length: int, dampen: Sequence[float], want_f32: bool = False):
        """fleet_update over a uint8 host array [M, row_pitch] whose row i holds upload i's
        `length` Base64 chars; page-locked rows (register_host) go to HBM without a host copy."""
        return update_rows([self], rows, length, dampen, want_f32)

    def register_host(self, arr: np.ndarray):
        """Page-lock a host array for copy-free ingress (fleet_host_register)."""
        self._check(self._L.fleet_host_register(self._h, arr.ctypes.data, arr.nbytes))

    def unregister_host(self, arr: np.ndarray):
        self._check(self._L.fleet_host_unregister(self._h, arr.ctypes.data))

    # -- device-resident (torch tensors on this device) -----------------------
    def update_device(self, uploads_u8, length: int, dampen: Sequence[float], header_pos, merged_u8,
                      merged_f32=None, group_begin: int = 0, group_end: Optional[int] = None, stream=None,
                      window: bool = False):
        """uploads_u8: uint8 CUDA tensor [M, pitch]; merged_u8: uint8 [>= 16*groups].

        window=False: the tensors hold whole rows (group 0 at column 0).
        window=True: they hold only the groups [group_begin, group_end) of every
        row (uploads [M, >= 16*(ge-gb)], merged [16*(ge-gb)], merged_f32
        [3*(ge-gb)]); header_pos stay in whole-upload coordinates.

        header_pos (here and in update_encode_device / update_kardam_device / accumulator):
        strictly ascending positions inside [0, b64_count(length)), at most
        FLEET_MAX_HEADERS; any other list raises FleetError (FLEET_ERR_ARG), nothing is
        launched and the context keeps the parameters of its last accepted call."""
        M, pitch = uploads_u8.shape
        groups = (b64_count(length) + 2) // 3
        ge = groups if group_end is None else min(group_end, groups)
        hp = np.ascontiguousarray(header_pos, dtype=np.int32)
        d = np.ascontiguousarray(dampen, dtype=np.float64)
        shift_b = 16 * group_begin if window else 0
        shift_f = 3 * 4 * group_begin if window else 0
        if window:
            w = ge - group_begin
            if pitch < 16 * w or merged_u8.numel() < 16 * w or (merged_f32 is not None and merged_f32.numel() < 3 * w):
                raise ValueError("window tensors smaller than the selected groups")
        rc = self._L.fleet_update_device(self._h, uploads_u8.data_ptr() - shift_b, pitch, length, M, d.ctypes.data,
                                         hp.ctypes.data, len(hp), group_begin, ge, merged_u8.data_ptr() - shift_b,
                                         merged_f32.data_ptr() - shift_f if merged_f32 is not None else None,
                                         _stream(stream))
        self._check(rc)

    def update_encode_device(self, uploads_u8, length: int, dampen: Sequence[float], header_pos, merged_u8,
                             merged_f32, values_f32, next_uploads_u8, stream=None):
        """One pipelined step (fleet_update_encode_device): update_device over the whole
        uploads_u8 [M, pitch] and encode_device of values_f32 [M, vpitch] into
        next_uploads_u8 [M, pitch] (a different buffer), in one launch."""
        M, pitch = uploads_u8.shape
        if tuple(next_uploads_u8.shape) != (M, pitch) or values_f32.shape[0] != M:
            raise ValueError("next_uploads / values must have the uploads' rows and pitch")
        hp = np.ascontiguousarray(header_pos, dtype=np.int32)
        d = np.ascontiguousarray(dampen, dtype=np.float64)
        rc = self._L.fleet_update_encode_device(self._h, uploads_u8.data_ptr(), pitch, length, M, d.ctypes.data,
                                                hp.ctypes.data, len(hp), merged_u8.data_ptr(),
                                                merged_f32.data_ptr() if merged_f32 is not None else None,
                                                values_f32.data_ptr(), values_f32.shape[1],
                                                next_uploads_u8.data_ptr(), _stream(stream))
        self._check(rc)

    def update_kardam_device(self, uploads_u8, length: int, dampen: Sequence[float], header_pos, lr: float,
                             merged_u8, merged_f32=None, prev_f32=None, has_prev=None, g_out_f32=None, stream=None):
        """update_device plus Kardam's per-client norms in the same pass (fleet_update_kardam_device):
        returns (norm_g[M], norm_diff[M]); prev_f32 / g_out_f32: float32 CUDA tensors [M, vpitch]
        of decoded Kardam gradients in upload coordinates (g_out_f32 may be prev_f32 itself:
        this round's G then replaces prev in place)."""
        M, pitch = uploads_u8.shape
        hp = np.ascontiguousarray(header_pos, dtype=np.int32)
        d = np.ascontiguousarray(dampen, dtype=np.float64)
        vpitch = (prev_f32 if prev_f32 is not None else g_out_f32).shape[1] if (
            prev_f32 is not None or g_out_f32 is not None) else 0
        hv = None
        if prev_f32 is not None:
            hv = np.ascontiguousarray(has_prev if has_prev is not None else np.ones(M), dtype=np.uint8)
        ng, nd = np.empty(M, np.float64), np.empty(M, np.float64)
        rc = self._L.fleet_update_kardam_device(
            self._h, uploads_u8.data_ptr(), pitch, length, M, d.ctypes.data, hp.ctypes.data, len(hp), float(lr),
            prev_f32.data_ptr() if prev_f32 is not None else None, hv.ctypes.data if hv is not None else None,
            g_out_f32.data_ptr() if g_out_f32 is not None else None, vpitch, merged_u8.data_ptr(),
            merged_f32.data_ptr() if merged_f32 is not None else None, ng.ctypes.data, nd.ctypes.data,
            _stream(stream))
        self._check(rc)
        return ng, nd

    def test_kardam_skew(self, skew: int) -> None:
        """Test hook: the pipelined Kardam form's reduce blocks wait for a later epoch than
        the tiles publish (skew != 0), so the call fails on their bounded wait."""
        self._check(self._L.fleet_test_kardam_skew(self._h, int(skew)))

    def encode_device(self, values_f32, n: int, out_u8, stream=None):
        """values_f32: float32 CUDA tensor [M, vpitch]; out_u8: uint8 [M, pitch]."""
        M, vpitch = values_f32.shape
        _, pitch = out_u8.shape
        rc = self._L.fleet_encode_device(self._h, values_f32.data_ptr(), n, vpitch, M, out_u8.data_ptr(), pitch,
                                         _stream(stream))
        self._check(rc)

    def decode_device(self, text_u8, length: int, out_f32, stream=None):
        M, pitch = text_u8.shape
        _, vpitch = out_f32.shape
        rc = self._L.fleet_decode_device(self._h, text_u8.data_ptr(), length, pitch, M, out_f32.data_ptr(), vpitch,
                                         _stream(stream))
        self._check(rc)

    def synth_device(self, seed: int, values_f32, n_up: int, header_pos, header_val, client0: int = 0,
                     stream=None, elem0: int = 0):
        """Synthetic buckets (fleet_synth_window_device): rows client0.. of a problem whose
        elements elem0 .. elem0 + n_up this tensor holds; header_pos in its coordinates,
        each inside [0, n_up) (else FleetError, FLEET_ERR_ARG, before anything is launched)."""
        M, vpitch = values_f32.shape
        hp = np.ascontiguousarray(header_pos, dtype=np.int32)
        hv = np.ascontiguousarray(header_val, dtype=np.float32)
        rc = self._L.fleet_synth_window_device(self._h, seed, M, client0, elem0, hp.ctypes.data, hv.ctypes.data,
                                               len(hp), n_up, values_f32.data_ptr(), vpitch, _stream(stream))
        self._check(rc)

    def selftest_digest(self, fn: int) -> int:
        """Digest of the device codec arithmetic over a whole input domain (fleet_codec.h)."""
        out = C.c_uint64(0)
        self._check(self._L.fleet_selftest_digest(self._h, fn, C.byref(out)))
        return out.value

    def check(self, stream=None):
        self._check(self._L.fleet_check(self._h, _stream(stream)))

    def sync(self, stream=None):
        self._check(self._L.fleet_sync(self._h, _stream(stream)))

    # -- DISTILLATION_MODE=1 model codec ----------------
    @staticmethod
    def _model_args(weights, dims):
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        d = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1)
        if len(d) % 3:
            raise ValueError("dims: (cols, rows, chans) per matrix")
        n = int(sum(int(d[k]) * int(d[k + 1]) * int(d[k + 2]) for k in range(0, len(d), 3)))
        if len(w) != n:
            raise ValueError(f"{len(w)} weights for a model of {n}")
        return w, d, n

    def model_quantize_index(self, weights, dims):
        """quantization_weight_model + getParams' dictionary and selected-index set
        (network.h:594-692, 1683-1774): (quantised weights, dictionary, indices)."""
        w, d, n = self._model_args(weights, dims)
        wq = np.empty(n, np.float32)
        dic = np.empty(max(1, n), np.float32)
        idx = np.empty(n, np.int32)
        U = C.c_int(0)
        self._check(self._L.fleet_model_quantize_index(self._h, w.ctypes.data, d.ctypes.data, len(d) // 3,
                                                       wq.ctypes.data, dic.ctypes.data, C.byref(U), idx.ctypes.data))
        return wq, dic[: U.value].copy(), idx

    def model_weights_text(self, weights, dims) -> bytes:
        """getParams' DISTILLATION_MODE=1 weights section for these (unquantised) weights."""
        w, d, n = self._model_args(weights, dims)
        need = C.c_size_t(0)
        rc = self._L.fleet_model_weights_text(self._h, w.ctypes.data, d.ctypes.data, len(d) // 3, None, 0,
                                              C.byref(need))
        if rc not in (0, FLEET_ERR_CAPACITY):
            self._check(rc)
        buf = np.empty(max(1, need.value), np.uint8)
        self._check(self._L.fleet_model_weights_text(self._h, w.ctypes.data, d.ctypes.data, len(d) // 3,
                                                     buf.ctypes.data, need.value, C.byref(need)))
        return buf[: need.value].tobytes()

    def values_text(self, values, block_sizes=None, stream=None) -> bytes:
        """The text of `ostream << float` ('%g') for these values, formatted on the device
        (fleet_values_text). block_sizes: "value " per value and a newline after each block
        (getParams' bias and mode-0 weight lines; an empty block prints its lone newline);
        None: the "i\\nvalue\\n" pairs of the mode-1 dictionary section. `values` is a
        numpy array, or a float32 device tensor that is read where it is."""
        bs = None if block_sizes is None else np.ascontiguousarray(block_sizes, dtype=np.int64).reshape(-1)
        if bs is not None and len(bs) == 0:
            raise ValueError("block_sizes: at least one block (None selects the pairs form)")
        nb, bp = (0, None) if bs is None else (len(bs), bs.ctypes.data)
        if hasattr(values, "data_ptr"):
            import torch
            if values.dtype != torch.float32 or not values.is_cuda or not values.is_contiguous():
                raise ValueError("values: a contiguous float32 device tensor")
            n = values.numel()

            def call(buf, cap, need):
                return self._L.fleet_values_text_device(self._h, values.data_ptr(), n, bp, nb, buf, cap, C.byref(need),
                                                        _stream(stream))
        else:
            v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
            n = len(v)

            def call(buf, cap, need):
                return self._L.fleet_values_text(self._h, v.ctypes.data, n, bp, nb, buf, cap, C.byref(need))
        need = C.c_size_t(0)
        cap = 14 * n + nb + 16 if bs is not None else 26 * n + 16  # 12 bytes + separators (+ an int key)
        buf = np.empty(cap, np.uint8)
        self._check(call(buf.ctypes.data, cap, need))
        return buf[: need.value].tobytes()

    def model_read_weights(self, text, dims) -> np.ndarray:
        """network::read's DISTILLATION_MODE=1 branch: weights section -> weights."""
        t = _as_bytes(text)
        d = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1)
        n = int(sum(int(d[k]) * int(d[k + 1]) * int(d[k + 2]) for k in range(0, len(d), 3)))
        out = np.empty(n, np.float32)
        self._check(self._L.fleet_model_read_weights(self._h, t, len(t), d.ctypes.data, len(d) // 3,
                                                     out.ctypes.data))
        return out

    def model_version(self, weights, dims, biases):
        """descentNative's mode-1 model copy: read(getParams()) of the unquantised model
        (weights via the first-occurrence dictionary, %g/strtof round trips)."""
        w, d, n = self._model_args(weights, dims)
        b = np.ascontiguousarray(biases, dtype=np.float32).reshape(-1)
        wo = np.empty(n, np.float32)
        bo = np.empty(len(b), np.float32)
        self._check(self._L.fleet_model_version(self._h, w.ctypes.data, d.ctypes.data, len(d) // 3, b.ctypes.data,
                                                len(b), wo.ctypes.data, bo.ctypes.data))
        return wo, bo

    def getModelParametersNative(self, weights, biases, graph_edges: int) -> bytes:  # noqa: N802  (java:148)
        """Base64 of network::getModelParams (cppNN_backend.cpp:227-242): the use_bias() biases repeated
        graph_edges (= layer_graph.size()) times, then the non-null W."""
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        b = np.ascontiguousarray(biases, dtype=np.float32).reshape(-1)
        n = len(b) * int(graph_edges) + len(w)
        return self._text_call(self._L.fleet_model_params, (w.ctypes.data, len(w), b.ctypes.data, len(b),
                                                            int(graph_edges)), b64_len(n))

    # -- Kardam bookkeeping ------------------------------------
    def kardam_grads(self, uploads: Sequence, dampen: Sequence[float], lr: float, prev=None):
        """For the M picked uploads (CppNNUpdater.java:463-481): the texts
        g_c = getFlatGradient(u_c).scalarMultiply(d_c).scalarMultiply(lr), their norms and,
        where prev[c] is given, the norms of g_c.subtract(prev[c]) (else NaN)."""
        ups = [_as_bytes(u) for u in uploads]
        M = len(ups)
        if M == 0 or len(dampen) != M:
            raise ValueError("one dampening factor per upload")
        arr = (C.c_char_p * M)(*ups)
        lens = np.array([len(u) for u in ups], dtype=np.uint64)
        d = np.ascontiguousarray(dampen, dtype=np.float64)
        pv = None
        if prev is not None:
            if len(prev) != M:
                raise ValueError("one previous gradient (or None) per upload")
            pv = (C.c_char_p * M)(*[(_as_bytes(x) if x is not None else None) for x in prev])
        pitch = len(ups[0]) + 16
        g = np.empty((M, pitch), np.uint8)
        glen = C.c_size_t(0)
        ng = np.empty(M, np.float64)
        nd = np.empty(M, np.float64)
        self._check(self._L.fleet_kardam_grads(self._h, C.cast(arr, C.c_void_p), lens.ctypes.data, M, d.ctypes.data,
                                               float(lr), C.cast(pv, C.c_void_p) if pv is not None else None,
                                               g.ctypes.data, pitch, C.byref(glen), ng.ctypes.data, nd.ctypes.data))
        return [g[c, : glen.value].tobytes() for c in range(M)], ng, nd

    # -- getMiniBatch -------------------------------------------
    def getMiniBatch(self, images, labels, idx, header, teacher=None) -> bytes:  # noqa: N802  (cppNN_backend.cpp:677)
        """Base64 of the sampler's mini-batch vector (cppNN_backend.cpp:553-699) for the
        sample indices `idx`: header (7 floats, fleet_amd.sampler.minibatch_header),
        per sample its features, (mode 1) the teacher's probabilities, its label."""
        x = np.ascontiguousarray(images, dtype=np.float32)
        n_img, F = x.shape
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        ix = np.ascontiguousarray(idx, dtype=np.int32)
        h = np.ascontiguousarray(header, dtype=np.float32)
        if len(h) != 7:
            raise ValueError("header holds E, sigma, C, lr, batchSize, featureSize, numLabels")
        t, nl = None, 0
        if teacher is not None:
            t = np.ascontiguousarray(teacher, dtype=np.float32)
            nl = t.shape[1]
            if t.shape[0] != len(ix):
                raise ValueError("one teacher row per sample")
        cap = self._L.fleet_minibatch_len(F, len(ix), nl, t is not None)
        return self._text_call(self._L.fleet_minibatch, (x.ctypes.data, n_img, F, lab.ctypes.data, ix.ctypes.data,
                                                         len(ix), t.ctypes.data if t is not None else None, nl,
                                                         h.ctypes.data), cap)

    def minibatch_device(self, images_f32, labels_i32, idx_i32, header, out_u8, teacher_f32=None, stream=None):
        """Device-resident getMiniBatch: CUDA tensors images [N, F], labels [N], idx [B],
        out uint8 [>= fleet_minibatch_len]. Index errors surface at check()."""
        n_img, F = images_f32.shape
        h = np.ascontiguousarray(header, dtype=np.float32)
        nl = teacher_f32.shape[1] if teacher_f32 is not None else 0
        self._check(self._L.fleet_minibatch_device(self._h, images_f32.data_ptr(), n_img, F, labels_i32.data_ptr(),
                                                   idx_i32.data_ptr(), idx_i32.numel(),
                                                   teacher_f32.data_ptr() if teacher_f32 is not None else None, nl,
                                                   h.ctypes.data, out_u8.data_ptr(), _stream(stream)))

    # -- the sampler's mode-1 teacher forward ----------------
    def teacher_forward(self, w, b, images, idx=None, temperature: float = 2.0) -> np.ndarray:
        """uniformSample's teacher.forward(sample, TEMPERATURE, -1, 1) (cppNN_backend.cpp:603)
        for images[idx] (all rows when idx is None): [B, 10] class probabilities of
        initSampler's teacher network with weights w (non-null W in network order) and
        biases b (use_bias() layers in layer order)."""
        wv = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
        bv = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        x = np.ascontiguousarray(images, dtype=np.float32)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        n_img, F = x.shape
        ix = np.arange(n_img, dtype=np.int32) if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        out = np.empty((len(ix), 10), np.float32)
        self._check(self._L.fleet_teacher_forward(self._h, wv.ctypes.data, len(wv), bv.ctypes.data, len(bv),
                                                  x.ctypes.data, n_img, F, ix.ctypes.data, len(ix),
                                                  float(temperature), out.ctypes.data))
        return out

    def teacher_forward_device(self, w_f32, b_f32, images_f32, probs_f32, idx_i32=None, temperature: float = 2.0,
                               stream=None):
        """Device-resident teacher forward: CUDA tensors w [21448], b [82], images [N, F >= 784],
        probs [B, 10] written for images[idx] (B = N rows when idx is None). Index errors at check()."""
        n_img, F = images_f32.shape
        if w_f32.numel() != self._L.fleet_teacher_weight_count() or b_f32.numel() != self._L.fleet_teacher_bias_count():
            raise ValueError("teacher weights / biases of the wrong size")
        B = idx_i32.numel() if idx_i32 is not None else n_img
        if probs_f32.numel() < 10 * B:
            raise ValueError("probs holds B x 10 floats")
        self._check(self._L.fleet_teacher_forward_device(self._h, w_f32.data_ptr(), b_f32.data_ptr(),
                                                         images_f32.data_ptr(), n_img, F,
                                                         idx_i32.data_ptr() if idx_i32 is not None else None, B,
                                                         float(temperature), probs_f32.data_ptr(), _stream(stream)))

    # -- the Driver's evaluation ---------------------------------
    def evaluate(self, w, b, images, labels, idx=None) -> "Evaluation":
        """The Driver's ``test()`` (Driver/src/main/c++/cppNN_backend.cpp:53-75) of the MNIST
        network with weights ``w`` and biases ``b`` (``teacher_forward``'s layout) over
        ``images[idx]`` (every image in order when ``idx`` is None): bit for bit the
        reference's error, accuracy, predictions and their probabilities."""
        wv = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
        bv = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        rc, ev = _eval_host_call(self._L.fleet_evaluate, (self._h, wv.ctypes.data, len(wv), bv.ctypes.data, len(bv)),
                                 images, labels, idx)
        self._check(rc)
        return ev

    def evaluate_device(self, w_f32, b_f32, images_f32, labels_i32, idx_i32=None, out=None, stream=None) -> dict:
        """Device-resident :meth:`evaluate`: CUDA tensors w [21448], b [82], images [N, F >= 784]
        float32, labels [N] int32, idx int32 or None. Runs on ``stream`` (default: torch's
        current) and does not synchronise. ``out`` may hold tensors to write -- ``predictions``
        [B] int32, ``probabilities`` [B], ``result`` [3] (float error, float accuracy, the bits of
        int32 correct), and optionally ``costs`` [B], ``probs10`` [B, 10]; ``predictions`` or
        ``probabilities`` given as None are not written. Returns the dict of tensors written
        (:func:`evaluation_from_device` reads it). Index errors at check()."""
        if w_f32.numel() != self._L.fleet_teacher_weight_count() or b_f32.numel() != self._L.fleet_teacher_bias_count():
            raise ValueError("weights / biases of the wrong size")
        n_img, F, B, o = _eval_device_out(images_f32, labels_i32, idx_i32, out)
        self._check(self._L.fleet_evaluate_device(self._h, w_f32.data_ptr(), b_f32.data_ptr(), images_f32.data_ptr(),
                                                  n_img, F, labels_i32.data_ptr(), _ptr(idx_i32), B,
                                                  _ptr(o.get("predictions")), _ptr(o.get("probabilities")),
                                                  _ptr(o.get("costs")), _ptr(o.get("probs10")), o["result"].data_ptr(),
                                                  _stream(stream)))
        return o

    # -- descentNative's model step ----------------------------
    @staticmethod
    def _layout_args(layout):
        ws = np.ascontiguousarray(layout.w_sizes, dtype=np.int32)
        wp = np.ascontiguousarray(layout.w_present(), dtype=np.uint8)
        bs = np.ascontiguousarray(layout.b_sizes, dtype=np.int32)
        fc = np.ascontiguousarray(layout.fc_flags(), dtype=np.uint8)
        return ws, wp, bs, fc

    def descent(self, weights, fc_bias, grad, layout, lr: float):
        """network::descent(vector) with the sgd solver (cppNN_backend.cpp:336-352): returns the
        updated (weights, fc_bias); `grad` = decodeFloat(merged) in the layout's gradients() order."""
        w = np.array(weights, dtype=np.float32, copy=True).reshape(-1)
        b = np.array(fc_bias, dtype=np.float32, copy=True).reshape(-1)
        g = np.ascontiguousarray(grad, dtype=np.float32).reshape(-1)
        ws, wp, bs, fc = self._layout_args(layout)
        self._check(self._L.fleet_descent(self._h, w.ctypes.data, len(w), b.ctypes.data, len(b), g.ctypes.data,
                                          len(g), ws.ctypes.data, wp.ctypes.data, len(ws), bs.ctypes.data,
                                          fc.ctypes.data, len(bs), float(lr)))
        return w, b

    def descent_window_device(self, weights_f32, fc_bias_f32, grad_window_f32, value_begin: int, value_end: int,
                              layout, lr: float, stream=None):
        """The model step of one element shard: grad_window_f32 holds the merged fp32 values
        [value_begin, value_end); only the parameters those positions cover are updated."""
        ws, wp, bs, fc = self._layout_args(layout)
        self._check(self._L.fleet_descent_window_device(self._h, weights_f32.data_ptr(),
                                                        fc_bias_f32.data_ptr() if fc_bias_f32 is not None else None,
                                                        grad_window_f32.data_ptr(), int(value_begin), int(value_end),
                                                        ws.ctypes.data, wp.ctypes.data, len(ws), bs.ctypes.data,
                                                        fc.ctypes.data, len(bs), float(lr), _stream(stream)))

    def descent_device(self, weights_f32, fc_bias_f32, grad_f32, layout, lr: float, stream=None):
        """Device-resident model step: float32 CUDA tensors updated in place."""
        ws, wp, bs, fc = self._layout_args(layout)
        self._check(self._L.fleet_descent_device(self._h, weights_f32.data_ptr(),
                                                 fc_bias_f32.data_ptr() if fc_bias_f32 is not None else None,
                                                 grad_f32.data_ptr(), ws.ctypes.data, wp.ctypes.data, len(ws),
                                                 bs.ctypes.data, fc.ctypes.data, len(bs), float(lr),
                                                 _stream(stream)))


    @staticmethod
    def _solver_number(solver) -> int:
        if isinstance(solver, str):
            n = lib().fleet_solver_from_name(solver.encode())
            if n < 0:
                raise ValueError(f"no solver {solver!r}: one of {', '.join(SOLVERS)}")
            return n
        return int(solver)

    def descent_solver(self, solver, weights, g1, g2, fc_bias, grad, layout, lr: float):
        """:meth:`descent` under ``solver`` ("sgd", "adagrad", "rmsprop", "adam" or its
        FLEET_SOLVER_* number; commonLib/cppNN/solver.h:97-195): returns the updated
        (weights, g1, g2, fc_bias). ``g1`` / ``g2``: the solver's state, one float per weight
        (``g2``: adam only, None otherwise and returned as None; both None for sgd)."""
        sv = self._solver_number(solver)
        w = np.array(weights, dtype=np.float32, copy=True).reshape(-1)
        s1 = None if g1 is None else np.array(g1, dtype=np.float32, copy=True).reshape(-1)
        s2 = None if g2 is None else np.array(g2, dtype=np.float32, copy=True).reshape(-1)
        if any(s is not None and len(s) != len(w) for s in (s1, s2)):
            raise ValueError("a state row holds one float per weight")
        b = np.array(fc_bias, dtype=np.float32, copy=True).reshape(-1)
        g = np.ascontiguousarray(grad, dtype=np.float32).reshape(-1)
        ws, wp, bs, fc = self._layout_args(layout)
        self._check(self._L.fleet_descent_solver(self._h, sv, w.ctypes.data, len(w),
                                                 None if s1 is None else s1.ctypes.data,
                                                 None if s2 is None else s2.ctypes.data, b.ctypes.data, len(b),
                                                 g.ctypes.data, len(g), ws.ctypes.data, wp.ctypes.data, len(ws),
                                                 bs.ctypes.data, fc.ctypes.data, len(bs), float(lr)))
        return w, s1, s2, b

    def descent_solver_device(self, solver, weights_f32, g1_f32, g2_f32, fc_bias_f32, grad_f32, layout, lr: float,
                              stream=None):
        """:meth:`descent_device` under ``solver``: weights and state rows (float32 CUDA
        tensors of one size) updated in place."""
        sv = self._solver_number(solver)
        for t in (g1_f32, g2_f32):
            if t is not None and t.numel() != weights_f32.numel():
                raise ValueError("a state row holds one float per weight")
        ws, wp, bs, fc = self._layout_args(layout)
        self._check(self._L.fleet_descent_solver_device(self._h, sv, weights_f32.data_ptr(),
                                                        g1_f32.data_ptr() if g1_f32 is not None else None,
                                                        g2_f32.data_ptr() if g2_f32 is not None else None,
                                                        fc_bias_f32.data_ptr() if fc_bias_f32 is not None else None,
                                                        grad_f32.data_ptr(), ws.ctypes.data, wp.ctypes.data, len(ws),
                                                        bs.ctypes.data, fc.ctypes.data, len(bs), float(lr),
                                                        _stream(stream)))


class Accumulator:
    """Streaming aggregation on one context (fleet_acc, include/fleet_codec.h): the
    reference's `acc` of buffered uploads (CppNNUpdater.java:383-391) kept as the running
    sum of the chain instead of the uploads themselves. ``push`` is synchronous and
    transactional (a rejected upload raises and leaves the batch as it was);
    ``push_device`` is asynchronous and commits at once, a bad upload surfacing as a
    sticky error at ``finish*`` or a later push until ``reset``. Uploads that are at
    hand together go in as a burst (``push_many`` / ``push_many_device``: one kernel per
    ``ACC_BURST`` of them, the same bytes as pushing each), and ``push_finish`` /
    ``push_finish_device`` fold the burst that completes a batch and finish in one call."""

    def __init__(self, codec: Codec, length: int, header_pos, group_begin: int = 0, group_end: Optional[int] = None):
        self.codec = codec
        self._L = codec._L
        self.length = int(length)
        self.groups = (b64_count(self.length) + 2) // 3
        self.group_begin = int(group_begin)
        self.group_end = self.groups if group_end is None else min(int(group_end), self.groups)
        hp = np.ascontiguousarray(header_pos, dtype=np.int32)
        h = C.c_void_p()
        self._h = None
        codec._check(self._L.fleet_acc_create(codec._h, self.length, hp.ctypes.data, len(hp), self.group_begin,
                                              self.group_end, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and getattr(self.codec, "_h", None):
            self._L.fleet_acc_destroy(self._h)
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

    @property
    def count(self) -> int:
        return self._L.fleet_acc_count(self._h)

    def push(self, upload, dampen: float) -> None:
        s = _as_bytes(upload)
        self.codec._check(self._L.fleet_acc_push(self._h, s, len(s), float(dampen)))

    def push_device(self, u8_tensor, dampen: float, stream=None) -> None:
        """u8_tensor: a uint8 CUDA tensor holding the whole upload row (>= length bytes)."""
        if u8_tensor.numel() < self.length:
            raise ValueError("the tensor is shorter than the accumulator's uploads")
        self.codec._check(self._L.fleet_acc_push_device(self._h, u8_tensor.data_ptr(), float(dampen), _stream(stream)))

    def finish(self, want_f32: bool = False):
        """The merged Base64 of the uploads pushed since the last finish (and, with
        ``want_f32``, decodeFloat of it); the accumulator is then empty. With a group
        window only the window's bytes / values of the returned buffers are written."""
        out = np.zeros(self.length + 16, np.uint8)
        n = C.c_size_t(0)
        f32 = np.zeros(b64_count(self.length) + 1, np.float32) if want_f32 else None
        self.codec._check(self._L.fleet_acc_finish(self._h, out.ctypes.data, len(out), C.byref(n),
                                                   f32.ctypes.data if want_f32 else None))
        merged = out[: n.value].tobytes()
        if want_f32:
            return merged, f32[: b64_count(self.length)].copy()
        return merged

    def finish_device(self, merged_u8, merged_f32=None, stream=None) -> None:
        """merged_u8: uint8 CUDA tensor [>= 16 * groups], merged_f32: float32 [>= n values]
        (whole-upload coordinates); synchronises the stream to report a bad device push."""
        if merged_u8.numel() < 16 * self.groups or (
                merged_f32 is not None and merged_f32.numel() < b64_count(self.length)):
            raise ValueError("merged tensors smaller than the upload's groups")
        self.codec._check(self._L.fleet_acc_finish_device(self._h, merged_u8.data_ptr(),
                                                          merged_f32.data_ptr() if merged_f32 is not None else None,
                                                          _stream(stream)))

    def reset(self) -> None:
        self.codec._check(self._L.fleet_acc_reset(self._h))

    # bursts: K uploads folded by one kernel per ACC_BURST of them

    @staticmethod
    def _burst_args(uploads, dampens):
        ups = [_as_bytes(u) for u in uploads]
        if not ups:
            raise ValueError("no uploads")
        if len(dampens) != len(ups):
            raise ValueError("one dampening factor per upload")
        arr = (C.c_char_p * len(ups))(*ups)
        lens = np.array([len(u) for u in ups], dtype=np.uint64)
        d = np.ascontiguousarray(dampens, dtype=np.float64)
        return ups, arr, lens, d

    def _device_rows(self, u8_tensor, dampens):
        if u8_tensor.dim() != 2 or u8_tensor.stride(1) != 1:
            raise ValueError("expected a uint8 CUDA tensor [K, pitch] with contiguous rows")
        K = int(u8_tensor.shape[0])
        if K == 0:
            raise ValueError("no uploads")
        if len(dampens) != K:
            raise ValueError("one dampening factor per upload")
        if u8_tensor.shape[1] < (self.length if K == 1 else 16 * self.groups):
            raise ValueError("the rows are shorter than the accumulator's uploads")
        return K, int(u8_tensor.stride(0)) if K > 1 else 0, np.ascontiguousarray(dampens, dtype=np.float64)

    def push_many(self, uploads, dampens) -> None:
        """Folds the uploads in order, as ``push`` on each would, in one synchronous call;
        all or nothing: if one is rejected the call raises and the batch is as before."""
        ups, arr, lens, d = self._burst_args(uploads, dampens)
        self.codec._check(self._L.fleet_acc_push_many(self._h, arr, lens.ctypes.data, len(ups), d.ctypes.data))

    def push_many_device(self, u8_tensor, dampens, stream=None) -> None:
        """u8_tensor: a uint8 CUDA tensor [K, pitch] of whole upload rows (pitch a multiple of
        16, >= 16 * groups); asynchronous, errors are sticky as with ``push_device``."""
        K, pitch, d = self._device_rows(u8_tensor, dampens)
        self.codec._check(self._L.fleet_acc_push_many_device(self._h, u8_tensor.data_ptr(), pitch, K, d.ctypes.data,
                                                             _stream(stream)))

    def push_finish(self, uploads, dampens, want_f32: bool = False):
        """``push_many`` and ``finish`` in one call: the kernel that folds the last uploads
        also writes the merged gradient. Transactional like ``push_many``."""
        ups, arr, lens, d = self._burst_args(uploads, dampens)
        out = np.zeros(self.length + 16, np.uint8)
        n = C.c_size_t(0)
        f32 = np.zeros(b64_count(self.length) + 1, np.float32) if want_f32 else None
        self.codec._check(self._L.fleet_acc_push_finish(self._h, arr, lens.ctypes.data, len(ups), d.ctypes.data,
                                                        out.ctypes.data, len(out), C.byref(n),
                                                        f32.ctypes.data if want_f32 else None))
        merged = out[: n.value].tobytes()
        if want_f32:
            return merged, f32[: b64_count(self.length)].copy()
        return merged

    def push_finish_device(self, u8_tensor, dampens, merged_u8, merged_f32=None, stream=None) -> None:
        """``push_many_device`` and ``finish_device`` in one call; synchronises the stream,
        and a bad row of the burst leaves the accumulator as before the call."""
        K, pitch, d = self._device_rows(u8_tensor, dampens)
        if merged_u8.numel() < 16 * self.groups or (
                merged_f32 is not None and merged_f32.numel() < b64_count(self.length)):
            raise ValueError("merged tensors smaller than the upload's groups")
        self.codec._check(self._L.fleet_acc_push_finish_device(
            self._h, u8_tensor.data_ptr(), pitch, K, d.ctypes.data, merged_u8.data_ptr(),
            merged_f32.data_ptr() if merged_f32 is not None else None, _stream(stream)))


class Pool:
    """Buffered uploads kept in HBM (fleet_pool, include/fleet_codec.h): the reference's
    `acc` in the staleSize > 0 branch (CppNNUpdater.java:383-411), where
    StalenessSimulator.stalenessSim picks, at update time, which buffered uploads to
    aggregate and in which order. ``put`` / ``put_device`` store an arrival in a slot,
    ``update`` / ``update_device`` aggregate any subset of occupied slots in the given
    order and change no slot, ``drop`` frees one. When an update raises ``Base64Error`` or
    ``LayoutError`` the pool is as before, and the exception's ``slots`` lists the picked
    slots whose uploads were at fault (``slot_status``)."""

    def __init__(self, codec: Codec, length: int, header_pos, slots: int, group_begin: int = 0,
                 group_end: Optional[int] = None):
        self.codec = codec
        self._L = codec._L
        self.length = int(length)
        self.groups = (b64_count(self.length) + 2) // 3
        self.group_begin = int(group_begin)
        self.group_end = self.groups if group_end is None else min(int(group_end), self.groups)
        hp = np.ascontiguousarray(header_pos, dtype=np.int32)
        h = C.c_void_p()
        self._h = None
        codec._check(self._L.fleet_pool_create(codec._h, self.length, hp.ctypes.data, len(hp), self.group_begin,
                                               self.group_end, int(slots), C.byref(h)))
        self._h = h
        self.slots = int(self._L.fleet_pool_slots(h))

    def close(self):
        if getattr(self, "_h", None) and getattr(self.codec, "_h", None):
            self._L.fleet_pool_destroy(self._h)
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

    def _check(self, rc: int, picks=()):
        try:
            self.codec._check(rc)
        except (Base64Error, LayoutError) as e:
            e.slots = [int(s) for s in picks if self.slot_status(int(s)) > 0]
            raise

    def _slot_query(self, fn, slot: int) -> int:
        v = fn(self._h, int(slot))
        if v < 0:
            raise FleetError(v, f"slot {slot} outside [0, {self.slots})")
        return v

    def occupied(self, slot: int) -> bool:
        return bool(self._slot_query(self._L.fleet_pool_occupied, slot))

    def free_slot(self) -> Optional[int]:
        """The lowest free slot, or None when the pool is full."""
        for s in range(self.slots):
            if not self._L.fleet_pool_occupied(self._h, s):
                return s
        return None

    def slot_status(self, slot: int) -> int:
        """Error bits the last update saw in the slot's upload (1 Base64, 2 layout header)."""
        return self._slot_query(self._L.fleet_pool_slot_status, slot)

    def put(self, slot: int, upload) -> None:
        s = _as_bytes(upload)
        self._check(self._L.fleet_pool_put(self._h, int(slot), s, len(s)))

    def put_device(self, slot: int, u8_tensor, stream=None) -> None:
        """u8_tensor: a uint8 CUDA tensor holding the whole upload row (>= length bytes)."""
        if u8_tensor.numel() < self.length:
            raise ValueError("the tensor is shorter than the pool's uploads")
        self._check(self._L.fleet_pool_put_device(self._h, int(slot), u8_tensor.data_ptr(), _stream(stream)))

    def drop(self, slot: int) -> None:
        self._check(self._L.fleet_pool_drop(self._h, int(slot)))

    @staticmethod
    def _pick_args(picks, dampens):
        pk = np.ascontiguousarray(picks, dtype=np.int32)
        if len(dampens) != len(pk):
            raise ValueError("one dampening factor per pick")
        return pk, np.ascontiguousarray(dampens, dtype=np.float64)

    def update(self, picks, dampens, want_f32: bool = False):
        """The merged Base64 of the uploads in the slots ``picks``, in that order (and, with
        ``want_f32``, decodeFloat of it). With a group window only the window's bytes /
        values of the returned buffers are written."""
        pk, d = self._pick_args(picks, dampens)
        out = np.zeros(self.length + 16, np.uint8)
        n = C.c_size_t(0)
        f32 = np.zeros(b64_count(self.length) + 1, np.float32) if want_f32 else None
        self._check(self._L.fleet_pool_update(self._h, pk.ctypes.data, len(pk), d.ctypes.data, out.ctypes.data, len(out),
                                              C.byref(n), f32.ctypes.data if want_f32 else None), pk)
        merged = out[: n.value].tobytes()
        if want_f32:
            return merged, f32[: b64_count(self.length)].copy()
        return merged

    def update_device(self, picks, dampens, merged_u8, merged_f32=None, stream=None) -> None:
        """merged_u8: uint8 CUDA tensor [>= 16 * groups], merged_f32: float32 [>= n values]
        (whole-upload coordinates); synchronises the stream to read the slots' status."""
        pk, d = self._pick_args(picks, dampens)
        if merged_u8.numel() < 16 * self.groups or (
                merged_f32 is not None and merged_f32.numel() < b64_count(self.length)):
            raise ValueError("merged tensors smaller than the upload's groups")
        self._check(self._L.fleet_pool_update_device(self._h, pk.ctypes.data, len(pk), d.ctypes.data,
                                                     merged_u8.data_ptr(),
                                                     merged_f32.data_ptr() if merged_f32 is not None else None,
                                                     _stream(stream)), pk)

    def ledger(self, workers: int, max_store: Optional[int] = None) -> "Ledger":
        """A Kardam ledger (fleet_kledger) over this pool: ``workers`` worker ids, at most
        ``max_store`` (default: the pool's slots) picks of one update that store a row."""
        return Ledger(self, workers, self.slots if max_store is None else max_store)

    def gate(self, header_values=None) -> "Gate":
        """An arrival gate (fleet_gate) beside this pool. ``header_values``: the value every
        header slot of a good upload decodes to, in position order (``Layout.header_values()``);
        None: the header slots are not checked."""
        return Gate(self, header_values)


def header_codes(values) -> np.ndarray:
    """``float2int`` of each value (fleet_gate_header_codes; Base64.cpp:60-73): the codes a
    client's ``Base64::encode(cnn.gradients())`` puts in the header slots when ``values`` are
    the layout's block counts and sizes (``Layout.header_values()``). Runs on the host."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros(len(v), np.int32)
    rc = lib().fleet_gate_header_codes(v.ctypes.data, len(v), out.ctypes.data)
    if rc != FLEET_OK:
        raise FleetError(rc, "fleet_gate_header_codes")
    return out


class Vet:
    """One slot's verdict from a :class:`Gate`: ``status`` (0 good, 1 not Base64::encode
    output, 2 a header slot's code is not the model's), ``sumsq`` (the squared norm of the
    flat gradient over the pool's window) and ``max_abs`` (its largest magnitude there)."""

    __slots__ = ("status", "sumsq", "max_abs")

    def __init__(self, status: int, sumsq: float, max_abs: float):
        self.status, self.sumsq, self.max_abs = int(status), float(sumsq), float(max_abs)

    @property
    def norm(self) -> float:
        """``new ByteVec(getFlatGradient(g)).getNorm()`` when the pool holds the whole upload."""
        return float(np.sqrt(self.sumsq))

    def __iter__(self):
        return iter((self.status, self.sumsq, self.max_abs))

    def __eq__(self, other):
        return isinstance(other, Vet) and tuple(self) == tuple(other)

    def __repr__(self):
        return f"Vet(status={self.status}, sumsq={self.sumsq!r}, max_abs={self.max_abs!r})"


class Gate:
    """An upload vetted when it arrives, beside an upload pool (fleet_gate,
    include/fleet_codec.h): one device pass over resident slots that folds nothing and gives
    per slot the Base64 verdict an update would reach, the header codes against the model's,
    and the flat gradient's squared norm and largest magnitude (``new
    ByteVec(getFlatGradient(g)).getNorm()``, cppNN_backend.cpp:701-720, 779-795). ``put`` is
    the pool's ``put`` into a free slot that keeps the upload only when it is good. The gate
    never writes the pool's ``slot_status``. Close it before its pool."""

    def __init__(self, pool: Pool, header_values=None):
        self.pool = pool
        self._L = pool._L
        self._h = None
        self.codes = None if header_values is None else header_codes(header_values)
        h = C.c_void_p()
        pool.codec._check(self._L.fleet_gate_create(
            pool._h, None if self.codes is None else self.codes.ctypes.data, 0 if self.codes is None else len(self.codes),
            C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and getattr(self.pool, "_h", None) and getattr(self.pool.codec, "_h", None):
            self._L.fleet_gate_destroy(self._h)
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
        """The handle, while the gate and its pool are open."""
        if not getattr(self, "_h", None) or not getattr(self.pool, "_h", None):
            raise ValueError("the gate or its pool is closed")
        return self._h

    def vet(self, slots):
        """A list of :class:`Vet`, one per slot of ``slots`` (occupied, distinct), in that order."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        K = len(sl)
        st, ss, mx = np.zeros(K, np.int32), np.zeros(K, np.float64), np.zeros(K, np.float32)
        self.pool.codec._check(self._L.fleet_gate_vet(self._live(), sl.ctypes.data, K, st.ctypes.data, ss.ctypes.data,
                                                      mx.ctypes.data))
        return [Vet(a, b, c) for a, b, c in zip(st, ss, mx)]

    def vet_device(self, slots, status_i32, sumsq_f64, max_abs_f32, stream=None) -> None:
        """The device form: int32, float64 and float32 CUDA tensors of at least ``len(slots)``
        entries receive the results on ``stream``; nothing is synchronised."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        for t, dt in ((status_i32, "int32"), (sumsq_f64, "float64"), (max_abs_f32, "float32")):
            if str(t.dtype) != "torch." + dt or not t.is_cuda or not t.is_contiguous() or t.numel() < len(sl):
                raise ValueError(f"a contiguous {dt} CUDA tensor of at least {len(sl)} entries per output")
        self.pool.codec._check(self._L.fleet_gate_vet_device(self._live(), sl.ctypes.data, len(sl), status_i32.data_ptr(),
                                                             sumsq_f64.data_ptr(), max_abs_f32.data_ptr(),
                                                             _stream(stream)))

    def put(self, slot: int, upload) -> Vet:
        """``Pool.put`` into the free slot ``slot`` (an occupied one raises), then its vet. The
        upload stays in the slot only when the returned ``status`` is 0; a refused upload
        leaves the slot free and the pool as it was."""
        s = _as_bytes(upload)
        st, ss, mx = C.c_int32(0), C.c_double(0.0), C.c_float(0.0)
        rc = self._L.fleet_gate_put(self._live(), int(slot), s, len(s), C.byref(st), C.byref(ss), C.byref(mx))
        if rc not in (FLEET_OK, FLEET_ERR_BASE64, FLEET_ERR_LAYOUT):
            self.pool.codec._check(rc)
        return Vet(st.value, ss.value, mx.value)


class Ledger:
    """Kardam's ``grads`` map kept in HBM beside an upload pool (fleet_kledger,
    include/fleet_codec.h; Kardam.java:56-71): ``update`` / ``update_device`` are the pool's
    plus ``setGrad`` for every pick, in pick order -- the gradient norm, the norm of the
    difference to the worker's previous gradient and the ``setGrad`` result per pick -- from
    the one pass over the picked rows that produces the merged bytes. When an update raises
    ``Base64Error`` or ``LayoutError`` the ledger and the pool are as before and the
    exception's ``slots`` lists the slots at fault. Close it before its pool."""

    def __init__(self, pool: Pool, workers: int, max_store: int):
        self.pool = pool
        self._L = pool._L
        self._h = None
        h = C.c_void_p()
        pool.codec._check(self._L.fleet_kledger_create(pool._h, int(workers), int(max_store), C.byref(h)))
        self._h = h
        self.workers = int(self._L.fleet_kledger_workers(h))
        self.max_store = int(max_store)

    def close(self):
        if getattr(self, "_h", None) and getattr(self.pool, "_h", None) and getattr(self.pool.codec, "_h", None):
            self._L.fleet_kledger_destroy(self._h)
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
        """The handle, while the ledger and its pool are open."""
        if not getattr(self, "_h", None) or not getattr(self.pool, "_h", None):
            raise ValueError("the ledger or its pool is closed")
        return self._h

    def has(self, worker: int) -> bool:
        v = self._L.fleet_kledger_has(self._live(), int(worker))
        if v < 0:
            raise FleetError(v, f"worker {worker} outside [0, {self.workers})")
        return bool(v)

    def epoch(self, worker: int) -> int:
        """The epoch recorded with the worker's gradient (the worker must be in the ledger)."""
        e = C.c_int(0)
        self.pool.codec._check(self._L.fleet_kledger_epoch(self._live(), int(worker), C.byref(e)))
        return int(e.value)

    def forget(self, worker: int) -> None:
        self.pool.codec._check(self._L.fleet_kledger_forget(self._live(), int(worker)))

    def read(self, worker: int):
        """The worker's gradient: float32 in upload coordinates, header slots 0."""
        g = np.zeros(b64_count(self.pool.length), np.float32)
        self.pool.codec._check(self._L.fleet_kledger_read(self._live(), int(worker), g.ctypes.data, len(g)))
        return g

    def _args(self, picks, dampens, workers, epochs):
        pk, d = Pool._pick_args(picks, dampens)
        w = np.ascontiguousarray(workers, dtype=np.int32)
        e = np.ascontiguousarray(epochs, dtype=np.int32)
        if len(w) != len(pk) or len(e) != len(pk):
            raise ValueError("one worker and one epoch per pick")
        K = len(pk)
        return pk, d, w, e, np.full(K, np.nan), np.full(K, np.nan), np.zeros(K, np.uint8)

    def update(self, picks, dampens, workers, epochs, lr: float, want_f32: bool = False):
        """``Pool.update`` over ``picks`` plus ``setGrad(workers[k], g_k * lr, epochs[k])`` for
        each pick (``workers[k] < 0``: none for that pick). Returns ``(merged, f32 or None,
        norm_g, norm_diff, set)``; a norm that ``setGrad`` does not compute is NaN."""
        pk, d, w, e, ng, nd, st = self._args(picks, dampens, workers, epochs)
        length = self.pool.length
        out = np.zeros(length + 16, np.uint8)
        n = C.c_size_t(0)
        f32 = np.zeros(b64_count(length) + 1, np.float32) if want_f32 else None
        self.pool._check(self._L.fleet_kledger_update(
            self._live(), pk.ctypes.data, len(pk), d.ctypes.data, w.ctypes.data, e.ctypes.data, float(lr), out.ctypes.data,
            len(out), C.byref(n), f32.ctypes.data if want_f32 else None, ng.ctypes.data, nd.ctypes.data,
            st.ctypes.data), pk)
        return (out[: n.value].tobytes(), f32[: b64_count(length)].copy() if want_f32 else None, ng, nd,
                st.astype(bool))

    def update_device(self, picks, dampens, workers, epochs, lr: float, merged_u8, merged_f32=None, stream=None):
        """The device form (``Pool.update_device``'s tensors). Returns ``(norm_g, norm_diff, set)``."""
        pk, d, w, e, ng, nd, st = self._args(picks, dampens, workers, epochs)
        if merged_u8.numel() < 16 * self.pool.groups or (
                merged_f32 is not None and merged_f32.numel() < b64_count(self.pool.length)):
            raise ValueError("merged tensors smaller than the upload's groups")
        self.pool._check(self._L.fleet_kledger_update_device(
            self._live(), pk.ctypes.data, len(pk), d.ctypes.data, w.ctypes.data, e.ctypes.data, float(lr),
            merged_u8.data_ptr(), merged_f32.data_ptr() if merged_f32 is not None else None, ng.ctypes.data,
            nd.ctypes.data, st.ctypes.data, _stream(stream)), pk)
        return ng, nd, st.astype(bool)

    def filter(self, n_weights: int, n_biases: int, graph_edges: int) -> "KardamFilter":
        """A Kardam filter (fleet_kfilter) over this ledger for a model of ``n_weights``
        weights and ``n_biases`` biases repeated ``graph_edges`` times (``Model.shape()``)."""
        return KardamFilter(self, n_weights, n_biases, graph_edges)


class KardamFilter:
    """What ``Kardam.checkByz`` reads of an update's picks, kept in HBM beside a ledger
    (fleet_kfilter, include/fleet_codec.h; Kardam.java:136-185). ``set_model`` stages
    currModel and returns its norms; ``update`` is ``Ledger.update`` plus, for every pick,
    the norm of its dampened gradient and of its difference to the last average, and leaves
    the update pending; the caller decides (``updater.Kardam.check_byz``) and ``resolve``
    gives the merged bytes of the accepted picks, or None when none was accepted. Between
    ``update`` and ``resolve`` no picked slot may be put into or dropped. Close it before
    its ledger."""

    def __init__(self, ledger: Ledger, n_weights: int, n_biases: int, graph_edges: int):
        self.ledger = ledger
        self.pool = ledger.pool
        self._L = ledger._L
        self._h = None
        self.n_weights, self.n_biases, self.graph_edges = int(n_weights), int(n_biases), int(graph_edges)
        h = C.c_void_p()
        self.pool.codec._check(self._L.fleet_kfilter_create(ledger._live(), self.n_weights, self.n_biases,
                                                            self.graph_edges, C.byref(h)))
        self._h = h

    def close(self):
        if (getattr(self, "_h", None) and getattr(self.ledger, "_h", None) and getattr(self.pool, "_h", None)
                and getattr(self.pool.codec, "_h", None)):
            self._L.fleet_kfilter_destroy(self._h)
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
        if not getattr(self, "_h", None):
            raise ValueError("the filter is closed")
        self.ledger._live()
        return self._h

    @property
    def has_last(self) -> bool:
        """lastGrad != null: an earlier update of this filter ended with an average."""
        return bool(self._L.fleet_kfilter_has_last(self._live()))

    def set_model(self, weights, biases):
        """currModel from its weights and use_bias() biases (``Model.export``'s vectors).
        Returns ``(norm_model, norm_model_diff)``, the second NaN while there is no last model."""
        w = np.ascontiguousarray(weights, dtype=np.float32)
        b = np.ascontiguousarray(biases, dtype=np.float32)
        if len(w) != self.n_weights or len(b) != self.n_biases:
            raise ValueError(f"the filter holds {self.n_weights} weights and {self.n_biases} biases")
        nm, nd = C.c_double(0), C.c_double(0)
        self.pool.codec._check(self._L.fleet_kfilter_set_model(
            self._live(), w.ctypes.data if len(w) else None, b.ctypes.data if len(b) else None, C.byref(nm), C.byref(nd)))
        return float(nm.value), float(nd.value)

    def set_model_device(self, weights_f32, biases_f32, stream=None):
        """``set_model`` from float32 tensors on the codec's device (``ResidentModel.version_tensors``)."""
        if weights_f32.numel() != self.n_weights or biases_f32.numel() != self.n_biases:
            raise ValueError(f"the filter holds {self.n_weights} weights and {self.n_biases} biases")
        nm, nd = C.c_double(0), C.c_double(0)
        self.pool.codec._check(self._L.fleet_kfilter_set_model_device(
            self._live(), weights_f32.data_ptr() if self.n_weights else None,
            biases_f32.data_ptr() if self.n_biases else None, C.byref(nm), C.byref(nd), _stream(stream)))
        return float(nm.value), float(nd.value)

    def _check_tensors(self, merged_u8, merged_f32):
        if merged_u8.numel() < 16 * self.pool.groups or (
                merged_f32 is not None and merged_f32.numel() < b64_count(self.pool.length)):
            raise ValueError("merged tensors smaller than the upload's groups")

    def update(self, picks, dampens, workers, epochs, lr: float, want_f32: bool = False):
        """``Ledger.update`` with every pick accepted, plus the filter's norms. Returns
        ``(merged, f32 or None, norm_g, norm_diff, set, norm_p, norm_pdiff)``; ``norm_pdiff``
        is NaN while ``has_last`` is false. The update is then pending."""
        pk, d, w, e, ng, nd, st = self.ledger._args(picks, dampens, workers, epochs)
        K = len(pk)
        np_, npd = np.full(K, np.nan), np.full(K, np.nan)
        length = self.pool.length
        out = np.zeros(length + 16, np.uint8)
        n = C.c_size_t(0)
        f32 = np.zeros(b64_count(length) + 1, np.float32) if want_f32 else None
        self.pool._check(self._L.fleet_kfilter_update(
            self._live(), pk.ctypes.data, K, d.ctypes.data, w.ctypes.data, e.ctypes.data, float(lr), out.ctypes.data,
            len(out), C.byref(n), f32.ctypes.data if want_f32 else None, ng.ctypes.data, nd.ctypes.data, st.ctypes.data,
            np_.ctypes.data, npd.ctypes.data), pk)
        return (out[: n.value].tobytes(), f32[: b64_count(length)].copy() if want_f32 else None, ng, nd,
                st.astype(bool), np_, npd)

    def update_device(self, picks, dampens, workers, epochs, lr: float, merged_u8, merged_f32=None, stream=None):
        """The device form. Returns ``(norm_g, norm_diff, set, norm_p, norm_pdiff)``."""
        pk, d, w, e, ng, nd, st = self.ledger._args(picks, dampens, workers, epochs)
        K = len(pk)
        np_, npd = np.full(K, np.nan), np.full(K, np.nan)
        self._check_tensors(merged_u8, merged_f32)
        self.pool._check(self._L.fleet_kfilter_update_device(
            self._live(), pk.ctypes.data, K, d.ctypes.data, w.ctypes.data, e.ctypes.data, float(lr),
            merged_u8.data_ptr(), merged_f32.data_ptr() if merged_f32 is not None else None, ng.ctypes.data,
            nd.ctypes.data, st.ctypes.data, np_.ctypes.data, npd.ctypes.data, _stream(stream)), pk)
        return ng, nd, st.astype(bool), np_, npd

    def resolve(self, accept, want_f32: bool = False):
        """The pending update's result for the decisions ``accept`` (one per pick): the merged
        bytes (``(merged, f32)`` with ``want_f32``), or None when no pick was accepted."""
        a = np.ascontiguousarray(np.asarray(accept, dtype=bool), dtype=np.uint8)
        length = self.pool.length
        out = np.zeros(length + 16, np.uint8)
        n = C.c_size_t(0)
        f32 = np.zeros(b64_count(length) + 1, np.float32) if want_f32 else None
        self.pool._check(self._L.fleet_kfilter_resolve(self._live(), a.ctypes.data, len(a), out.ctypes.data, len(out),
                                                       C.byref(n), f32.ctypes.data if want_f32 else None))
        if n.value == 0:
            return None
        merged = out[: n.value].tobytes()
        return (merged, f32[: b64_count(length)].copy()) if want_f32 else merged

    def resolve_device(self, accept, merged_u8, merged_f32=None, stream=None) -> bool:
        """The device form: writes the tensors when a pick was accepted and returns whether one was."""
        a = np.ascontiguousarray(np.asarray(accept, dtype=bool), dtype=np.uint8)
        self._check_tensors(merged_u8, merged_f32)
        n = C.c_size_t(0)
        self.pool._check(self._L.fleet_kfilter_resolve_device(
            self._live(), a.ctypes.data, len(a), merged_u8.data_ptr(),
            merged_f32.data_ptr() if merged_f32 is not None else None, C.byref(n), _stream(stream)))
        return n.value != 0


class ModelLedger:
    """Kardam's ``models`` map kept in HBM (fleet_mledger, include/fleet_codec.h;
    Kardam.java:114-125). Model versions are made resident under caller-chosen ids
    (``stage``, ``stage_model``) as the fp32 rows decoding their getModelParametersNative
    text would give; ``update`` is ``setModel`` for every pick of an update, in pick order,
    with the norms of all the row pairs it needs from one device pass. Rows belong to
    versions: a worker's model is a reference to a row. Close it before its codec."""

    STATUS_SKIPPED, STATUS_FIRST, STATUS_IGNORED, STATUS_SET = 0, 1, 2, 3

    def __init__(self, codec: "Codec", n_weights: int, n_biases: int, graph_edges: int, workers: int,
                 max_versions: Optional[int] = None):
        self.codec = codec
        self._L = codec._L
        self._h = None
        self.n_weights, self.n_biases, self.graph_edges = int(n_weights), int(n_biases), int(graph_edges)
        self.workers = int(workers)
        self.max_versions = self.workers if max_versions is None else int(max_versions)
        self.n = self.n_biases * self.graph_edges + self.n_weights
        h = C.c_void_p()
        codec._check(self._L.fleet_mledger_create(codec._h, self.n_weights, self.n_biases, self.graph_edges, self.workers,
                                                  self.max_versions, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and getattr(self.codec, "_h", None):
            self._L.fleet_mledger_destroy(self._h)
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
        if not getattr(self, "_h", None) or not getattr(self.codec, "_h", None):
            raise ValueError("the model ledger or its codec is closed")
        return self._h

    @staticmethod
    def launch_shape():
        """(lanes per wave, values a block takes per pass, blocks per pair at most) of the pair kernel."""
        w, b, m = C.c_int(0), C.c_int(0), C.c_int(0)
        lib().fleet_mledger_launch_shape(C.byref(w), C.byref(b), C.byref(m))
        return w.value, b.value, m.value

    def stage(self, version_id: int, weights, biases) -> None:
        """Make a version resident from its weights and use_bias() biases (``Model.export``'s
        vectors); a resident id is a no-op."""
        w = np.ascontiguousarray(weights, dtype=np.float32)
        b = np.ascontiguousarray(biases, dtype=np.float32)
        if len(w) != self.n_weights or len(b) != self.n_biases:
            raise ValueError(f"the ledger holds {self.n_weights} weights and {self.n_biases} biases")
        self.codec._check(self._L.fleet_mledger_stage(self._live(), int(version_id), w.ctypes.data if len(w) else None,
                                                      b.ctypes.data if len(b) else None))

    def stage_device(self, version_id: int, weights_f32, biases_f32, stream=None) -> None:
        """``stage`` from float32 tensors on the codec's device, on ``stream``."""
        if weights_f32.numel() != self.n_weights or biases_f32.numel() != self.n_biases:
            raise ValueError(f"the ledger holds {self.n_weights} weights and {self.n_biases} biases")
        self.codec._check(self._L.fleet_mledger_stage_device(
            self._live(), int(version_id), weights_f32.data_ptr() if self.n_weights else None,
            biases_f32.data_ptr() if self.n_biases else None, _stream(stream)))

    def stage_model(self, model, version: int) -> int:
        """Make ``models[version]`` of a :class:`Model` or a :class:`ResidentModel` (device to
        device) resident under its ``version_id``; returns the id."""
        vid = C.c_int64(-1)
        stage = (self._L.fleet_rmodel_stage_mledger if isinstance(model, ResidentModel)
                 else self._L.fleet_mledger_stage_model)
        rc = stage(self._live(), model._h, int(version), C.byref(vid))
        if rc != FLEET_OK:
            model._check(rc)
        return int(vid.value)

    def resident(self, version_id: int) -> bool:
        return bool(self._L.fleet_mledger_resident(self._live(), int(version_id)))

    def update(self, version_ids, workers):
        """``setModel(workers[k], version version_ids[k])`` for each pick in order (``workers[k]
        < 0``: Kardam does not run for that pick). Returns ``(norm_model, norm_diff,
        status)``: status 0 skipped, 1 first model (stored), 2 ignored (norm == 0, nothing
        changes), 3 set (stored, ``norm_diff`` the norm); a norm not computed is NaN."""
        ids = np.ascontiguousarray(version_ids, dtype=np.int64)
        w = np.ascontiguousarray(workers, dtype=np.int32)
        if len(ids) != len(w):
            raise ValueError("one version id and one worker per pick")
        K = len(w)
        nm, nd, st = np.full(K, np.nan), np.full(K, np.nan), np.zeros(K, np.uint8)
        h = self._live()
        if K:  # (no pick: nothing to ask)
            self.codec._check(self._L.fleet_mledger_update(h, ids.ctypes.data, w.ctypes.data, K, nm.ctypes.data,
                                                           nd.ctypes.data, st.ctypes.data))
        return nm, nd, st

    def has(self, worker: int) -> bool:
        v = self._L.fleet_mledger_has(self._live(), int(worker))
        if v < 0:
            raise FleetError(v, f"worker {worker} outside [0, {self.workers})")
        return bool(v)

    def version(self, worker: int) -> int:
        """The id of the version the worker holds (the worker must hold one)."""
        vid = C.c_int64(0)
        self.codec._check(self._L.fleet_mledger_version(self._live(), int(worker), C.byref(vid)))
        return int(vid.value)

    def forget(self, worker: int) -> None:
        self.codec._check(self._L.fleet_mledger_forget(self._live(), int(worker)))

    def read(self, worker: int) -> np.ndarray:
        """decodeFloat of the worker's model text: the values of its row."""
        p = np.zeros(self.n, np.float32)
        self.codec._check(self._L.fleet_mledger_read(self._live(), int(worker), p.ctypes.data, len(p)))
        return p

    def read_version(self, version_id: int) -> np.ndarray:
        p = np.zeros(self.n, np.float32)
        self.codec._check(self._L.fleet_mledger_read_version(self._live(), int(version_id), p.ctypes.data, len(p)))
        return p

    @property
    def resident_bytes(self) -> int:
        """HBM the rows take: workers + max_versions rows of n floats rounded up to 4."""
        return 4 * ((self.n + 3) // 4 * 4) * (self.workers + self.max_versions)


def update_multi(codecs: Sequence["Codec"], uploads: Sequence, dampen: Sequence[float], want_f32: bool = False):
    """Codec.update spread over several device contexts from one process
    (fleet_update_multi): context k aggregates a contiguous range of the 3-value
    groups of every upload and writes its slice of the output; byte-identical to
    one context's update. The first context reports errors."""
    if not codecs:
        raise ValueError("no contexts")
    ups = [_as_bytes(u) for u in uploads]
    M = len(ups)
    if M == 0:
        raise ValueError("no uploads")
    if len(dampen) != M:
        raise ValueError("one dampening factor per upload")
    L = lib()
    arr = (C.c_char_p * M)(*ups)
    lens = np.array([len(u) for u in ups], dtype=np.uint64)
    d = np.ascontiguousarray(dampen, dtype=np.float64)
    hs = (C.c_void_p * len(codecs))(*[c._h for c in codecs])
    n_len = len(ups[0])
    out = np.empty(n_len + 16, np.uint8)
    n = C.c_size_t(0)
    f32 = np.empty(b64_count(n_len) + 1, np.float32) if want_f32 else None
    rc = L.fleet_update_multi(C.cast(hs, C.c_void_p), len(codecs), C.cast(arr, C.c_void_p), lens.ctypes.data, M,
                              d.ctypes.data, out.ctypes.data, len(out), C.byref(n),
                              f32.ctypes.data if want_f32 else None)
    codecs[0]._check(rc)
    merged = out[: n.value].tobytes()
    if want_f32:
        return merged, f32[: b64_count(n_len)].copy()
    return merged


def update_rows(codecs: Sequence["Codec"], rows: np.ndarray, length: int, dampen: Sequence[float],
                want_f32: bool = False):
    """fleet_update_rows(_multi): the update over uploads stored as the rows of one host
    array (rows[i, :length] = upload i), on one or several device contexts."""
    if rows.ndim != 2 or rows.dtype != np.uint8 or not rows.flags.c_contiguous:
        raise ValueError("rows: a C-contiguous uint8 array [M, row_pitch]")
    M, pitch = rows.shape
    if len(dampen) != M:
        raise ValueError("one dampening factor per upload")
    d = np.ascontiguousarray(dampen, dtype=np.float64)
    out = np.empty(length + 16, np.uint8)
    n = C.c_size_t(0)
    f32 = np.empty(b64_count(length) + 1, np.float32) if want_f32 else None
    L = lib()
    if len(codecs) == 1:
        rc = L.fleet_update_rows(codecs[0]._h, rows.ctypes.data, pitch, length, M, d.ctypes.data, out.ctypes.data,
                                 len(out), C.byref(n), f32.ctypes.data if want_f32 else None)
    else:
        hs = (C.c_void_p * len(codecs))(*[c._h for c in codecs])
        rc = L.fleet_update_rows_multi(C.cast(hs, C.c_void_p), len(codecs), rows.ctypes.data, pitch, length, M,
                                       d.ctypes.data, out.ctypes.data, len(out), C.byref(n),
                                       f32.ctypes.data if want_f32 else None)
    codecs[0]._check(rc)
    merged = out[: n.value].tobytes()
    if want_f32:
        return merged, f32[: b64_count(length)].copy()
    return merged


class Model:
    """The server's resident model (fleet_model): the state the reference's updater
    natives keep in libnative.so (cppNN_backend.cpp: cnn, models, lrates_vec,
    currEpoch, priority), with the natives' names as methods."""

    def __init__(self, codec: "Codec", params_text, distillation_mode: int = 1, solver: str = "sgd"):
        """fetchParamsNative (cppNN_backend.cpp:282-301): network::read of a getParams text.
        ``solver``: what the server's ``mojo::network cnn(solver.c_str())`` (:40-42) is built
        with, one of :data:`SOLVERS`; its state belongs to ``cnn`` alone and starts at zero."""
        t = _as_bytes(params_text)
        h = C.c_void_p()
        rc = codec._L.fleet_model_load(codec._h, t, len(t), int(distillation_mode), C.byref(h))
        if rc != FLEET_OK:
            raise FleetError(rc, "fleet_model_load failed (see stderr): not a supported getParams text")
        self._h, self._L, self.codec = h, codec._L, codec
        if solver != "sgd":
            self.set_solver(solver)

    def set_solver(self, name: str) -> None:
        """After the load and before the first descent (FleetError otherwise, and for a name
        that is none of :data:`SOLVERS`): allocates the zeroed state."""
        self._check(self._L.fleet_model_set_solver(self._h, str(name).encode()))

    @property
    def solver(self) -> str:
        return SOLVERS[self._L.fleet_model_solver(self._h)]

    def solver_state(self, which: int) -> np.ndarray:
        """State row ``which`` (0: g1, 1: adam's g2) of ``cnn``, one float per weight."""
        out = np.empty(self.shape()[0], np.float32)
        self._check(self._L.fleet_model_solver_state(self._h, int(which), out.ctypes.data, len(out)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.fleet_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != FLEET_OK:
            msg = self._L.fleet_model_last_error(self._h).decode(errors="replace")
            raise (LayoutError if rc == FLEET_ERR_LAYOUT else Base64Error if rc == FLEET_ERR_BASE64 else FleetError)(rc, msg)

    def _text(self, fn, version):
        need = C.c_size_t(0)
        rc = fn(self._h, int(version), None, 0, C.byref(need))
        if rc not in (FLEET_OK, FLEET_ERR_CAPACITY):
            self._check(rc)
        out = np.empty(max(1, need.value), np.uint8)
        self._check(fn(self._h, int(version), out.ctypes.data, need.value, C.byref(need)))
        return out[: need.value].tobytes()

    def initUpdater(self, lrates) -> None:  # noqa: N802  (cppNN_backend.cpp:161-225, model part)
        lr = np.ascontiguousarray(lrates, dtype=np.float64)
        self._check(self._L.fleet_model_init_updater(self._h, lr.ctypes.data, len(lr)))

    def descentNative(self, merged, client_batch_size: int, stale_size: int) -> None:  # noqa: N802  (:329-383)
        m = _as_bytes(merged)
        self._check(self._L.fleet_model_descent(self._h, m, len(m), int(client_batch_size), int(stale_size)))

    def modelsSize(self) -> int:  # noqa: N802  (:324-327)
        return self._L.fleet_model_count(self._h)

    def getParametersNative(self, priority: int) -> bytes:  # noqa: N802  (:244-280)
        return self._text(self._L.fleet_model_get_params, priority)

    def getModelParametersNative(self, priority: int) -> bytes:  # noqa: N802  (:227-242)
        return self._text(self._L.fleet_model_get_model_params, priority)

    def getCurrEpoch(self) -> int:  # noqa: N802
        return self._L.fleet_model_get_epoch(self._h)

    def setCurrEpoch(self, e: int) -> None:  # noqa: N802
        self._L.fleet_model_set_epoch(self._h, int(e))

    def getPriority(self) -> int:  # noqa: N802
        return self._L.fleet_model_get_priority(self._h)

    def setPriority(self, p: int) -> None:  # noqa: N802
        self._L.fleet_model_set_priority(self._h, int(p))

    def getLrate(self) -> float:  # noqa: N802
        return self._L.fleet_model_get_lrate(self._h)

    def shape(self):
        nw, nb = C.c_size_t(0), C.c_size_t(0)
        ge, nl = C.c_int(0), C.c_int(0)
        self._check(self._L.fleet_model_shape(self._h, C.byref(nw), C.byref(nb), C.byref(ge), C.byref(nl)))
        return nw.value, nb.value, ge.value, nl.value

    def version_id(self, version: int) -> int:
        """A stable id of ``models[version]``: indices shift when descentNative drops the
        oldest version, the id of a version never changes."""
        vid = C.c_int64(-1)
        self._check(self._L.fleet_model_version_id(self._h, int(version), C.byref(vid)))
        return int(vid.value)

    def kardam_ledger(self, workers: int, max_versions: Optional[int] = None) -> "ModelLedger":
        """A :class:`ModelLedger` of this model's shape on its codec."""
        nw, nb, ge, _ = self.shape()
        return self.codec.model_ledger(nw, nb, ge, workers, max_versions)

    def evaluate(self, images, labels, version=None, idx=None) -> "Evaluation":
        """What the Driver reports for a version of this model: fetchParamsNative + evaluateNative
        (Driver/src/main/c++/cppNN_backend.cpp:179-205) over ``images[idx]``. ``version``: None =
        the newest of ``models`` (what Evaluator.crossValidation asks for), ``-1`` = ``cnn``, else
        ``models[version]``. The model must be the MNIST network (FleetError otherwise).

        The Driver's view in mode 1: the Driver evaluates the broadcast text, whose weights are
        the quantised dictionary values printed with 6 digits, not the stored version. That is
        ``Model(codec, rm.getParametersNative(v), mode).evaluate(images, labels, version=-1)``:
        the text is read by this project's own network::read and what it read is evaluated."""
        v = self.modelsSize() - 1 if version is None else int(version)
        if version is None and v < 0:
            raise ValueError("the model holds no version yet (initUpdater); version=-1 evaluates cnn")
        rc, ev = _eval_host_call(self._L.fleet_model_evaluate, (self._h, v), images, labels, idx)
        self._check(rc)
        return ev

    def export(self, version: int = -1):
        """(weights, biases) of models[version]; version -1 = the current model."""
        nw, nb, _, _ = self.shape()
        w, b = np.empty(nw, np.float32), np.empty(nb, np.float32)
        self._check(self._L.fleet_model_export(self._h, int(version), w.ctypes.data, nw, b.ctypes.data, nb))
        return w, b


class ResidentModel:
    """:class:`Model` with ``cnn`` and ``models`` resident in HBM (fleet_rmodel): the same
    natives under the same names, bit for bit the same results. A step takes the merged
    gradient where ``update_device`` left it (``descent_device``), a new version is staged
    in a :class:`ModelLedger` device to device, and the parameter texts are formatted on
    the device; no weight travels host to device after the load.

    HBM: ``stats()['resident_bytes'] = 4 * roundup64(n_weights + n_biases) *
    (max_versions + 2)`` -- cnn and a ring of ``max_versions + 1`` version rows (descentNative
    pushes before it pops) -- plus ``stats()['workspace_bytes']`` allocated once at load, plus
    ``4 * n_weights`` per state row of a ``solver`` other than sgd (one; two for adam).
    ``stale_size`` of a step may not exceed ``max_versions``."""

    def __init__(self, codec: "Codec", params_text, distillation_mode: int = 1, max_versions: int = 8,
                 solver: str = "sgd"):
        t = _as_bytes(params_text)
        h = C.c_void_p()
        rc = codec._L.fleet_rmodel_load(codec._h, t, len(t), int(distillation_mode), int(max_versions), C.byref(h))
        if rc != FLEET_OK:
            raise FleetError(rc, "fleet_rmodel_load failed (see stderr): not a supported getParams text")
        self._h, self._L, self.codec = h, codec._L, codec
        self.max_versions = int(max_versions)
        if solver != "sgd":
            self.set_solver(solver)

    def set_solver(self, name: str) -> None:
        """:meth:`Model.set_solver`; the state rows (``n_weights`` floats each) live in HBM and
        count in ``stats()['resident_bytes']``."""
        self._check(self._L.fleet_rmodel_set_solver(self._h, str(name).encode()))

    @property
    def solver(self) -> str:
        return SOLVERS[self._L.fleet_rmodel_solver(self._h)]

    def solver_state(self, which: int) -> np.ndarray:
        out = np.empty(self.shape()[0], np.float32)
        self._check(self._L.fleet_rmodel_solver_state(self._h, int(which), out.ctypes.data, len(out)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.fleet_rmodel_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != FLEET_OK:
            msg = self._L.fleet_rmodel_last_error(self._h).decode(errors="replace")
            raise (LayoutError if rc == FLEET_ERR_LAYOUT else Base64Error if rc == FLEET_ERR_BASE64 else FleetError)(rc, msg)

    def _device_tensor(self, t, dtype: str, name: str) -> None:
        """A kernel is handed t.data_ptr(): anything but a contiguous tensor of that type on the
        codec's device is refused here."""
        import torch
        if (not isinstance(t, torch.Tensor) or t.dtype != getattr(torch, dtype) or not t.is_cuda
                or t.device.index != self.codec.device or not t.is_contiguous()):
            raise ValueError(f"{name}: a contiguous {dtype} tensor on cuda:{self.codec.device}")

    def initUpdater(self, lrates) -> None:  # noqa: N802
        lr = np.ascontiguousarray(lrates, dtype=np.float64)
        self._check(self._L.fleet_rmodel_init_updater(self._h, lr.ctypes.data, len(lr)))

    def descentNative(self, merged, client_batch_size: int, stale_size: int) -> None:  # noqa: N802
        m = _as_bytes(merged)
        self._check(self._L.fleet_rmodel_descent(self._h, m, len(m), int(client_batch_size), int(stale_size)))

    def descent_device(self, merged_f32, stale_size: int, stream=None, n_values: Optional[int] = None) -> None:
        """descentNative from decodeFloat of the merged text in a float32 device tensor (what
        ``update_device`` / ``Pool.update_device`` / ``Ledger.update_device`` write); the first
        ``n_values`` floats (default: all of them) are the gradient."""
        self._device_tensor(merged_f32, "float32", "merged_f32")
        n = merged_f32.numel() if n_values is None else int(n_values)
        if n < 0 or n > merged_f32.numel():
            raise ValueError("n_values exceeds the tensor")
        self._check(self._L.fleet_rmodel_descent_device(self._h, merged_f32.data_ptr(), n, int(stale_size),
                                                        _stream(stream)))

    def modelsSize(self) -> int:  # noqa: N802
        return self._L.fleet_rmodel_count(self._h)

    def getParametersNative(self, priority: int) -> bytes:  # noqa: N802
        cap = self._L.fleet_rmodel_params_cap(self._h)
        out = np.empty(max(1, cap), np.uint8)
        need = C.c_size_t(0)
        self._check(self._L.fleet_rmodel_get_params(self._h, int(priority), out.ctypes.data, cap, C.byref(need)))
        return out[: need.value].tobytes()

    def getModelParametersNative(self, priority: int) -> bytes:  # noqa: N802
        nw, nb, ge, _ = self.shape()
        cap = b64_len(nb * ge + nw)
        out = np.empty(max(1, cap), np.uint8)
        need = C.c_size_t(0)
        self._check(self._L.fleet_rmodel_get_model_params(self._h, int(priority), out.ctypes.data, cap, C.byref(need)))
        return out[: need.value].tobytes()

    def getModelParametersNative_device(self, priority: int, out_u8, stream=None) -> int:  # noqa: N802
        """The a20 text into a uint8 device tensor (its length rounded up to 16, plus 16, at
        least); returns the text's length."""
        self._device_tensor(out_u8, "uint8", "out_u8")
        nw, nb, ge, _ = self.shape()
        n = b64_len(nb * ge + nw)
        if out_u8.numel() < (n + 15) // 16 * 16 + 16:
            raise ValueError("out_u8 smaller than the text's 16-byte groups")
        self._check(self._L.fleet_rmodel_get_model_params_device(self._h, int(priority), out_u8.data_ptr(),
                                                                 _stream(stream)))
        return n

    def getCurrEpoch(self) -> int:  # noqa: N802
        return self._L.fleet_rmodel_get_epoch(self._h)

    def setCurrEpoch(self, e: int) -> None:  # noqa: N802
        self._L.fleet_rmodel_set_epoch(self._h, int(e))

    def getPriority(self) -> int:  # noqa: N802
        return self._L.fleet_rmodel_get_priority(self._h)

    def setPriority(self, p: int) -> None:  # noqa: N802
        self._L.fleet_rmodel_set_priority(self._h, int(p))

    def getLrate(self) -> float:  # noqa: N802
        return self._L.fleet_rmodel_get_lrate(self._h)

    def shape(self):
        nw, nb = C.c_size_t(0), C.c_size_t(0)
        ge, nl = C.c_int(0), C.c_int(0)
        self._check(self._L.fleet_rmodel_shape(self._h, C.byref(nw), C.byref(nb), C.byref(ge), C.byref(nl)))
        return nw.value, nb.value, ge.value, nl.value

    def version_id(self, version: int) -> int:
        vid = C.c_int64(-1)
        self._check(self._L.fleet_rmodel_version_id(self._h, int(version), C.byref(vid)))
        return int(vid.value)

    def version_tensors(self, version: int = -1):
        """(weights, biases) of models[version] (-1: cnn) as float32 tensors over the resident
        row itself: no copy, valid until that version is dropped."""
        import torch
        nw, nb, _, _ = self.shape()
        pw, pb = C.c_void_p(), C.c_void_p()
        self._check(self._L.fleet_rmodel_version_device(self._h, int(version), C.byref(pw), C.byref(pb)))

        def view(ptr, n):
            if n == 0:
                return torch.empty(0, dtype=torch.float32, device=f"cuda:{self.codec.device}")
            iface = {"shape": (n,), "typestr": "<f4", "data": (ptr.value, False), "version": 2}
            holder = type("_Row", (), {"__cuda_array_interface__": iface})()
            return torch.as_tensor(holder, device=f"cuda:{self.codec.device}")
        return view(pw, nw), view(pb, nb)

    def kardam_ledger(self, workers: int, max_versions: Optional[int] = None) -> "ModelLedger":
        nw, nb, ge, _ = self.shape()
        return self.codec.model_ledger(nw, nb, ge, workers, max_versions)

    def export(self, version: int = -1):
        nw, nb, _, _ = self.shape()
        w, b = np.empty(nw, np.float32), np.empty(nb, np.float32)
        self._check(self._L.fleet_rmodel_export(self._h, int(version), w.ctypes.data, nw, b.ctypes.data, nb))
        return w, b

    def _eval_version(self, version):
        v = self.modelsSize() - 1 if version is None else int(version)
        if version is None and v < 0:
            raise ValueError("the model holds no version yet (initUpdater); version=-1 evaluates cnn")
        return v

    def evaluate(self, images, labels, version=None, idx=None) -> "Evaluation":
        """:meth:`Model.evaluate` from the resident row: host images, labels and indices are
        uploaded, no weight crosses PCIe; returns synchronised."""
        rc, ev = _eval_host_call(self._L.fleet_rmodel_evaluate, (self._h, self._eval_version(version)), images, labels, idx)
        self._check(rc)
        return ev

    def evaluate_device(self, images_f32, labels_i32, version=None, idx=None, out=None, stream=None) -> dict:
        """:meth:`evaluate` on tensors where they live: images [N, F >= 784] float32, labels [N]
        int32, idx int32 or None, on this model's device. Runs on ``stream`` (default: torch's
        current) and does not synchronise; returns device tensors ``predictions`` [B] int32,
        ``probabilities`` [B] and ``result`` [3] (float error, float accuracy, the bits of int32
        correct), written into ``out``'s tensors where it has them (``predictions`` /
        ``probabilities`` given as None are not written). :func:`evaluation_from_device` reads
        them. Index errors at ``codec.check()``."""
        n_img, F, B, o = _eval_device_out(images_f32, labels_i32, idx, out)
        self._check(self._L.fleet_rmodel_evaluate_device(self._h, self._eval_version(version), images_f32.data_ptr(),
                                                         n_img, F, labels_i32.data_ptr(), _ptr(idx), B,
                                                         _ptr(o.get("predictions")), _ptr(o.get("probabilities")),
                                                         o["result"].data_ptr(), _stream(stream)))
        return o

    def stats(self) -> dict:
        rb, na = C.c_size_t(0), C.c_int(0)
        self._check(self._L.fleet_rmodel_stats(self._h, C.byref(rb), C.byref(na)))
        return {"resident_bytes": rb.value, "device_allocs": na.value,
                "workspace_bytes": self._L.fleet_rmodel_workspace_bytes(self._h)}


class ByteVec:
    """Mirror of Server/src/main/java/utils/ByteVec.java: a Base64 vector whose
    arithmetic runs through the natives (here: the HIP codec)."""

    def __init__(self, v, codec: Codec):
        self.v = _as_bytes(v)  # ByteVec.java:33-35 clones
        self.codec = codec

    def add(self, other: "ByteVec") -> "ByteVec":  # :85-88
        return ByteVec(self.codec.addNative(self.v, other.v), self.codec)

    def subtract(self, other: "ByteVec") -> "ByteVec":  # :96-99
        return ByteVec(self.codec.subtractNative(self.v, other.v), self.codec)

    def scalarMultiply(self, a: float) -> "ByteVec":  # noqa: N802  :121-123
        return ByteVec(self.codec.scalarMulNative(self.v, a), self.codec)

    def getNorm(self) -> float:  # noqa: N802  :69-71
        return self.codec.getNorm(self.v)
