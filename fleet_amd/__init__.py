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
from .layouts import LAYOUTS, Layout  # noqa: F401
from ._capi import (FLEET_ERR_ARG, FLEET_ERR_BASE64, FLEET_ERR_CAPACITY, FLEET_ERR_HIP, FLEET_ERR_LAYOUT,  # noqa: F401
                    FLEET_ERR_NOMEM, FLEET_MAX_HEADERS, FLEET_OK, HEADER_PATH, LIB_PATH, PKG, ROOT, SOLVERS, Base64Error,
                    FleetError, LayoutError, _as_bytes, _ptr, _stream, b64_count, b64_len, exported_symbols_from_header,
                    lib)
from .codec import (ByteVec, Codec, Evaluation, _eval_device_out, _eval_host_args, _eval_host_call,  # noqa: F401
                    evaluate_block_images, evaluate_grid_override, evaluation_from_device, layout_from_sizes, plan,
                    plan_override, set_plan, update_encode_kernel, update_kernel, update_multi, update_plan_grid,
                    update_rows)
from .streaming import Accumulator, Gate, Pool, Vet, header_codes  # noqa: F401
from .kardam import KardamFilter, Ledger, ModelLedger  # noqa: F401
from .model import Model, ResidentModel  # noqa: F401
from . import client  # noqa: F401  (the client's gradients: fleet_amd.client.client_gradients ...)


def __getattr__(name):
    # ACC_BURST: uploads one k_acc_push_many launch folds (fleet_acc_burst), read from the
    # library when first asked for, so importing the package does not load it
    if name == "ACC_BURST":
        v = globals()["ACC_BURST"] = int(lib().fleet_acc_burst())
        return v
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
