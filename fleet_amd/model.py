"""The server's model state: :class:`Model` on the host, :class:`ResidentModel` in HBM."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from ._capi import FLEET_ERR_CAPACITY, FLEET_OK, SOLVERS, FleetError, Handle, _as_bytes, _ptr, _stream, b64_len, raise_for
from .codec import _eval_device_out, _eval_host_call


class _ModelState(Handle):
    """What :class:`Model` and :class:`ResidentModel` share: the natives whose entry points
    differ only in the C prefix (``fleet_model_`` / ``fleet_rmodel_``). A method that one of
    the two documents in its own words is overridden there for the docstring alone."""

    _prefix = ""

    def _fn(self, name: str):
        return getattr(self._L, self._prefix + name)

    @property
    def solver(self) -> str:
        return SOLVERS[self._fn("solver")(self._h)]

    def solver_state(self, which: int) -> np.ndarray:
        out = np.empty(self.shape()[0], np.float32)
        self._check(self._fn("solver_state")(self._h, int(which), out.ctypes.data, len(out)))
        return out

    def _check(self, rc):
        if rc != FLEET_OK:
            raise_for(rc, self._fn("last_error")(self._h).decode(errors="replace"))

    def initUpdater(self, lrates) -> None:  # noqa: N802  (cppNN_backend.cpp:161-225, model part)
        lr = np.ascontiguousarray(lrates, dtype=np.float64)
        self._check(self._fn("init_updater")(self._h, lr.ctypes.data, len(lr)))

    def descentNative(self, merged, client_batch_size: int, stale_size: int) -> None:  # noqa: N802  (:329-383)
        m = _as_bytes(merged)
        self._check(self._fn("descent")(self._h, m, len(m), int(client_batch_size), int(stale_size)))

    def modelsSize(self) -> int:  # noqa: N802  (:324-327)
        return self._fn("count")(self._h)

    def getCurrEpoch(self) -> int:  # noqa: N802
        return self._fn("get_epoch")(self._h)

    def setCurrEpoch(self, e: int) -> None:  # noqa: N802
        self._fn("set_epoch")(self._h, int(e))

    def getPriority(self) -> int:  # noqa: N802
        return self._fn("get_priority")(self._h)

    def setPriority(self, p: int) -> None:  # noqa: N802
        self._fn("set_priority")(self._h, int(p))

    def getLrate(self) -> float:  # noqa: N802
        return self._fn("get_lrate")(self._h)

    def shape(self):
        nw, nb = C.c_size_t(0), C.c_size_t(0)
        ge, nl = C.c_int(0), C.c_int(0)
        self._check(self._fn("shape")(self._h, C.byref(nw), C.byref(nb), C.byref(ge), C.byref(nl)))
        return nw.value, nb.value, ge.value, nl.value

    def version_id(self, version: int) -> int:
        vid = C.c_int64(-1)
        self._check(self._fn("version_id")(self._h, int(version), C.byref(vid)))
        return int(vid.value)

    def kardam_ledger(self, workers: int, max_versions: Optional[int] = None) -> "ModelLedger":
        nw, nb, ge, _ = self.shape()
        return self.codec.model_ledger(nw, nb, ge, workers, max_versions)

    def export(self, version: int = -1):
        nw, nb, _, _ = self.shape()
        w, b = np.empty(nw, np.float32), np.empty(nb, np.float32)
        self._check(self._fn("export")(self._h, int(version), w.ctypes.data, nw, b.ctypes.data, nb))
        return w, b

    def _eval_version(self, version):
        v = self.modelsSize() - 1 if version is None else int(version)
        if version is None and v < 0:
            raise ValueError("the model holds no version yet (initUpdater); version=-1 evaluates cnn")
        return v


class Model(_ModelState):
    """The server's resident model (fleet_model): the state the reference's updater
    natives keep in libnative.so (cppNN_backend.cpp: cnn, models, lrates_vec,
    currEpoch, priority), with the natives' names as methods."""

    _prefix, _destroy, _closed = "fleet_model_", "fleet_model_destroy", "the model is closed"

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

    def solver_state(self, which: int) -> np.ndarray:
        """State row ``which`` (0: g1, 1: adam's g2) of ``cnn``, one float per weight."""
        return super().solver_state(which)

    def _text(self, fn, version):
        need = C.c_size_t(0)
        rc = fn(self._h, int(version), None, 0, C.byref(need))
        if rc not in (FLEET_OK, FLEET_ERR_CAPACITY):
            self._check(rc)
        out = np.empty(max(1, need.value), np.uint8)
        self._check(fn(self._h, int(version), out.ctypes.data, need.value, C.byref(need)))
        return out[: need.value].tobytes()

    def getParametersNative(self, priority: int) -> bytes:  # noqa: N802  (:244-280)
        return self._text(self._L.fleet_model_get_params, priority)

    def getModelParametersNative(self, priority: int) -> bytes:  # noqa: N802  (:227-242)
        return self._text(self._L.fleet_model_get_model_params, priority)

    def version_id(self, version: int) -> int:
        """A stable id of ``models[version]``: indices shift when descentNative drops the
        oldest version, the id of a version never changes."""
        return super().version_id(version)

    def kardam_ledger(self, workers: int, max_versions: Optional[int] = None) -> "ModelLedger":
        """A :class:`ModelLedger` of this model's shape on its codec."""
        return super().kardam_ledger(workers, max_versions)

    def evaluate(self, images, labels, version=None, idx=None) -> "Evaluation":
        """What the Driver reports for a version of this model: fetchParamsNative + evaluateNative
        (Driver/src/main/c++/cppNN_backend.cpp:179-205) over ``images[idx]``. ``version``: None =
        the newest of ``models`` (what Evaluator.crossValidation asks for), ``-1`` = ``cnn``, else
        ``models[version]``. The model must be the MNIST network (FleetError otherwise).

        The Driver's view in mode 1: the Driver evaluates the broadcast text, whose weights are
        the quantised dictionary values printed with 6 digits, not the stored version. That is
        ``Model(codec, rm.getParametersNative(v), mode).evaluate(images, labels, version=-1)``:
        the text is read by this project's own network::read and what it read is evaluated."""
        rc, ev = _eval_host_call(self._L.fleet_model_evaluate, (self._h, self._eval_version(version)), images, labels, idx)
        self._check(rc)
        return ev

    def export(self, version: int = -1):
        """(weights, biases) of models[version]; version -1 = the current model."""
        return super().export(version)


class ResidentModel(_ModelState):
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

    _prefix, _destroy, _closed = "fleet_rmodel_", "fleet_rmodel_destroy", "the model is closed"

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

    def _device_tensor(self, t, dtype: str, name: str) -> None:
        """A kernel is handed t.data_ptr(): anything but a contiguous tensor of that type on the
        codec's device is refused here."""
        import torch
        if (not isinstance(t, torch.Tensor) or t.dtype != getattr(torch, dtype) or not t.is_cuda
                or t.device.index != self.codec.device or not t.is_contiguous()):
            raise ValueError(f"{name}: a contiguous {dtype} tensor on cuda:{self.codec.device}")

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
