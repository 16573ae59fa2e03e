"""One device context and what runs on it: :class:`Codec`, the launch plan, the evaluation."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from ._capi import (FLEET_ERR_CAPACITY, FLEET_MAX_HEADERS, FLEET_OK, SOLVERS, FleetError, Handle, _as_bytes, _ptr, _stream,
                    b64_count, b64_len, lib, merged_out, merged_result, raise_for, upload_args)


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


class Codec(Handle):
    """One HIP device context (``fleet_ctx``). Raises if no GPU / library."""

    _destroy = "fleet_destroy"
    _closed = "the codec is closed"

    def __init__(self, device: int = 0):
        L = lib()
        h = C.c_void_p()
        rc = L.fleet_create(device, C.byref(h))
        if rc != FLEET_OK:
            raise FleetError(rc, f"fleet_create(device={device}) failed: no usable MI355X/HIP device")
        self._h = h
        self._L = L
        self.device = device

    # -- error plumbing -------------------------------------------------------
    def _check(self, rc: int):
        if rc != FLEET_OK:
            raise_for(rc, self._L.fleet_last_error(self._h).decode(errors="replace"))

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
        ups, arr, lens, d = upload_args(uploads, dampen)
        M = len(ups)
        L = len(ups[0])
        out, n, f32 = merged_out(L, want_f32)
        rc = self._L.fleet_update(self._h, C.cast(arr, C.c_void_p), lens.ctypes.data, M, d.ctypes.data,
                                  out.ctypes.data, len(out), C.byref(n), f32.ctypes.data if want_f32 else None)
        self._check(rc)
        return merged_result(L, out, n, f32)

    def accumulator(self, length: int, header_pos, group_begin: int = 0, group_end: Optional[int] = None):
        """A streaming accumulator (fleet_acc) for uploads of `length` Base64 bytes with the
        given layout header positions: each upload is folded into a resident sum when it
        arrives, and ``finish`` returns what ``update`` returns for the same uploads."""
        from .streaming import Accumulator
        return Accumulator(self, length, header_pos, group_begin, group_end)

    def pool(self, length: int, header_pos, slots: int, group_begin: int = 0, group_end: Optional[int] = None):
        """An upload pool (fleet_pool) of `slots` resident uploads of `length` Base64 bytes:
        uploads are put into slots when they arrive, and ``update`` over any subset of the
        slots, in any order, returns what ``update`` returns for those uploads in that order."""
        from .streaming import Pool
        return Pool(self, length, header_pos, slots, group_begin, group_end)

    def model_ledger(self, n_weights: int, n_biases: int, graph_edges: int, workers: int,
                     max_versions: Optional[int] = None):
        """A Kardam model ledger (fleet_mledger) for models of ``n_weights`` non-null W floats
        and ``n_biases`` use_bias() biases over ``graph_edges`` layer-graph edges: ``workers``
        worker ids, at most ``max_versions`` (default: ``workers``) resident versions that no
        worker holds."""
        from .kardam import ModelLedger
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


def update_multi(codecs: Sequence["Codec"], uploads: Sequence, dampen: Sequence[float], want_f32: bool = False):
    """Codec.update spread over several device contexts from one process
    (fleet_update_multi): context k aggregates a contiguous range of the 3-value
    groups of every upload and writes its slice of the output; byte-identical to
    one context's update. The first context reports errors."""
    if not codecs:
        raise ValueError("no contexts")
    ups, arr, lens, d = upload_args(uploads, dampen)
    M = len(ups)
    L = lib()
    hs = (C.c_void_p * len(codecs))(*[c._h for c in codecs])
    n_len = len(ups[0])
    out, n, f32 = merged_out(n_len, want_f32)
    rc = L.fleet_update_multi(C.cast(hs, C.c_void_p), len(codecs), C.cast(arr, C.c_void_p), lens.ctypes.data, M,
                              d.ctypes.data, out.ctypes.data, len(out), C.byref(n),
                              f32.ctypes.data if want_f32 else None)
    codecs[0]._check(rc)
    return merged_result(n_len, out, n, f32)


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
    out, n, f32 = merged_out(length, want_f32)
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
    return merged_result(length, out, n, f32)


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
