"""Uploads kept on the device as they arrive: :class:`Accumulator`, :class:`Pool`, :class:`Gate`."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from ._capi import (FLEET_ERR_BASE64, FLEET_ERR_LAYOUT, FLEET_OK, Base64Error, FleetError, Handle, LayoutError, _as_bytes,
                    _stream, b64_count, lib, merged_out, merged_ptrs, merged_result, upload_args)
from .codec import Codec


class Accumulator(Handle):
    """Streaming aggregation on one context (fleet_acc, include/fleet_codec.h): the
    reference's `acc` of buffered uploads (CppNNUpdater.java:383-391) kept as the running
    sum of the chain instead of the uploads themselves. ``push`` is synchronous and
    transactional (a rejected upload raises and leaves the batch as it was);
    ``push_device`` is asynchronous and commits at once, a bad upload surfacing as a
    sticky error at ``finish*`` or a later push until ``reset``. Uploads that are at
    hand together go in as a burst (``push_many`` / ``push_many_device``: one kernel per
    ``ACC_BURST`` of them, the same bytes as pushing each), and ``push_finish`` /
    ``push_finish_device`` fold the burst that completes a batch and finish in one call."""

    _destroy, _owners, _closed = "fleet_acc_destroy", ("codec",), "the accumulator or its codec is closed"

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
        out, n, f32 = merged_out(self.length, want_f32)
        self.codec._check(self._L.fleet_acc_finish(self._h, out.ctypes.data, len(out), C.byref(n),
                                                   f32.ctypes.data if want_f32 else None))
        return merged_result(self.length, out, n, f32)

    def finish_device(self, merged_u8, merged_f32=None, stream=None) -> None:
        """merged_u8: uint8 CUDA tensor [>= 16 * groups], merged_f32: float32 [>= n values]
        (whole-upload coordinates); synchronises the stream to report a bad device push."""
        p_u8, p_f32 = merged_ptrs(merged_u8, merged_f32, self.groups, self.length)
        self.codec._check(self._L.fleet_acc_finish_device(self._h, p_u8, p_f32, _stream(stream)))

    def reset(self) -> None:
        self.codec._check(self._L.fleet_acc_reset(self._h))

    # bursts: K uploads folded by one kernel per ACC_BURST of them

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
        ups, arr, lens, d = upload_args(uploads, dampens)
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
        ups, arr, lens, d = upload_args(uploads, dampens)
        out, n, f32 = merged_out(self.length, want_f32)
        self.codec._check(self._L.fleet_acc_push_finish(self._h, arr, lens.ctypes.data, len(ups), d.ctypes.data,
                                                        out.ctypes.data, len(out), C.byref(n),
                                                        f32.ctypes.data if want_f32 else None))
        return merged_result(self.length, out, n, f32)

    def push_finish_device(self, u8_tensor, dampens, merged_u8, merged_f32=None, stream=None) -> None:
        """``push_many_device`` and ``finish_device`` in one call; synchronises the stream,
        and a bad row of the burst leaves the accumulator as before the call."""
        K, pitch, d = self._device_rows(u8_tensor, dampens)
        p_u8, p_f32 = merged_ptrs(merged_u8, merged_f32, self.groups, self.length)
        self.codec._check(self._L.fleet_acc_push_finish_device(
            self._h, u8_tensor.data_ptr(), pitch, K, d.ctypes.data, p_u8, p_f32, _stream(stream)))


class Pool(Handle):
    """Buffered uploads kept in HBM (fleet_pool, include/fleet_codec.h): the reference's
    `acc` in the staleSize > 0 branch (CppNNUpdater.java:383-411), where
    StalenessSimulator.stalenessSim picks, at update time, which buffered uploads to
    aggregate and in which order. ``put`` / ``put_device`` store an arrival in a slot,
    ``update`` / ``update_device`` aggregate any subset of occupied slots in the given
    order and change no slot, ``drop`` frees one. When an update raises ``Base64Error`` or
    ``LayoutError`` the pool is as before, and the exception's ``slots`` lists the picked
    slots whose uploads were at fault (``slot_status``)."""

    _destroy, _owners, _closed = "fleet_pool_destroy", ("codec",), "the pool or its codec is closed"

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
        out, n, f32 = merged_out(self.length, want_f32)
        self._check(self._L.fleet_pool_update(self._h, pk.ctypes.data, len(pk), d.ctypes.data, out.ctypes.data, len(out),
                                              C.byref(n), f32.ctypes.data if want_f32 else None), pk)
        return merged_result(self.length, out, n, f32)

    def update_device(self, picks, dampens, merged_u8, merged_f32=None, stream=None) -> None:
        """merged_u8: uint8 CUDA tensor [>= 16 * groups], merged_f32: float32 [>= n values]
        (whole-upload coordinates); synchronises the stream to read the slots' status."""
        pk, d = self._pick_args(picks, dampens)
        p_u8, p_f32 = merged_ptrs(merged_u8, merged_f32, self.groups, self.length)
        self._check(self._L.fleet_pool_update_device(self._h, pk.ctypes.data, len(pk), d.ctypes.data, p_u8, p_f32,
                                                     _stream(stream)), pk)

    def ledger(self, workers: int, max_store: Optional[int] = None) -> "Ledger":
        """A Kardam ledger (fleet_kledger) over this pool: ``workers`` worker ids, at most
        ``max_store`` (default: the pool's slots) picks of one update that store a row."""
        from .kardam import Ledger
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


class Gate(Handle):
    """An upload vetted when it arrives, beside an upload pool (fleet_gate,
    include/fleet_codec.h): one device pass over resident slots that folds nothing and gives
    per slot the Base64 verdict an update would reach, the header codes against the model's,
    and the flat gradient's squared norm and largest magnitude (``new
    ByteVec(getFlatGradient(g)).getNorm()``, cppNN_backend.cpp:701-720, 779-795). ``put`` is
    the pool's ``put`` into a free slot that keeps the upload only when it is good. The gate
    never writes the pool's ``slot_status``. Close it before its pool."""

    _destroy, _owners, _closed = "fleet_gate_destroy", ("pool", "pool.codec"), "the gate or its pool is closed"

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
