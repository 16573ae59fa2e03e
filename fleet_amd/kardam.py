"""Kardam's maps beside an upload pool: :class:`Ledger`, :class:`KardamFilter`, :class:`ModelLedger`."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from ._capi import FLEET_OK, FleetError, Handle, _stream, b64_count, lib, merged_out, merged_pair, merged_ptrs, merged_result
from .streaming import Pool


class Ledger(Handle):
    """Kardam's ``grads`` map kept in HBM beside an upload pool (fleet_kledger,
    include/fleet_codec.h; Kardam.java:56-71): ``update`` / ``update_device`` are the pool's
    plus ``setGrad`` for every pick, in pick order -- the gradient norm, the norm of the
    difference to the worker's previous gradient and the ``setGrad`` result per pick -- from
    the one pass over the picked rows that produces the merged bytes. When an update raises
    ``Base64Error`` or ``LayoutError`` the ledger and the pool are as before and the
    exception's ``slots`` lists the slots at fault. Close it before its pool."""

    _destroy, _owners, _closed = "fleet_kledger_destroy", ("pool", "pool.codec"), "the ledger or its pool is closed"

    def __init__(self, pool: Pool, workers: int, max_store: int):
        self.pool = pool
        self._L = pool._L
        self._h = None
        h = C.c_void_p()
        pool.codec._check(self._L.fleet_kledger_create(pool._h, int(workers), int(max_store), C.byref(h)))
        self._h = h
        self.workers = int(self._L.fleet_kledger_workers(h))
        self.max_store = int(max_store)

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
        out, n, f32 = merged_out(length, want_f32)
        self.pool._check(self._L.fleet_kledger_update(
            self._live(), pk.ctypes.data, len(pk), d.ctypes.data, w.ctypes.data, e.ctypes.data, float(lr), out.ctypes.data,
            len(out), C.byref(n), f32.ctypes.data if want_f32 else None, ng.ctypes.data, nd.ctypes.data,
            st.ctypes.data), pk)
        return (*merged_pair(length, out, n, f32), ng, nd, st.astype(bool))

    def update_device(self, picks, dampens, workers, epochs, lr: float, merged_u8, merged_f32=None, stream=None):
        """The device form (``Pool.update_device``'s tensors). Returns ``(norm_g, norm_diff, set)``."""
        pk, d, w, e, ng, nd, st = self._args(picks, dampens, workers, epochs)
        p_u8, p_f32 = merged_ptrs(merged_u8, merged_f32, self.pool.groups, self.pool.length)
        self.pool._check(self._L.fleet_kledger_update_device(
            self._live(), pk.ctypes.data, len(pk), d.ctypes.data, w.ctypes.data, e.ctypes.data, float(lr),
            p_u8, p_f32, ng.ctypes.data,
            nd.ctypes.data, st.ctypes.data, _stream(stream)), pk)
        return ng, nd, st.astype(bool)

    def filter(self, n_weights: int, n_biases: int, graph_edges: int) -> "KardamFilter":
        """A Kardam filter (fleet_kfilter) over this ledger for a model of ``n_weights``
        weights and ``n_biases`` biases repeated ``graph_edges`` times (``Model.shape()``)."""
        return KardamFilter(self, n_weights, n_biases, graph_edges)


class KardamFilter(Handle):
    """What ``Kardam.checkByz`` reads of an update's picks, kept in HBM beside a ledger
    (fleet_kfilter, include/fleet_codec.h; Kardam.java:136-185). ``set_model`` stages
    currModel and returns its norms; ``update`` is ``Ledger.update`` plus, for every pick,
    the norm of its dampened gradient and of its difference to the last average, and leaves
    the update pending; the caller decides (``updater.Kardam.check_byz``) and ``resolve``
    gives the merged bytes of the accepted picks, or None when none was accepted. Between
    ``update`` and ``resolve`` no picked slot may be put into or dropped. Close it before
    its ledger."""

    _destroy, _owners, _closed = "fleet_kfilter_destroy", ("ledger", "pool", "pool.codec"), "the filter is closed"

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

    def _live(self):
        if not getattr(self, "_h", None):
            raise ValueError(self._closed)
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

    def update(self, picks, dampens, workers, epochs, lr: float, want_f32: bool = False):
        """``Ledger.update`` with every pick accepted, plus the filter's norms. Returns
        ``(merged, f32 or None, norm_g, norm_diff, set, norm_p, norm_pdiff)``; ``norm_pdiff``
        is NaN while ``has_last`` is false. The update is then pending."""
        pk, d, w, e, ng, nd, st = self.ledger._args(picks, dampens, workers, epochs)
        K = len(pk)
        np_, npd = np.full(K, np.nan), np.full(K, np.nan)
        length = self.pool.length
        out, n, f32 = merged_out(length, want_f32)
        self.pool._check(self._L.fleet_kfilter_update(
            self._live(), pk.ctypes.data, K, d.ctypes.data, w.ctypes.data, e.ctypes.data, float(lr), out.ctypes.data,
            len(out), C.byref(n), f32.ctypes.data if want_f32 else None, ng.ctypes.data, nd.ctypes.data, st.ctypes.data,
            np_.ctypes.data, npd.ctypes.data), pk)
        return (*merged_pair(length, out, n, f32), ng, nd, st.astype(bool), np_, npd)

    def update_device(self, picks, dampens, workers, epochs, lr: float, merged_u8, merged_f32=None, stream=None):
        """The device form. Returns ``(norm_g, norm_diff, set, norm_p, norm_pdiff)``."""
        pk, d, w, e, ng, nd, st = self.ledger._args(picks, dampens, workers, epochs)
        K = len(pk)
        np_, npd = np.full(K, np.nan), np.full(K, np.nan)
        p_u8, p_f32 = merged_ptrs(merged_u8, merged_f32, self.pool.groups, self.pool.length)
        self.pool._check(self._L.fleet_kfilter_update_device(
            self._live(), pk.ctypes.data, K, d.ctypes.data, w.ctypes.data, e.ctypes.data, float(lr),
            p_u8, p_f32, ng.ctypes.data,
            nd.ctypes.data, st.ctypes.data, np_.ctypes.data, npd.ctypes.data, _stream(stream)), pk)
        return ng, nd, st.astype(bool), np_, npd

    def resolve(self, accept, want_f32: bool = False):
        """The pending update's result for the decisions ``accept`` (one per pick): the merged
        bytes (``(merged, f32)`` with ``want_f32``), or None when no pick was accepted."""
        a = np.ascontiguousarray(np.asarray(accept, dtype=bool), dtype=np.uint8)
        length = self.pool.length
        out, n, f32 = merged_out(length, want_f32)
        self.pool._check(self._L.fleet_kfilter_resolve(self._live(), a.ctypes.data, len(a), out.ctypes.data, len(out),
                                                       C.byref(n), f32.ctypes.data if want_f32 else None))
        return merged_result(length, out, n, f32, empty_is_none=True)

    def resolve_device(self, accept, merged_u8, merged_f32=None, stream=None) -> bool:
        """The device form: writes the tensors when a pick was accepted and returns whether one was."""
        a = np.ascontiguousarray(np.asarray(accept, dtype=bool), dtype=np.uint8)
        p_u8, p_f32 = merged_ptrs(merged_u8, merged_f32, self.pool.groups, self.pool.length)
        n = C.c_size_t(0)
        self.pool._check(self._L.fleet_kfilter_resolve_device(
            self._live(), a.ctypes.data, len(a), p_u8, p_f32, C.byref(n), _stream(stream)))
        return n.value != 0


class ModelLedger(Handle):
    """Kardam's ``models`` map kept in HBM (fleet_mledger, include/fleet_codec.h;
    Kardam.java:114-125). Model versions are made resident under caller-chosen ids
    (``stage``, ``stage_model``) as the fp32 rows decoding their getModelParametersNative
    text would give; ``update`` is ``setModel`` for every pick of an update, in pick order,
    with the norms of all the row pairs it needs from one device pass. Rows belong to
    versions: a worker's model is a reference to a row. Close it before its codec."""

    STATUS_SKIPPED, STATUS_FIRST, STATUS_IGNORED, STATUS_SET = 0, 1, 2, 3
    _destroy, _owners, _closed = "fleet_mledger_destroy", ("codec",), "the model ledger or its codec is closed"

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
        from .model import ResidentModel
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
