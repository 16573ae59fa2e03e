"""Mirror of CppNNUpdater's aggregation path on the MI355X codec.

Server/src/main/java/apps/cppNN/CppNNUpdater.java drives the hot path through
JNI: it buffers client uploads until M have arrived (M-softsync, :383-391),
picks them in FIFO order (:420-421), dampens each by ``getDampen(tau,
similarity)`` (:300-327, :463-464), sums and averages them (:490-507), merges
the average into the last picked upload's layout (:508) and calls
``descentNative`` (:509). :class:`FleetUpdater` keeps that control logic on the
host (it is O(M) and O(labels)) and runs the per-element work as two device
calls: ``Codec.update`` (the exact re-quantised dampen/sum/average/merge chain)
and ``Codec.descent`` (sgd on the resident model). With ``streaming=True`` every
upload is instead folded into a resident sum when it arrives (``Codec.accumulator``),
and the M-th call is left with its own push, the finish and the model step.

Scope: the ``staleSize == 0`` branch (``aggregated = acc``, :408-411) with the
pruning thresholds at 0 (their defaults in the quick start), and the
``staleSize > 0`` branch (:394-407) with the caller's ``picker`` in the place of
StalenessSimulator.stalenessSim: the buffered uploads then live in an upload pool
in HBM (``Codec.pool``), the picker names which of them an update aggregates and
in which order, and the rest stay buffered. Staleness simulation itself
(StalenessSimulator) and percentile pruning are the reference's host-side experiment
controls and are not rebuilt; their O(N) natives (getNorm,
subtract) are on :class:`Codec`. Kardam's bookkeeping of the picked uploads (:470-484)
is opt-in in the picker mode (``kardam=``): its gradients live in a ledger beside the
pool, and the pool's fold computes their norms as side outputs; with ``kardam_models=`` its
models live in a model ledger too, and one pass over the picked versions' rows gives every
pick's setModel result. With ``vet=True`` an arrival enters the pool through an arrival gate
(``Pool.gate``), which refuses a malformed or wrong-model upload on the request that brought it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np


def _java_max(a: float, b: float) -> float:
    """Math.max: NaN if either argument is NaN."""
    if a != a or b != b:
        return float("nan")
    return a if a >= b else b


def get_dampen(policy: int, tau: int, similarity: float = 1.0, stale_size: int = 0, alpha: float = 0.0,
               has_outlier: bool = False) -> float:
    """CppNNUpdater.getDampen (:300-327), in Java double arithmetic. (Java's
    Math.exp may differ from libm's exp in the last bit; the factors are inputs
    of the device chain, which is exact for any given value.)"""
    l_tau = 1.0
    if policy == 0:  # average
        l_tau = 1.0
    elif policy == 1:  # inverse
        l_tau = 1 / float(tau + 1)
    elif policy == 2:  # inverse + class-aware
        l_tau = 1 / float(tau + 1)
        if has_outlier and tau > 1.5 * stale_size:
            l_tau /= _java_max(0.1, similarity)
    elif policy == 3:  # exponential
        l_tau = math.exp((-1) * alpha * min(tau, stale_size))
    elif policy == 4:  # exponential + class-aware
        l_tau = math.exp((-1) * alpha * min(tau, stale_size))
        if has_outlier and tau > 1.5 * stale_size:
            l_tau /= _java_max(0.1, similarity)
    return l_tau


def similarity(x: Sequence[int], y: Sequence[int]) -> float:
    """Helpers.similarity (commonLib/utils/Helpers.java:140-161): Bhattacharyya
    coefficient of the two label histograms, each normalised by its sum (an
    all-zero histogram normalises to NaN, as 0.0/0 does in Java)."""
    def norm(v):
        s = float(sum(v))
        return [(a / s) if s != 0 else (float("nan") if a == 0 else math.copysign(math.inf, a)) for a in v]
    b = 0.0
    for a, c in zip(norm(x), norm(y)):
        b += math.sqrt(a) * math.sqrt(c) if a == a and c == c else float("nan")
    return b


def percentile(values: Sequence[float], p: float) -> float:
    """Helpers.percentile (commonLib/utils/Helpers.java:52-59): commons-math3 3.6.1's
    ``new Percentile().evaluate(sorted values, p)`` with its default estimation type
    (``Percentile.EstimationType.LEGACY``, the algorithm of the class's Javadoc): with n
    values, n = 1 gives that value; otherwise ``pos = p * (n + 1) / 100``, ``pos < 1`` gives
    the minimum, ``pos >= n`` the maximum, and anything between
    ``lower + (pos - floor(pos)) * (upper - lower)`` with ``lower`` and ``upper`` the sorted
    values at ranks ``floor(pos)`` and ``floor(pos) + 1`` counted from 1. As there, no value
    gives NaN and a ``p`` outside (0, 100] is an error. Non-finite values are outside what
    is pinned here: Java's sort and the library's NaN strategy order them their own way."""
    if not (0 < p <= 100):
        raise ValueError(f"out of bounds quantile value: {p}, must be in (0, 100]")
    v = sorted(float(x) for x in values)
    n = len(v)
    if n == 0:
        return float("nan")
    if n == 1:
        return v[0]
    pos = p * (n + 1) / 100
    fpos = math.floor(pos)
    if pos < 1:
        return v[0]
    if pos >= n:
        return v[n - 1]
    lower, upper = v[int(fpos) - 1], v[int(fpos)]
    return lower + (pos - fpos) * (upper - lower)


def _java_div(a: float, b: float) -> float:
    """a / b in IEEE double arithmetic, as Java divides: x/0 is an infinity, 0/0 NaN."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return float("nan")
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


class Kardam:
    """utils/Kardam.java's bookkeeping (setGrad :48-62, setModel :93-106, updateLip
    :190-203) with its O(N) vector work on the GPU: the gradient texts and norms of
    all picked uploads come from one ``Codec.kardam_grads`` call,
    the model-difference norm from ``subtractNative`` + ``getNorm`` over two texts, or,
    with a model ledger (``apply_model``), from one device pass over the picked versions'
    resident rows. ``check_byz`` is ``checkByz`` (:136-185) on the norms a
    ``fleet_amd.KardamFilter`` computes: CppNNUpdater bypasses it (``if (true || ...)``,
    :488), ``FleetUpdater(kardam_filter=True)`` runs it."""

    def __init__(self, codec, workers: int = 10, ledger=None, model_ledger=None):
        self.codec = codec
        self.workers = workers
        # ledger-backed mode: `grads` lives in HBM (fleet_amd.Ledger, which an update through
        # the upload pool keeps current); setGrad's results arrive through apply(), and
        # set_grads, which computes texts, is not used
        self.ledger = ledger
        # likewise `models` (fleet_amd.ModelLedger): setModel's results arrive through
        # apply_model(), and set_model, which subtracts texts, is not used
        self.model_ledger = model_ledger
        self.grads = {}           # worker -> (g text, epoch)
        self.models = {}          # worker -> model text
        self.model_diff_norm = {}
        self.grad_diff_norm = {}
        self.lips = {}
        self.subsequent_rejects = 0

    def check_byz(self, worker: int, norm_p: float, norm_pdiff: float, norm_model: float, norm_model_diff: float,
                  has_last: bool) -> bool:
        """checkByz (Kardam.java:136-185) for one pick from its norms: ``norm_p`` =
        getNorm(g), ``norm_pdiff`` = getNorm(g.subtract(lastGrad)), ``norm_model`` =
        getNorm(currModel), ``norm_model_diff`` = getNorm(currModel.subtract(lastModel));
        ``has_last``: lastGrad != null. ``worker`` is not read, as there. Every worker's lips
        are sorted in place on the way (:149), which changes the value a later ``update_lip``
        drops."""
        if not self.lips:  # :138-141
            self.subsequent_rejects = 0
            return True
        top = []
        for w in self.lips:  # :142-151
            top.append(max(self.lips[w]))
            self.lips[w].sort()
        high = percentile(top, 200 / 3.0)  # :156
        if not has_last:  # :159-162
            check_norm = _java_div(norm_p, norm_model)
        else:  # :163-169
            check_norm = _java_div(norm_pdiff, norm_model_diff)
        if check_norm <= high:  # :170-173 (NaN compares false: rejected below)
            self.subsequent_rejects = 0
            return True
        if self.subsequent_rejects == self.workers:  # :174-178
            self.subsequent_rejects = 0
            return True
        self.subsequent_rejects += 1  # :179-182
        return False

    def set_grads(self, worker_ids, uploads, dampen, lr: float, epochs):
        """setGrad for each picked upload: one device pass computes every g_c and its
        difference norm to the worker's previous g. Returns the setGrad results."""
        worker_ids = list(worker_ids)
        if len(set(worker_ids)) < len(worker_ids):  # a worker twice in one batch: its pushes in order
            out = []
            for i in range(len(worker_ids)):
                out += self.set_grads(worker_ids[i:i + 1], uploads[i:i + 1], dampen[i:i + 1], lr, epochs[i:i + 1])
            return out
        prev = [self.grads[w][0] if w in self.grads else None for w in worker_ids]
        texts, _, diff = self.codec.kardam_grads(uploads, dampen, lr, prev)
        out = []
        for w, g, dn, ep in zip(worker_ids, texts, diff, epochs):
            if w in self.grads:
                if self.grads[w][1] == ep:  # same epoch as the previous push: ignored
                    out.append(False)
                    continue
                self.grad_diff_norm[w] = float(dn)
                self.grads[w] = (g, ep)
                out.append(True)
            else:
                self.grads[w] = (g, ep)
                out.append(False)
        return out

    def apply(self, worker: int, set_flag: bool, norm_diff: float) -> bool:
        """One pick's setGrad result as the ledger computed it (``Ledger.update``'s ``set`` and
        ``norm_diff``): gradDiffNorm is recorded when setGrad returned true (Kardam.java:63-65).
        Returns ``set_flag``."""
        if set_flag:
            self.grad_diff_norm[worker] = float(norm_diff)
        return bool(set_flag)

    def set_model(self, worker: int, model_text: bytes) -> None:
        if worker in self.models:
            norm = self.codec.getNorm(self.codec.subtractNative(model_text, self.models[worker]))
            if norm == 0:  # same model as before: ignored
                return
            self.model_diff_norm[worker] = norm
        self.models[worker] = model_text

    def apply_model(self, worker: int, status: int, norm_diff: float) -> int:
        """One pick's setModel result as the model ledger computed it (``ModelLedger.update``'s
        ``status`` and ``norm_diff``): modelDiffNorm is recorded when the model was set over a
        previous one (status 3, Kardam.java:122); a first model (1) and an ignored one (2,
        :118-121) record nothing. The models themselves stay in the ledger. Returns ``status``."""
        if int(status) == 3:
            self.model_diff_norm[worker] = float(norm_diff)
        return int(status)

    def update_lip(self, worker: int) -> None:
        lip = self.grad_diff_norm[worker] / self.model_diff_norm[worker]
        lst = self.lips.setdefault(worker, [])
        if len(lst) > 25:
            lst.pop(0)
        lst.append(lip)


@dataclass
class Pending:
    upload: bytes
    labels: List[int]
    epoch: int
    client_id: int
    dampen: Optional[float] = None  # streaming: the pick's factor, computed when it arrived
    slot: Optional[int] = None      # picker: the upload's slot in the pool


class _HostSeat:
    """The model on the host: ``weights``, ``fc_bias`` and the ``lrates`` schedule, stepped by ``codec.descent``
    (always sgd). A batch is merged by the host form of its update call: ``(merged, fp32 gradient, ...)``."""

    model = None
    fused_finish = True  # update_many: push_finish folds a run and merges the batch in one call

    def __init__(self, updater, weights, fc_bias):
        self.u = updater  # its codec, layout, lrates and curr_epoch are read when they are used
        self.lr = np.float32(updater.lrates[0])  # initUpdater: cnn.set_learning_rate(lrates_vec[0])
        self.weights = np.array(weights, dtype=np.float32, copy=True)
        self.fc_bias = np.array(fc_bias, dtype=np.float32, copy=True)

    def rate(self) -> float:
        """getLrate() before descentNative (:478): the rate of the previous step."""
        return float(self.lr)

    def merge(self, obj, form: str, length: int, *args, **host_kw):
        """``obj.<form>(*args, **host_kw)``; the result begins with ``(merged, fp32)``."""
        return getattr(obj, form)(*args, **host_kw)

    def merge_uploads(self, uploads, dampen):
        """A FIFO batch of upload texts: ``(result, length for step)``."""
        return self.u.codec.update(uploads, dampen, want_f32=True), None

    def step(self, result, length) -> bytes:
        """descentNative (cppNN_backend.cpp:329-353): lr from the schedule, then the model step."""
        u, (merged, grad) = self.u, result[:2]
        if u.curr_epoch < len(u.lrates):
            self.lr = np.float32(u.lrates[u.curr_epoch])
        self.weights, self.fc_bias = u.codec.descent(self.weights, self.fc_bias, grad, u.layout, self.lr)
        return merged


class _ResidentSeat:
    """The model in HBM (a ``fleet_amd.ResidentModel``). A batch is merged by the ``_device`` form of its
    update call into tensors the seat keeps, the model steps there (``descent_device``), and only the
    merged text comes back to the host, for the return value. ``weights`` / ``fc_bias`` are not used."""

    weights = fc_bias = None
    fused_finish = False  # the finish is the accumulator's device form, in _finish_batch

    def __init__(self, updater, model):
        self.u, self.model = updater, model
        self.lr = np.float32(updater.lrates[0])
        self._merged_u8 = self._merged_f32 = None
        if model.modelsSize() == 0:
            model.initUpdater(updater.lrates)

    def rate(self) -> float:
        return float(self.model.getLrate())

    def outputs(self, length: int):
        """The tensors a device-form update writes: the merged text and decodeFloat of it."""
        import torch
        from ._capi import b64_count
        groups = (b64_count(length) + 2) // 3
        if self._merged_u8 is None or self._merged_u8.numel() < 16 * groups + 16:
            dev = f"cuda:{self.u.codec.device}"
            self._merged_u8 = torch.zeros(16 * groups + 16, dtype=torch.uint8, device=dev)
            self._merged_f32 = torch.zeros(3 * groups + 4, dtype=torch.float32, device=dev)
        return self._merged_u8, self._merged_f32

    def merge(self, obj, form: str, length: int, *args, **host_kw):
        """``obj.<form>_device(*args, merged_u8, merged_f32)``: the host form's result less (merged, fp32)."""
        return getattr(obj, form + "_device")(*args, *self.outputs(length))

    def merge_uploads(self, uploads, dampen):
        import torch
        length = len(uploads[0])
        if any(len(u) != length for u in uploads):
            raise ValueError("the batch's uploads differ in length (one model layout)")
        mu8, mf32 = self.outputs(length)
        pitch = (length + 15) // 16 * 16 + 16
        rows = np.zeros((len(uploads), pitch), np.uint8)
        for i, u in enumerate(uploads):
            rows[i, :length] = np.frombuffer(u, np.uint8)
        d_rows = torch.from_numpy(rows).to(f"cuda:{self.u.codec.device}")
        self.u.codec.update_device(d_rows, length, dampen, self.u.layout.header_positions(), mu8, mf32)
        self.u.codec.check()  # a malformed upload raises before the model steps
        return None, length

    def step(self, result, length: int) -> bytes:
        """descentNative from the merged gradient in HBM; the merged text is all that is copied to the host."""
        from ._capi import b64_count
        self.model.descent_device(self._merged_f32, self.u.stale_size, n_values=b64_count(length))
        self.lr = np.float32(self.model.getLrate())
        return self._merged_u8[:length].cpu().numpy().tobytes()


class FleetUpdater:
    """CppNNUpdater.update's aggregation + descentNative's model step.

    ``weights`` (the non-null W concatenated in slot order) and ``fc_bias`` (the fully-connected layers'
    biases) are the model the server keeps (``cnn`` in cppNN_backend.cpp); ``lrates`` is initUpdater's
    schedule (cppNN_backend.cpp:161-172). With ``model=`` (a ``fleet_amd.ResidentModel``) the model lives
    in HBM instead: ``weights`` and ``fc_bias`` may be None, every path runs the device form of its update
    into tensors the updater keeps and steps the model there (``descent_device``), and only the merged
    text comes back to the host. ``kardam_models=`` may be that same model. The model steps under the
    solver it was made with (``ResidentModel(..., solver=)``); the ``weights=`` / ``fc_bias=`` path keeps
    no solver state and is always sgd."""

    def __init__(self, codec, layout, M: int, lrates: Sequence[float], weights, fc_bias, policy: int = 0,
                 alpha: float = 0.0, stale_size: int = 0, num_labels: int = 10, has_outlier: bool = False,
                 streaming: bool = False, picker=None, pool_slots: Optional[int] = None, kardam=None,
                 kardam_model=None, kardam_models=None, model=None, kardam_filter: bool = False, vet: bool = False,
                 vet_max_norm: Optional[float] = None):
        if model is None and (weights is None or fc_bias is None):
            raise ValueError("weights and fc_bias are the model the updater steps: give them, or model= (a "
                             "fleet_amd.ResidentModel that holds them in HBM)")
        if kardam_model is not None and kardam_models is not None:
            raise ValueError("kardam_model (a callback that returns texts) and kardam_models (a fleet_amd.Model whose "
                             "versions go through a model ledger) are two ways to the same models: give one")
        if kardam is not None and (picker is None or (kardam_model is None and kardam_models is None)):
            raise ValueError("Kardam's bookkeeping runs in the staleSize > 0 branch: kardam needs a picker and a "
                             "kardam_model or kardam_models")
        if kardam_filter and (kardam is None or kardam_models is None):
            raise ValueError("kardam_filter runs checkByz on the picks of the pooled branch: it needs a picker, kardam "
                             "and kardam_models (the model whose newest version is currModel)")
        if stale_size != 0 and picker is None:
            raise NotImplementedError("staleness simulation (StalenessSimulator) is not rebuilt: staleSize != 0 needs a "
                                      "picker")
        if picker is not None and streaming:
            raise ValueError("a picker chooses among buffered uploads; streaming folds them on arrival")
        if (vet or vet_max_norm is not None) and picker is None:
            raise ValueError("vet checks an upload on its way into the upload pool: it needs a picker")
        if vet_max_norm is not None and not vet:
            raise ValueError("vet_max_norm is a threshold on the norm the vet computes: it needs vet=True")
        self.codec, self.layout, self.M = codec, layout, M
        self.policy, self.alpha, self.stale_size, self.has_outlier = policy, alpha, stale_size, has_outlier
        self.lrates = [float(v) for v in lrates]
        self._seat = _ResidentSeat(self, model) if model is not None else _HostSeat(self, weights, fc_bias)
        self.curr_epoch = 0
        self.acc: List[Pending] = []
        self.global_labels = [0] * num_labels
        self.last_merged: Optional[bytes] = None
        self.streaming = bool(streaming)  # (_push)
        self.picker = picker  # (_pick)
        self.pool_slots = 4 * M if pool_slots is None else int(pool_slots)
        self.kardam, self.kardam_model, self.kardam_models = kardam, kardam_model, kardam_models  # (_update_picked)
        self.kardam_filter = bool(kardam_filter)  # (_update_filtered)
        self.last_accept: Optional[List[bool]] = None
        self.vet = bool(vet)  # (_arrive)
        self.vet_max_norm = None if vet_max_norm is None else float(vet_max_norm)
        self.refused: List[tuple] = []
        self._stream_acc = self._pool = self._gate = self._ledger = self._mledger = self._filter = None

    weights = property(lambda self: self._seat.weights)
    fc_bias = property(lambda self: self._seat.fc_bias)
    lr = property(lambda self: self._seat.lr)
    model = property(lambda self: self._seat.model)

    def _dampen_of(self, p: "Pending") -> float:
        """getDampen for one pick (:463-464) from the current epoch and label vector."""
        tau = self.curr_epoch - p.epoch
        sim = similarity(p.labels, self.global_labels)
        return get_dampen(self.policy, tau, sim, self.stale_size, self.alpha, self.has_outlier)

    def _add_labels(self, picked) -> None:
        """The picks' label vectors summed into ``global_labels`` (:502-504)."""
        window = [0] * len(self.global_labels)
        for q in picked:
            for j, v in enumerate(q.labels[: len(window)]):
                window[j] += v
        for j, v in enumerate(window):
            self.global_labels[j] += v

    def _close_round(self, result, length, averaged: bool = True) -> Optional[bytes]:
        """The model step on the merged gradient an update left (``result``, ``length``: what the seat's
        merge gave), then the epoch. With nothing averaged (``avg == null``, :506-512: the filter
        accepted no pick) there is no model step, the epoch stays and the round returns None."""
        if not averaged:
            return None
        merged = self._seat.step(result, length)
        self.curr_epoch += 1
        self.last_merged = merged
        return merged

    def _leave(self, picked) -> None:
        """Uploads leave the pool and `acc`: the picked ones (:421, :516), whatever was decided about them,
        or the ones an update found at fault. Everything else stays buffered."""
        for q in picked:
            self._pool.drop(q.slot)
        gone = {q.slot for q in picked}
        self.acc = [q for q in self.acc if q.slot not in gone]

    def update(self, upload: bytes, labels: Sequence[int], epoch: int, client_id: int = 0) -> Optional[bytes]:
        """One client upload (CppNNUpdater.update, :330-518). Returns the merged gradient when this upload
        completed a batch of M (and the model stepped), else None."""
        p = Pending(bytes(upload), list(labels), int(epoch), int(client_id))
        if self.picker is not None:
            return self._update_pooled(p)
        if self.streaming:
            self._push(p)
        self.acc.append(p)
        return None if len(self.acc) < self.M else self._finish_batch()  # M-softsync (:388-391)

    def _open_acc(self, length: int):
        """The accumulator for uploads of ``length`` bytes: opened, or re-opened between batches for a new one."""
        a = self._stream_acc
        if a is None or (a.length != length and a.count == 0):
            if a is not None:
                a.close()
            a = self._stream_acc = self.codec.accumulator(length, self.layout.header_positions())
        return a

    def _push(self, p: "Pending") -> None:
        """streaming: every upload is folded into a resident sum when it arrives (Codec.accumulator), so
        the M-th call is left with one push, the finish and the model step. With staleSize == 0 picking
        order is arrival order (:409, :421) and getDampen reads only curr_epoch and global_labels, which
        change inside the M-th call alone (:502-504, descentNative): the factor computed at arrival is
        the one _finish_batch's loop computes for that pick."""
        a = self._open_acc(len(p.upload))
        p.dampen = self._dampen_of(p)
        a.push(p.upload, p.dampen)  # a malformed upload raises here and joins nothing
        p.upload = b""

    def _finish_batch(self, fused=None) -> bytes:
        """The M-th call's part after the arrival (:420-421, :463-464, :490-516): picks the batch, merges
        it (``fused``: the (merged, grad) a push_finish already produced) and steps the model."""
        picked, dampen = [], []
        for _ in range(self.M):  # FIFO (:420-421)
            p = self.acc.pop(0)
            picked.append(p)
            dampen.append(self._dampen_of(p) if p.dampen is None else p.dampen)
        self._add_labels(picked)
        # A merge that raises from here on (codec.update on a malformed upload) leaves the batch popped
        # and its labels summed, unlike the pooled paths, which drop only the slots at fault.
        a = self._stream_acc
        if self.streaming:
            result, length = fused or self._seat.merge(a, "finish", a.length, want_f32=True), a.length
        else:
            result, length = self._seat.merge_uploads([p.upload for p in picked], dampen)
        merged = self._close_round(result, length)
        self.acc.clear()  # aggregated.clear() (:516)
        return merged

    def update_many(self, arrivals) -> List[Optional[bytes]]:
        """Several uploads that are at hand together: ``arrivals`` is a list of ``(upload, labels, epoch,
        client_id)``, the result the list of what ``update`` returns for each in turn. With
        ``streaming=True`` the list is cut at batch boundaries and each run is folded by one call:
        ``push_many`` for a run that leaves the batch open, ``push_finish`` (the fold and the merged
        gradient from one kernel; the host model only) followed by the model step for a run that
        completes it. The factors are computed at arrival, as ``update`` does; ``_dampen_of`` reads
        ``curr_epoch`` and ``global_labels``, which the model step changes, so a run's factors are
        computed after the previous run's step. A run is all or nothing: a malformed upload raises and
        none of its run joins the batch (the runs before it stay)."""
        arrivals = list(arrivals)
        if not self.streaming:
            return [self.update(*a) for a in arrivals]
        out: List[Optional[bytes]] = []
        i = 0
        while i < len(arrivals):
            room = self.M - len(self.acc)
            run = [Pending(bytes(u), list(l), int(e), int(cid)) for u, l, e, cid in arrivals[i: i + room]]
            i += len(run)
            a = self._open_acc(len(run[0].upload))
            for p in run:
                p.dampen = self._dampen_of(p)
            ups, d = [p.upload for p in run], [p.dampen for p in run]
            fused = None
            if len(run) == room and self._seat.fused_finish:
                fused = a.push_finish(ups, d, want_f32=True)
            else:
                a.push_many(ups, d)
            for p in run:
                p.upload = b""
            self.acc.extend(run)
            out += [None] * (len(run) - 1)
            out.append(self._finish_batch(fused) if len(run) == room else None)
        return out

    def _update_pooled(self, p: "Pending") -> Optional[bytes]:
        """One arrival with a picker (:383-411, then :420-516 over the picked uploads)."""
        if not self._arrive(p) or len(self.acc) < self.M:  # M-softsync (:388-391)
            return None
        picked = self._pick()
        if picked is None:  # not possible to update with the buffered uploads (:405-406)
            return None
        dampen = [self._dampen_of(q) for q in picked]  # tau from the epoch at pick time (:427)
        # (before anything changes)
        versions = None if self.kardam is None or self.kardam_models is None else self._kardam_versions(picked)
        if self.kardam_filter:
            return self._update_filtered(picked, dampen, versions)
        result, kd = self._update_picked(picked, dampen, versions)
        if kd is not None:
            (self._kardam_texts_loop if versions is None else self._kardam_models_loop)(picked, *kd)
        self._add_labels(picked)
        merged = self._close_round(result, self._pool.length)
        self._leave(picked)
        return merged

    def _arrive(self, p: "Pending") -> bool:
        """The upload takes a free slot of the pool and joins `acc`; False when it was refused.
        vet: the arrival goes into the pool through an arrival gate (``Pool.gate`` with the layout's
        header codes, ``Gate.put``) instead of ``Pool.put``. An upload that is not Base64::encode output,
        or whose header slots are not this model's, is refused on the request that brought it: it never
        joins `acc`, does not count toward M, and update returns None for it, as for the reference's hash
        mismatch (:350-353). With ``vet_max_norm`` an upload whose flat gradient's norm (new
        ByteVec(getFlatGradient(g)).getNorm()) exceeds it is refused too, its slot dropped. ``refused``
        lists (client_id, status, norm) of every refused arrival."""
        pool = self._pool
        if pool is None:
            pool = self._pool = self.codec.pool(len(p.upload), self.layout.header_positions(), self.pool_slots)
        slot = pool.free_slot()
        if slot is None:  # before anything changes
            raise RuntimeError(f"the upload pool's {pool.slots} slots are all occupied")
        if self.vet:
            if self._gate is None:
                self._gate = pool.gate(self.layout.header_values())
            v = self._gate.put(slot, p.upload)
            over = self.vet_max_norm is not None and not v.norm <= self.vet_max_norm
            if v.status != 0 or over:
                if v.status == 0:  # a good text that is kept out: the slot it took is freed
                    pool.drop(slot)
                self.refused.append((p.client_id, v.status, v.norm))
                return False
        else:
            pool.put(slot, p.upload)
        p.slot, p.upload = slot, b""
        self.acc.append(p)
        return True

    def _pick(self) -> Optional[List[Pending]]:
        """picker: the staleSize > 0 branch (:394-407). ``picker(pending, curr_epoch)`` stands where
        staleSim.stalenessSim stands: called at every arrival once M uploads are buffered, it returns
        ``(picks, discard)`` -- ``picks`` None when no update is possible yet (:405-406), else M distinct
        indices into ``pending`` in pick order; ``discard`` the indices of buffered uploads to drop
        unpicked (the simulator's too-old gradients, which it removes whether or not it picks). The
        uploads wait in a pool of ``pool_slots`` slots in HBM and the update folds the picked slots
        there. Returns the picked uploads, or None; the discarded ones are gone either way."""
        picks, discard = self.picker(list(self.acc), self.curr_epoch)
        picks = None if picks is None else [int(i) for i in picks]
        discard = sorted({int(i) for i in discard or ()})
        n = len(self.acc)
        if any(i < 0 or i >= n for i in discard) or (picks is not None and (
                len(picks) != self.M or len(set(picks)) != self.M or any(i < 0 or i >= n for i in picks)
                or set(picks) & set(discard))):
            raise ValueError("picker: M distinct indices into the buffered uploads, none of them discarded")
        picked = None if picks is None else [self.acc[i] for i in picks]
        for i in reversed(discard):
            self._pool.drop(self.acc.pop(i).slot)
        return picked

    def _kardam_ledger(self):
        """Kardam's `grads` in a ledger beside the pool (``Pool.ledger``), made at first use."""
        if self._ledger is None:
            self._ledger = self.kardam.ledger = self._pool.ledger(self.kardam.workers)
        return self._ledger

    def _update_picked(self, picked, dampen, versions):
        """The update over the picked slots: ``(result, kd)`` with ``result`` for _close_round and ``kd``
        None, or Kardam's ``(models, diff, was_set)`` for the Kardam loop.
        kardam: Kardam's bookkeeping of the picked uploads (:470-484), opt-in. ``kardam`` is a
        :class:`Kardam`; its `grads` then live in a ledger beside the pool, and one ``Ledger.update``
        gives the merged bytes and every pick's setGrad result. ``kardam_model(tau)`` stands where
        getModelParametersNative(modelsSize()-1-tau) and the modelsSize() == staleSize gate stand
        (:472-474): the picked model's text, or None when Kardam does not run for that pick (:483-484).
        The caller holds the fleet_amd.Model with the versions. ``kardam_models``: _kardam_models_loop."""
        pool, seat = self._pool, self._seat
        slots = [q.slot for q in picked]
        try:
            if self.kardam is None:
                return seat.merge(pool, "update", pool.length, slots, dampen, want_f32=True), None
            ledger = self._kardam_ledger()
            models = versions if versions is not None else [
                self.kardam_model(self.curr_epoch - q.epoch) for q in picked]
            workers = [-1 if m is None else q.client_id for q, m in zip(picked, models)]
            result = seat.merge(ledger, "update", pool.length, slots, dampen, workers, [q.epoch for q in picked],
                                seat.rate(), want_f32=True)
            return result, (models, *result[-2:])  # (..., norm_g, norm_diff, set)
        except Exception as e:
            self._drop_at_fault(e)
            raise

    def _drop_at_fault(self, e) -> None:
        """Base64Error / LayoutError of an update: the slots at fault leave, the model stays."""
        bad = set(getattr(e, "slots", ()))
        self._leave([q for q in self.acc if q.slot in bad])

    def _kardam_texts_loop(self, picked, models, diff, was_set) -> None:
        """The Kardam loop over ``kardam_model``'s texts, in the loop's order (:476-480): a worker
        picked twice gets the reference's lips."""
        for q, m, dn, st in zip(picked, models, diff, was_set):
            if m is None:
                continue
            self.kardam.set_model(q.client_id, m)
            if self.kardam.apply(q.client_id, bool(st), float(dn)):
                self.kardam.update_lip(q.client_id)

    def _update_filtered(self, picked, dampen, versions) -> Optional[bytes]:
        """The update over the picked uploads with Kardam's filter (:417-516, :488 without its `true ||`,
        which CppNNUpdater bypasses): currModel's norms, one KardamFilter.update for every pick's
        checkByz norms and the optimistic result in the pass that folds the picks, the Kardam loop with
        the decision after each pick's updateLip (modelsSize() < staleSize or Kardam.check_byz), the
        resolve: the average is over the accepted picks, and an update none of whose picks was accepted
        has no average -- no model step, the epoch stays, update returns None (:506)."""
        from .model import ResidentModel
        pool, seat, km = self._pool, self._seat, self.kardam_models
        n_models = km.modelsSize()
        ledger = self._kardam_ledger()
        if self._filter is None:
            nw, nb, ge, _ = km.shape()
            self._filter = ledger.filter(nw, nb, ge)
        f = self._filter
        workers = [-1 if v is None else q.client_id for q, v in zip(picked, versions)]
        try:
            if isinstance(km, ResidentModel):  # currModel (:417)
                norm_model, norm_model_diff = f.set_model_device(*km.version_tensors(n_models - 1))
            else:
                norm_model, norm_model_diff = f.set_model(*km.export(n_models - 1))
            has_last = f.has_last
            diff, was_set, norm_p, norm_pdiff = seat.merge(
                f, "update", pool.length, [q.slot for q in picked], dampen, workers, [q.epoch for q in picked],
                seat.rate())[-4:]  # (..., norm_g, norm_diff, set, norm_p, norm_pdiff)
        except Exception as e:
            self._drop_at_fault(e)
            raise
        accept: List[bool] = []

        def decide(k: int) -> None:  # :488
            accept.append(n_models < self.stale_size or self.kardam.check_byz(
                picked[k].client_id, float(norm_p[k]), float(norm_pdiff[k]), norm_model, norm_model_diff, has_last))
        self._kardam_models_loop(picked, versions, diff, was_set, decide)
        self.last_accept = list(accept)
        self._add_labels(picked)
        result = seat.merge(f, "resolve", pool.length, accept, want_f32=True)  # None / False: none accepted
        merged = self._close_round(result, pool.length, averaged=bool(result))
        self._leave(picked)
        return merged

    def _kardam_versions(self, picked) -> List[Optional[int]]:
        """The gate of :472-474 for each pick, on ``kardam_models``: the index of the picked
        model in ``models`` (modelsSize()-1-tau), or None when Kardam does not run for the pick
        (no such version any more, :483-484, or modelsSize() != staleSize, :474)."""
        n = self.kardam_models.modelsSize()
        out: List[Optional[int]] = []
        for q in picked:
            v = n - 1 - (self.curr_epoch - q.epoch)
            if v >= n:  # (the reference indexes past `models` here)
                raise ValueError(f"an upload of epoch {q.epoch} at epoch {self.curr_epoch}: no such model version")
            out.append(v if v >= 0 and n == self.stale_size else None)
        return out

    def _kardam_models_loop(self, picked, versions, diff, was_set, decide=None) -> None:
        """``kardam_models``: the fleet_amd.Model with the versions itself. The updater applies the gate of
        :472-474 (_kardam_versions) and `models` lives in a model ledger too (``Model.kardam_ledger``):
        the picked versions are made resident once each and one ``ModelLedger.update`` gives every pick's
        setModel result, so no model text is built and no pick makes a host round trip. Then the loop's
        host part in pick order (:476-480): apply_model, apply, update_lip. ``decide(k)``, when given,
        runs after pick k's part, for every pick (:488)."""
        if self._mledger is None:
            if self.kardam.model_ledger is None:
                self.kardam.model_ledger = self.kardam_models.kardam_ledger(
                    self.kardam.workers, max(1, self.stale_size))
            self._mledger = self.kardam.model_ledger
        m = self._mledger
        ids = {}
        for v in versions:
            if v is not None and v not in ids:
                ids[v] = m.stage_model(self.kardam_models, v)
        _, mdiff, status = m.update([-1 if v is None else ids[v] for v in versions],
                                    [-1 if v is None else q.client_id for q, v in zip(picked, versions)])
        for k, (q, v, md, ms, dn, st) in enumerate(zip(picked, versions, mdiff, status, diff, was_set)):
            if v is not None:
                self.kardam.apply_model(q.client_id, int(ms), float(md))
                if self.kardam.apply(q.client_id, bool(st), float(dn)):
                    self.kardam.update_lip(q.client_id)
            if decide is not None:
                decide(k)
