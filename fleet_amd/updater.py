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


class FleetUpdater:
    """CppNNUpdater.update's aggregation + descentNative's model step.

    ``weights`` (the non-null W concatenated in slot order) and ``fc_bias`` (the
    fully-connected layers' biases) are the model the server keeps
    (``cnn`` in cppNN_backend.cpp); ``lrates`` is initUpdater's schedule
    (cppNN_backend.cpp:161-172). With ``model=`` (a ``fleet_amd.ResidentModel``) the model lives in
    HBM instead: ``weights`` and ``fc_bias`` may be None, every path runs the device form of its
    update into tensors the updater keeps and steps the model there (``descent_device``), and
    only the merged text comes back to the host. ``kardam_models=`` may be that same model.
    The model steps under the solver it was made with (``ResidentModel(..., solver=)``); the
    ``weights=`` / ``fc_bias=`` path keeps no solver state and is always sgd."""

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
        self.codec = codec
        self.layout = layout
        self.M = M
        self.policy = policy
        self.alpha = alpha
        self.stale_size = stale_size
        self.has_outlier = has_outlier
        self.lrates = [float(v) for v in lrates]
        self.lr = np.float32(self.lrates[0])  # initUpdater: cnn.set_learning_rate(lrates_vec[0])
        # model: a fleet_amd.ResidentModel. The model step then is its descent_device on the merged
        # gradient where the update left it (tensors the updater keeps); only the merged text
        # comes back to the host, for the return value. weights / fc_bias are not used.
        self.model = model
        self.weights = None if model is not None else np.array(weights, dtype=np.float32, copy=True)
        self.fc_bias = None if model is not None else np.array(fc_bias, dtype=np.float32, copy=True)
        self._merged_u8 = self._merged_f32 = None
        if model is not None and model.modelsSize() == 0:
            model.initUpdater(self.lrates)
        self.curr_epoch = 0
        self.acc: List[Pending] = []
        self.global_labels = [0] * num_labels
        self.last_merged: Optional[bytes] = None
        # streaming: every upload is folded into a resident sum when it arrives
        # (Codec.accumulator), so the M-th call is left with one push, the finish and the
        # model step. With staleSize == 0 picking order is arrival order (:409, :421) and
        # getDampen reads only curr_epoch and global_labels, which change inside the M-th
        # call alone (:502-504, descentNative): the factor computed at arrival is the one
        # the loop below computes for that pick.
        self.streaming = bool(streaming)
        self._stream_acc = None
        # picker: the staleSize > 0 branch (:394-407). ``picker(pending, curr_epoch)`` stands
        # where staleSim.stalenessSim stands: called at every arrival once M uploads are
        # buffered, it returns ``(picks, discard)`` -- ``picks`` None when no update is
        # possible yet (:405-406), else M distinct indices into ``pending`` in pick order;
        # ``discard`` the indices of buffered uploads to drop unpicked (the simulator's
        # too-old gradients, which it removes whether or not it picks). The uploads wait in
        # a pool of ``pool_slots`` slots in HBM and the update folds the picked slots there.
        self.picker = picker
        self.pool_slots = 4 * M if pool_slots is None else int(pool_slots)
        self._pool = None
        # kardam: Kardam's bookkeeping of the picked uploads (:470-484), opt-in. ``kardam`` is a
        # :class:`Kardam`; its `grads` then live in a ledger beside the pool (``Pool.ledger``),
        # and one ``Ledger.update`` gives the merged bytes and every pick's setGrad result.
        # ``kardam_model(tau)`` stands where getModelParametersNative(modelsSize()-1-tau) and
        # the modelsSize() == staleSize gate stand (:472-474): the picked model's text, or
        # None when Kardam does not run for that pick (:483-484). The caller holds the
        # fleet_amd.Model with the versions.
        # ``kardam_models`` instead: the fleet_amd.Model with the versions itself. The updater then
        # applies the gate of :472-474 (v = modelsSize()-1-tau >= 0 and modelsSize() == staleSize)
        # and `models` lives in a model ledger too (``Model.kardam_ledger``): the picked versions
        # are made resident once each and one ``ModelLedger.update`` gives every pick's setModel
        # result, so no model text is built and no pick makes a host round trip.
        self.kardam = kardam
        self.kardam_model = kardam_model
        self.kardam_models = kardam_models
        self._ledger = None
        self._mledger = None
        # kardam_filter: the filter CppNNUpdater bypasses (`true ||`, :488). An update then asks a
        # fleet_amd.KardamFilter for every pick's checkByz norms in the pass that folds the picks,
        # decides per pick in the Kardam loop (modelsSize() < staleSize or Kardam.check_byz) and
        # resolves: the average is over the accepted picks, and an update none of whose picks was
        # accepted has no average -- no model step, the epoch stays, update returns None (:506).
        self.kardam_filter = bool(kardam_filter)
        self._filter = None
        self.last_accept: Optional[List[bool]] = None
        # vet: an arrival goes into the pool through an arrival gate (``Pool.gate`` with the
        # layout's header codes, ``Gate.put``) instead of ``Pool.put``. An upload that is not
        # Base64::encode output, or whose header slots are not this model's, is refused on the
        # request that brought it: it never joins `acc`, does not count toward M, and update
        # returns None for it, as for the reference's hash mismatch (:350-353). With
        # ``vet_max_norm`` an upload whose flat gradient's norm (new
        # ByteVec(getFlatGradient(g)).getNorm()) exceeds it is refused too, its slot dropped.
        # ``refused`` lists (client_id, status, norm) of every refused arrival. Without vet the
        # updater makes the calls it made before.
        self.vet = bool(vet)
        self.vet_max_norm = None if vet_max_norm is None else float(vet_max_norm)
        self._gate = None
        self.refused: List[tuple] = []

    def _dampen_of(self, p: "Pending") -> float:
        """getDampen for one pick (:463-464) from the current epoch and label vector."""
        tau = self.curr_epoch - p.epoch
        sim = similarity(p.labels, self.global_labels)
        return get_dampen(self.policy, tau, sim, self.stale_size, self.alpha, self.has_outlier)

    def _push(self, p: "Pending") -> None:
        a = self._stream_acc
        if a is None or (a.length != len(p.upload) and a.count == 0):
            if a is not None:
                a.close()
            a = self._stream_acc = self.codec.accumulator(len(p.upload), self.layout.header_positions())
        p.dampen = self._dampen_of(p)
        a.push(p.upload, p.dampen)  # a malformed upload raises here and joins nothing
        p.upload = b""

    def _device_out(self, length: int):
        """The tensors a device-form update writes: the merged text and decodeFloat of it."""
        import torch
        from ._capi import b64_count
        groups = (b64_count(length) + 2) // 3
        if self._merged_u8 is None or self._merged_u8.numel() < 16 * groups + 16:
            dev = f"cuda:{self.codec.device}"
            self._merged_u8 = torch.zeros(16 * groups + 16, dtype=torch.uint8, device=dev)
            self._merged_f32 = torch.zeros(3 * groups + 4, dtype=torch.float32, device=dev)
        return self._merged_u8, self._merged_f32

    def _step_resident(self, length: int) -> bytes:
        """descentNative on the resident model from the merged gradient in HBM; the merged text
        is the one thing copied to the host."""
        from ._capi import b64_count
        self.model.descent_device(self._merged_f32, self.stale_size, n_values=b64_count(length))
        self.lr = np.float32(self.model.getLrate())
        return self._merged_u8[:length].cpu().numpy().tobytes()

    def update(self, upload: bytes, labels: Sequence[int], epoch: int, client_id: int = 0) -> Optional[bytes]:
        """One client upload (CppNNUpdater.update, :330-518). Returns the merged
        gradient when this upload completed a batch of M (and the model stepped),
        else None."""
        p = Pending(bytes(upload), list(labels), int(epoch), int(client_id))
        if self.picker is not None:
            return self._update_pooled(p)
        if self.streaming:
            self._push(p)
        self.acc.append(p)
        if len(self.acc) < self.M:  # M-softsync (:388-391)
            return None
        return self._finish_batch()

    def _update_pooled(self, p: "Pending") -> Optional[bytes]:
        """One arrival with a picker (:383-411, then :420-516 over the picked uploads)."""
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
                return None
        else:
            pool.put(slot, p.upload)
        p.slot, p.upload = slot, b""
        self.acc.append(p)
        if len(self.acc) < self.M:  # M-softsync (:388-391)
            return None
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
            pool.drop(self.acc.pop(i).slot)
        if picked is None:  # not possible to update with the buffered uploads (:405-406)
            return None
        dampen = [self._dampen_of(q) for q in picked]  # tau from the epoch at pick time (:427)
        kd = None
        versions = None
        if self.kardam is not None and self.kardam_models is not None:
            versions = self._kardam_versions(picked)  # before anything changes
        if self.kardam_filter:
            return self._update_filtered(pool, picked, dampen, versions)
        try:
            if self.model is not None:
                mu8, mf32 = self._device_out(pool.length)
            if self.kardam is None and self.model is not None:
                pool.update_device([q.slot for q in picked], dampen, mu8, mf32)
            elif self.kardam is None:
                merged, grad = pool.update([q.slot for q in picked], dampen, want_f32=True)
            else:
                if self._ledger is None:
                    self._ledger = self.kardam.ledger = pool.ledger(self.kardam.workers)
                models = versions if versions is not None else [
                    self.kardam_model(self.curr_epoch - q.epoch) for q in picked]
                workers = [-1 if m is None else q.client_id for q, m in zip(picked, models)]
                # getLrate() before descentNative (:478): the rate of the previous step
                if self.model is not None:
                    _, diff, was_set = self._ledger.update_device(
                        [q.slot for q in picked], dampen, workers, [q.epoch for q in picked],
                        float(self.model.getLrate()), mu8, mf32)
                else:
                    merged, grad, _, diff, was_set = self._ledger.update(
                        [q.slot for q in picked], dampen, workers, [q.epoch for q in picked], float(self.lr),
                        want_f32=True)
                kd = (models, diff, was_set)
        except Exception as e:
            self._drop_at_fault(pool, e)
            raise
        if kd is not None and versions is not None:
            self._kardam_models_loop(picked, *kd)
        elif kd is not None:  # the loop's order (:476-480): a worker picked twice gets the reference's lips
            for q, m, dn, st in zip(picked, *kd):
                if m is None:
                    continue
                self.kardam.set_model(q.client_id, m)
                if self.kardam.apply(q.client_id, bool(st), float(dn)):
                    self.kardam.update_lip(q.client_id)
        window = [0] * len(self.global_labels)
        for q in picked:
            for j, v in enumerate(q.labels[: len(window)]):
                window[j] += v
        for j, v in enumerate(window):
            self.global_labels[j] += v
        if self.model is not None:
            merged = self._step_resident(pool.length)
        else:
            if self.curr_epoch < len(self.lrates):
                self.lr = np.float32(self.lrates[self.curr_epoch])
            self.weights, self.fc_bias = self.codec.descent(self.weights, self.fc_bias, grad, self.layout, self.lr)
        self.curr_epoch += 1
        for q in picked:  # the picked uploads leave `acc` (:421), everything else stays buffered
            pool.drop(q.slot)
        gone = {q.slot for q in picked}
        self.acc = [q for q in self.acc if q.slot not in gone]
        self.last_merged = merged
        return merged

    def _drop_at_fault(self, pool, e) -> None:
        """Base64Error / LayoutError of an update: the slots at fault leave, the model stays."""
        bad = set(getattr(e, "slots", ()))
        for q in self.acc:
            if q.slot in bad:
                pool.drop(q.slot)
        self.acc = [q for q in self.acc if q.slot not in bad]

    def _update_filtered(self, pool, picked, dampen, versions) -> Optional[bytes]:
        """The update over the picked uploads with Kardam's filter (:417-516, :488 without its
        `true ||`): currModel's norms, one KardamFilter.update for every pick's norms and the
        optimistic result, the Kardam loop with the decision after each pick's updateLip, the
        resolve over what was accepted."""
        from .model import ResidentModel
        km = self.kardam_models
        n_models = km.modelsSize()
        if self._ledger is None:
            self._ledger = self.kardam.ledger = pool.ledger(self.kardam.workers)
        if self._filter is None:
            nw, nb, ge, _ = km.shape()
            self._filter = self._ledger.filter(nw, nb, ge)
        f = self._filter
        slots, epochs = [q.slot for q in picked], [q.epoch for q in picked]
        workers = [-1 if v is None else q.client_id for q, v in zip(picked, versions)]
        try:
            if isinstance(km, ResidentModel):  # currModel (:417)
                norm_model, norm_model_diff = f.set_model_device(*km.version_tensors(n_models - 1))
            else:
                norm_model, norm_model_diff = f.set_model(*km.export(n_models - 1))
            has_last = f.has_last
            if self.model is not None:
                mu8, mf32 = self._device_out(pool.length)
                _, diff, was_set, norm_p, norm_pdiff = f.update_device(
                    slots, dampen, workers, epochs, float(self.model.getLrate()), mu8, mf32)
            else:
                _, _, _, diff, was_set, norm_p, norm_pdiff = f.update(slots, dampen, workers, epochs, float(self.lr))
        except Exception as e:
            self._drop_at_fault(pool, e)
            raise
        accept: List[bool] = []

        def decide(k: int) -> None:  # :488
            accept.append(n_models < self.stale_size or self.kardam.check_byz(
                picked[k].client_id, float(norm_p[k]), float(norm_pdiff[k]), norm_model, norm_model_diff, has_last))
        self._kardam_models_loop(picked, versions, diff, was_set, decide)
        self.last_accept = list(accept)
        window = [0] * len(self.global_labels)
        for q in picked:
            for j, v in enumerate(q.labels[: len(window)]):
                window[j] += v
        for j, v in enumerate(window):
            self.global_labels[j] += v
        merged = None
        if self.model is not None:
            if f.resolve_device(accept, mu8, mf32):
                merged = self._step_resident(pool.length)
        else:
            r = f.resolve(accept, want_f32=True)
            if r is not None:
                merged, grad = r
                if self.curr_epoch < len(self.lrates):
                    self.lr = np.float32(self.lrates[self.curr_epoch])
                self.weights, self.fc_bias = self.codec.descent(self.weights, self.fc_bias, grad, self.layout, self.lr)
        if merged is not None:  # avg != null (:506-512)
            self.curr_epoch += 1
            self.last_merged = merged
        for q in picked:  # the picked uploads leave `acc` whatever was decided (:421, :516)
            pool.drop(q.slot)
        gone = {q.slot for q in picked}
        self.acc = [q for q in self.acc if q.slot not in gone]
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
        """setModel for every pick from one model-ledger update, then the loop's host part in
        pick order (:476-480): apply_model, apply, update_lip. ``decide(k)``, when given, runs
        after pick k's part, for every pick (:488)."""
        m = self._mledger
        if m is None:
            m = self.kardam.model_ledger
            if m is None:
                m = self.kardam.model_ledger = self.kardam_models.kardam_ledger(self.kardam.workers,
                                                                                max(1, self.stale_size))
            self._mledger = m
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

    def _finish_batch(self, fused=None) -> bytes:
        """The M-th call's part after the arrival (:420-421, :463-464, :490-516): picks the
        batch, merges it (``fused``: the (merged, grad) a push_finish already produced) and
        steps the model."""
        picked, dampen = [], []
        window = [0] * len(self.global_labels)
        for _ in range(self.M):  # FIFO (:420-421)
            p = self.acc.pop(0)
            picked.append(p.upload)
            dampen.append(self._dampen_of(p) if p.dampen is None else p.dampen)
            for j, v in enumerate(p.labels[: len(window)]):
                window[j] += v
        for j, v in enumerate(window):
            self.global_labels[j] += v
        if self.model is not None:
            return self._finish_resident(picked, dampen)
        if fused is not None:
            merged, grad = fused
        elif self.streaming:
            merged, grad = self._stream_acc.finish(want_f32=True)
        else:
            merged, grad = self.codec.update(picked, dampen, want_f32=True)
        # descentNative (cppNN_backend.cpp:329-353): lr from the schedule, then the model step
        if self.curr_epoch < len(self.lrates):
            self.lr = np.float32(self.lrates[self.curr_epoch])
        self.weights, self.fc_bias = self.codec.descent(self.weights, self.fc_bias, grad, self.layout, self.lr)
        self.curr_epoch += 1
        self.acc.clear()  # aggregated.clear() (:516)
        self.last_merged = merged
        return merged

    def _finish_resident(self, picked, dampen) -> bytes:
        """_finish_batch's merge and step with a resident model: the accumulator's finish_device,
        or update_device over the batch's uploads, then the step in HBM."""
        if self.streaming:
            length = self._stream_acc.length
            mu8, mf32 = self._device_out(length)
            self._stream_acc.finish_device(mu8, mf32)
        else:
            import torch
            length = len(picked[0])
            if any(len(u) != length for u in picked):
                raise ValueError("the batch's uploads differ in length (one model layout)")
            mu8, mf32 = self._device_out(length)
            pitch = (length + 15) // 16 * 16 + 16
            rows = np.zeros((len(picked), pitch), np.uint8)
            for i, u in enumerate(picked):
                rows[i, :length] = np.frombuffer(u, np.uint8)
            d_rows = torch.from_numpy(rows).to(f"cuda:{self.codec.device}")
            self.codec.update_device(d_rows, length, dampen, self.layout.header_positions(), mu8, mf32)
            self.codec.check()  # a malformed upload raises before the model steps
        merged = self._step_resident(length)
        self.curr_epoch += 1
        self.acc.clear()  # aggregated.clear() (:516)
        self.last_merged = merged
        return merged

    def update_many(self, arrivals) -> List[Optional[bytes]]:
        """Several uploads that are at hand together: ``arrivals`` is a list of ``(upload,
        labels, epoch, client_id)``, the result the list of what ``update`` returns for each
        in turn. With ``streaming=True`` the list is cut at batch boundaries and each run is
        folded by one call: ``push_many`` for a run that leaves the batch open,
        ``push_finish`` (the fold and the merged gradient from one kernel) followed by the
        model step for a run that completes it. The factors are computed at arrival, as
        ``update`` does; ``_dampen_of`` reads ``curr_epoch`` and ``global_labels``, which the
        model step changes, so a run's factors are computed after the previous run's step.
        A run is all or nothing: a malformed upload raises and none of its run joins the
        batch (the runs before it stay)."""
        arrivals = list(arrivals)
        if not self.streaming:
            return [self.update(*a) for a in arrivals]
        out: List[Optional[bytes]] = []
        i = 0
        while i < len(arrivals):
            room = self.M - len(self.acc)
            run = [Pending(bytes(u), list(l), int(e), int(cid)) for u, l, e, cid in arrivals[i: i + room]]
            i += len(run)
            a = self._stream_acc
            if a is None or (a.length != len(run[0].upload) and a.count == 0):
                if a is not None:
                    a.close()
                a = self._stream_acc = self.codec.accumulator(len(run[0].upload), self.layout.header_positions())
            for p in run:
                p.dampen = self._dampen_of(p)
            ups, d = [p.upload for p in run], [p.dampen for p in run]
            fused = None
            if len(run) == room and self.model is None:
                fused = a.push_finish(ups, d, want_f32=True)
            else:  # (a resident model: the finish is the device form's, in _finish_batch)
                a.push_many(ups, d)
            for p in run:
                p.upload = b""
            self.acc.extend(run)
            out += [None] * (len(run) - 1)
            out.append(self._finish_batch(fused) if len(run) == room else None)
        return out
