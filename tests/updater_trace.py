"""A call trace of FleetUpdater: recording fakes of everything the updater touches (codec,
accumulator, pool, gate, ledger, filter, model ledger, host Model, ResidentModel, picker and
Kardam's bookkeeping) and one scenario list that drives every mode of the updater through them.

Each fake method appends ``[object, method, arguments]`` to one list and returns values derived
from its arguments; arrays, bytes and tensors go in as a short digest. ``run_all(module)`` runs
the scenarios on the ``FleetUpdater`` / ``Kardam`` of any ``updater`` module and returns, per
scenario, the trace, what every ``update`` / ``update_many`` returned or raised, and the final
public state. ``tests/golden/make_updater_traces.py`` records that from a reference tree;
``tests/test_updater_trace_cpu.py`` holds the working tree to the record.

The fakes compute nothing, but they keep the contracts the updater relies on: a text that
starts with ``BAD`` is refused wherever the library would refuse a malformed upload (with the
slots at fault on the exception, in the pool's forms), ``REF`` is the gate's wrong-model upload
and ``N<norm>;`` carries the norm the gate reports; setGrad / setModel results follow what each
worker pushed before, so ``Kardam.update_lip`` always finds both of its norms.
"""
import contextlib
import hashlib
import json
import math
import zlib

import numpy as np

import fleet_amd as F
from fleet_amd.layouts import synthetic
from fleet_amd.model import ResidentModel

LAYOUT = synthetic(8)
DEVICE = "trace"  # the fake codec's device: f"cuda:{DEVICE}" is mapped to the CPU while scenarios run


def _sha(b: bytes) -> str:
    return hashlib.sha1(b).hexdigest()[:10]


def dg(x):
    """A JSON value for one argument or result: scalars as they are, data as a digest."""
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, float):
        return x if math.isfinite(x) else repr(x)
    if isinstance(x, np.generic):
        return dg(x.item())
    if isinstance(x, (bytes, bytearray)):
        return "bytes[%d]:%s" % (len(x), _sha(bytes(x)))
    if isinstance(x, np.ndarray):
        return "%s%s:%s" % (x.dtype, list(x.shape), _sha(np.ascontiguousarray(x).tobytes()))
    if hasattr(x, "numel") and hasattr(x, "cpu"):
        return "tensor:%s[%d]:%s" % (str(x.dtype).split(".")[-1], x.numel(), _sha(x.cpu().numpy().tobytes()))
    if isinstance(x, (list, tuple)):
        return [dg(v) for v in x]
    if isinstance(x, dict):
        return {str(k): dg(v) for k, v in x.items()}
    return getattr(x, "name", type(x).__name__)


class Trace:
    def __init__(self):
        self.log = []
        self.filter_norms = []  # per filter update: (norm_p, norm_pdiff) lists, else derived

    def call(self, obj, method, *args, **kw):
        """Records one call; returns a seed for its result."""
        e = [obj, method, dg(args)] + ([dg(kw)] if kw else [])
        self.log.append(e)
        return zlib.crc32(json.dumps(e, sort_keys=True).encode())


def text(seed: int, n: int) -> bytes:
    return (b"%08x" % seed * (n // 8 + 1))[:n]


def vec(seed: int, n: int = 5) -> np.ndarray:
    return ((seed % 997 + np.arange(n)) / 1024).astype(np.float32)


def bad(upload) -> bool:
    return bytes(upload).startswith(b"BAD")


def refuse(uploads, slots=None):
    """Base64Error when one of ``uploads`` is malformed, with ``slots`` at fault where given."""
    at = [k for k, u in enumerate(uploads) if bad(u)]
    if at:
        e = F.Base64Error(F.FLEET_ERR_BASE64, "input is not Base64::encode output")
        if slots is not None:
            e.slots = [slots[k] for k in at]
        raise e


def write(seed, length, mu8, mf32):
    """What a device-form update leaves in the updater's tensors."""
    import torch
    mu8[:length] = torch.from_numpy(np.frombuffer(text(seed, length), np.uint8).copy())
    mf32[:5] = torch.from_numpy(vec(seed))


class TAcc:
    name = "acc"

    def __init__(self, t, length):
        self.t, self.length, self.count = t, length, 0

    def push(self, upload, dampen):
        self.t.call(self.name, "push", upload, dampen)
        refuse([upload])
        self.count += 1

    def push_many(self, uploads, dampens):
        self.t.call(self.name, "push_many", uploads, dampens)
        refuse(uploads)
        self.count += len(uploads)

    def finish(self, want_f32=False):
        s = self.t.call(self.name, "finish", want_f32=want_f32)
        self.count = 0
        return text(s, self.length), vec(s)

    def push_finish(self, uploads, dampens, want_f32=False):
        s = self.t.call(self.name, "push_finish", uploads, dampens, want_f32=want_f32)
        refuse(uploads)
        self.count = 0
        return text(s, self.length), vec(s)

    def finish_device(self, mu8, mf32):
        s = self.t.call(self.name, "finish_device", mu8, mf32)
        self.count = 0
        write(s, self.length, mu8, mf32)

    def close(self):
        self.t.call(self.name, "close")


class TGate:
    name = "gate"

    def __init__(self, t, pool):
        self.t, self.pool = t, pool

    def put(self, slot, upload):
        self.t.call(self.name, "put", slot, upload)
        u = bytes(upload)
        status = 3 if u.startswith(b"REF") else 1 if bad(u) else 0
        norm = float(u[1:u.index(b";")]) if u.startswith(b"N") else float("nan") if status else 1.5
        if status == 0:
            self.pool.rows[slot] = u
        return _Vet(status, norm)


class _Vet:
    def __init__(self, status, norm):
        self.status, self.norm = status, norm


class TPool:
    name = "pool"

    def __init__(self, t, length, slots):
        self.t, self.length, self.slots, self.rows = t, length, slots, {}

    def free_slot(self):
        self.t.call(self.name, "free_slot")
        return next((s for s in range(self.slots) if s not in self.rows), None)

    def put(self, slot, upload):
        self.t.call(self.name, "put", slot, upload)
        self.rows[slot] = bytes(upload)

    def drop(self, slot):
        self.t.call(self.name, "drop", slot)
        del self.rows[slot]

    def _refuse(self, picks):
        refuse([self.rows[s] for s in picks], list(picks))

    def update(self, picks, dampens, want_f32=False):
        s = self.t.call(self.name, "update", picks, dampens, want_f32=want_f32)
        self._refuse(picks)
        return text(s, self.length), vec(s)

    def update_device(self, picks, dampens, mu8, mf32):
        s = self.t.call(self.name, "update_device", picks, dampens, mu8, mf32)
        self._refuse(picks)
        write(s, self.length, mu8, mf32)

    def ledger(self, workers):
        self.t.call(self.name, "ledger", workers)
        return TLedger(self.t, self)

    def gate(self, header_values):
        self.t.call(self.name, "gate", header_values)
        return TGate(self.t, self)


class TLedger:
    name = "ledger"

    def __init__(self, t, pool):
        self.t, self.pool, self.seen = t, pool, {}

    def set_grads(self, seed, workers, epochs):
        """setGrad per pick: true when the worker pushed before in another epoch."""
        diff, was_set = [], []
        for k, (w, ep) in enumerate(zip(workers, epochs)):
            was_set.append(w >= 0 and w in self.seen and self.seen[w] != ep)
            diff.append(1.0 + (seed + k) % 7 if was_set[-1] else float("nan"))
            if w >= 0 and self.seen.get(w) != ep:
                self.seen[w] = ep
        return np.ones(len(workers)), np.array(diff), np.array(was_set)

    def update(self, picks, dampens, workers, epochs, lr, want_f32=False):
        s = self.t.call(self.name, "update", picks, dampens, workers, epochs, lr, want_f32=want_f32)
        self.pool._refuse(picks)
        return (text(s, self.pool.length), vec(s)) + self.set_grads(s, workers, epochs)

    def update_device(self, picks, dampens, workers, epochs, lr, mu8, mf32):
        s = self.t.call(self.name, "update_device", picks, dampens, workers, epochs, lr, mu8, mf32)
        self.pool._refuse(picks)
        write(s, self.pool.length, mu8, mf32)
        return self.set_grads(s, workers, epochs)

    def filter(self, nw, nb, ge):
        self.t.call(self.name, "filter", nw, nb, ge)
        return TFilter(self.t, self)


class TFilter:
    name = "filter"

    def __init__(self, t, ledger):
        self.t, self.ledger, self.pool, self._has_last, self.pending = t, ledger, ledger.pool, False, None

    @property
    def has_last(self):
        self.t.call(self.name, "has_last")
        return self._has_last

    def _norms(self, s):
        return 1.0 + s % 5, 0.25 * (1 + s % 3)

    def set_model(self, weights, biases):
        return self._norms(self.t.call(self.name, "set_model", weights, biases))

    def set_model_device(self, weights, biases):
        return self._norms(self.t.call(self.name, "set_model_device", weights, biases))

    def _update(self, s, picks, workers, epochs):
        self.pool._refuse(picks)
        self.pending = s
        n = len(picks)
        norm_p, norm_pdiff = self.t.filter_norms.pop(0) if self.t.filter_norms else ([1.0] * n, [0.5] * n)
        return self.ledger.set_grads(s, workers, epochs) + (np.array(norm_p, float), np.array(norm_pdiff, float))

    def update(self, picks, dampens, workers, epochs, lr, want_f32=False):
        s = self.t.call(self.name, "update", picks, dampens, workers, epochs, lr, want_f32=want_f32)
        return (text(s, self.pool.length), None) + self._update(s, picks, workers, epochs)

    def update_device(self, picks, dampens, workers, epochs, lr, mu8, mf32):
        s = self.t.call(self.name, "update_device", picks, dampens, workers, epochs, lr, mu8, mf32)
        return self._update(s, picks, workers, epochs)

    def resolve(self, accept, want_f32=False):
        s = self.t.call(self.name, "resolve", accept, want_f32=want_f32)
        if not any(accept):
            return None
        self._has_last = True
        return text(s, self.pool.length), vec(s)

    def resolve_device(self, accept, mu8, mf32):
        s = self.t.call(self.name, "resolve_device", accept, mu8, mf32)
        if any(accept):
            self._has_last = True
            write(s, self.pool.length, mu8, mf32)
        return bool(any(accept))


class TModelLedger:
    name = "mledger"

    def __init__(self, t):
        self.t, self.staged, self.seen = t, [], {}

    def stage_model(self, model, version):
        self.t.call(self.name, "stage_model", model, version)
        self.staged.append(model.first + version)
        return len(self.staged) - 1

    def update(self, ids, workers):
        s = self.t.call(self.name, "update", ids, workers)
        status = []
        for i, w in zip(ids, workers):
            v = self.staged[i] if w >= 0 else None
            status.append(0 if w < 0 else 1 if w not in self.seen else 2 if self.seen[w] == v else 3)
            if w >= 0:
                self.seen[w] = v
        mdiff = [0.5 * (1 + (s + k) % 4) if st == 3 else float("nan") for k, st in enumerate(status)]
        return np.ones(len(ids)), np.array(mdiff), np.array(status)


class _Versions:
    """`models` of a model: ``size`` versions, the oldest with the running number ``first``."""

    def _step(self, stale_size):
        if self.size < max(1, stale_size):
            self.size += 1
        else:
            self.first += 1

    def modelsSize(self):  # noqa: N802
        self.t.call(self.name, "modelsSize")
        return self.size

    def shape(self):
        self.t.call(self.name, "shape")
        return 5, 2, 1, 0

    def kardam_ledger(self, workers, max_versions=None):
        self.t.call(self.name, "kardam_ledger", workers, max_versions)
        return TModelLedger(self.t)


class TModel(_Versions):
    """The host Model a caller holds as ``kardam_models``; the caller steps it."""
    name = "model"

    def __init__(self, t, size):
        self.t, self.size, self.first = t, size, 100

    def export(self, version):
        s = self.t.call(self.name, "export", version)
        return vec(s), vec(s + 1, 2)


class TResident(_Versions, ResidentModel):
    name = "rmodel"

    def __init__(self, t, size):  # (no handle: nothing of ResidentModel's own runs)
        self.t, self.size, self.first, self.epoch, self.lrates, self.lr = t, size, 100, 0, [0.5, 0.25], 1.0

    def initUpdater(self, lrates):  # noqa: N802
        self.t.call(self.name, "initUpdater", lrates)
        self.lrates, self.lr, self.size = list(lrates), lrates[0], 1

    def getLrate(self):  # noqa: N802
        self.t.call(self.name, "getLrate")
        return self.lr

    def descent_device(self, mf32, stale_size, stream=None, n_values=None):
        self.t.call(self.name, "descent_device", mf32, stale_size, n_values=n_values)
        if self.epoch < len(self.lrates):
            self.lr = self.lrates[self.epoch]
        self.epoch += 1
        self._step(stale_size)

    def version_tensors(self, version):
        import torch
        s = self.t.call(self.name, "version_tensors", version)
        return torch.from_numpy(vec(s)), torch.from_numpy(vec(s + 1, 2))


class TCodec:
    name = "codec"
    device = DEVICE

    def __init__(self, t):
        self.t = t

    def accumulator(self, length, header_pos):
        self.t.call(self.name, "accumulator", length, header_pos)
        return TAcc(self.t, length)

    def pool(self, length, header_pos, slots):
        self.t.call(self.name, "pool", length, header_pos, slots)
        return TPool(self.t, length, slots)

    def update(self, uploads, dampen, want_f32=False):
        s = self.t.call(self.name, "update", uploads, dampen, want_f32=want_f32)
        refuse(uploads)
        return text(s, len(uploads[-1])), vec(s)

    def update_device(self, rows, length, dampen, header_pos, mu8, mf32):
        s = self.t.call(self.name, "update_device", rows, length, dampen, header_pos, mu8, mf32)
        self.sticky = bytes(rows.numpy()[:, :3].tobytes())
        write(s, length, mu8, mf32)

    def check(self):
        self.t.call(self.name, "check")
        refuse([self.sticky[k:k + 3] for k in range(0, len(self.sticky), 3)])

    def descent(self, weights, fc_bias, grad, layout, lr):
        self.t.call(self.name, "descent", weights, fc_bias, grad, layout, lr)
        return weights + np.float32(lr) * grad[: len(weights)], fc_bias + np.float32(1)

    def subtractNative(self, a, b):  # noqa: N802
        return text(self.t.call(self.name, "subtractNative", a, b), len(a))

    def getNorm(self, a):  # noqa: N802
        return 1.0 + self.t.call(self.name, "getNorm", a) % 9


class Picker:
    """Plays back (picks, discard) results and records what it was shown."""

    def __init__(self, t, *results):
        self.t, self.results = t, list(results)

    def __call__(self, pending, curr_epoch):
        self.t.call("picker", "call", [(p.client_id, p.slot, p.epoch, p.upload) for p in pending], curr_epoch)
        return self.results.pop(0) if self.results else (None, [])


def recording_kardam(U, t, codec, workers=8, **kw):
    """Kardam with its own bookkeeping, every call the updater makes on it recorded."""
    class K(U.Kardam):
        pass

    def wrap(name):
        def f(self, *a):
            t.call("kardam", name, *a)
            return getattr(U.Kardam, name)(self, *a)
        setattr(K, name, f)
    for name in ("set_model", "apply", "apply_model", "update_lip", "check_byz"):
        wrap(name)
    return K(codec, workers, **kw)


def up(i, n=48, kind=b"u"):
    return (kind + b"%02d;" % i + b"x" * n)[:n]


def labels(i, n=10):
    return [(3 * i + j) % 7 for j in range(n)]


@contextlib.contextmanager
def cpu_tensors():
    """torch.zeros and Tensor.to with the fake codec's device name land on the CPU."""
    import torch
    zeros, to = torch.zeros, torch.Tensor.to
    fix = lambda d: "cpu" if d == f"cuda:{DEVICE}" else d  # noqa: E731
    torch.zeros = lambda *a, device=None, **k: zeros(*a, device=fix(device), **k)
    torch.Tensor.to = lambda self, d, *a, **k: to(self, fix(d), *a, **k)
    try:
        yield
    finally:
        torch.zeros, torch.Tensor.to = zeros, to


class Run:
    """One scenario: an updater over fresh fakes, the calls made on it, the record."""

    def __init__(self, U, seat, M, lrates=(0.05, 0.02), size=2, **kw):
        self.U, self.t, self.seat, self.returns = U, Trace(), seat, []
        self.codec = TCodec(self.t)
        self.resident = TResident(self.t, size) if seat == "resident" else None
        self.host_models = None
        if kw.get("kardam_models") == "host":
            kw["kardam_models"] = self.host_models = TModel(self.t, size)
        elif kw.get("kardam_models") == "same":
            kw["kardam_models"] = self.resident
        if "picker" in kw:
            kw["picker"] = Picker(self.t, *kw["picker"])
        if kw.get("kardam") is True:
            kw["kardam"] = recording_kardam(U, self.t, self.codec)
        elif kw.get("kardam") == "own ledger":  # a model ledger the caller gave Kardam
            kw["kardam"] = recording_kardam(U, self.t, self.codec, model_ledger=TModelLedger(self.t))
        self.kardam = kw.get("kardam")
        w, b = (None, None) if self.resident else (np.arange(5, dtype=np.float32), np.zeros(2, np.float32))
        self.u = U.FleetUpdater(self.codec, LAYOUT, M, list(lrates), w, b, model=self.resident, **kw)

    def _do(self, fn, *a):
        try:
            r = fn(*a)
        except Exception as e:  # the record is the point: type and message
            self.returns.append({"raises": type(e).__name__, "message": str(e), "slots": dg(getattr(e, "slots", None))})
            return
        self.returns.append(dg(r))
        for m in r if isinstance(r, list) else [r]:
            if m is not None and self.host_models is not None:
                self.host_models._step(self.u.stale_size)  # the caller's descentNative

    def update(self, upload, i, epoch, cid=0, n_labels=10):
        self._do(self.u.update, upload, labels(i, n_labels), epoch, cid)

    def update_many(self, arrivals):
        self._do(self.u.update_many, [(u, labels(i), e, cid) for u, i, e, cid in arrivals])

    def record(self):
        u, k = self.u, self.kardam
        state = {"weights": dg(u.weights), "fc_bias": dg(u.fc_bias), "lr": dg(u.lr), "model": dg(u.model),
                 "curr_epoch": u.curr_epoch, "global_labels": dg(u.global_labels),
                 "acc": [[p.client_id, p.epoch, p.slot, dg(p.upload), dg(p.dampen)] for p in u.acc],
                 "last_merged": dg(u.last_merged), "last_accept": dg(u.last_accept), "refused": dg(u.refused)}
        if k is not None:
            state["kardam"] = {"lips": dg(k.lips), "grad_diff_norm": dg(k.grad_diff_norm),
                               "model_diff_norm": dg(k.model_diff_norm), "rejects": k.subsequent_rejects,
                               "ledger": k.ledger is not None and k.ledger is u._ledger,
                               "model_ledger": k.model_ledger is not None and k.model_ledger is u._mledger}
        return {"trace": self.t.log, "returns": self.returns, "state": state}


# ------------------------------------------------------------------ scenarios
# Each takes (U, seat) and returns a Run. M = 3 in the FIFO forms, 2 in the pooled ones; the
# schedule is shorter than the rounds; upload epochs lag the updater's so that getDampen reads
# the label vector (policy 2 with has_outlier: tau > 1.5 * staleSize).

def fifo(U, seat, **kw):
    r = Run(U, seat, 3, size=0, policy=2, has_outlier=True, **kw)
    for i in range(10):
        r.update(up(i), i, max(0, i // 3 - 1), cid=i % 4, n_labels=(10, 12, 7)[i % 3])
    return r


def fifo_codec_replaced(U, seat):
    r = Run(U, seat, 3, policy=1)
    r.u.codec = TCodec(r.t)  # the updater's attributes are read when they are used
    r.u.codec.name, r.u.lrates, r.u.stale_size = "codec2", [0.125, 0.0625], 3
    for i in range(7):
        r.update(up(i), i, 0, cid=i)
    return r


def streaming(U, seat):
    r = Run(U, seat, 3, policy=2, has_outlier=True, streaming=True)
    for i in range(6):
        r.update(up(i), i, max(0, i // 3 - 1), cid=i)
    for i in range(6, 10):  # another upload length from the third batch on
        r.update(up(i, 64), i, 1, cid=i)
    return r


def update_many(U, seat):
    r = Run(U, seat, 3, policy=2, has_outlier=True, streaming=True)
    arr = lambda ids, e, n=48: [(up(i, n), i, e, i) for i in ids]  # noqa: E731
    r.update_many(arr([0, 1], 0))             # leaves the batch open
    r.update_many(arr([2], 0))                # completes it exactly
    r.update_many(arr(range(3, 9), 0))        # two whole batches
    r.update_many(arr(range(9, 13), 1, 64))   # a new length: one batch and one left open
    r.update_many([])
    r.update_many(arr([13, 14, 15], 2, 64))   # spans the open batch and the next
    return r


def update_many_fifo(U, seat):
    r = Run(U, seat, 3, policy=1)
    r.update_many([(up(i), i, 0, i) for i in range(7)])
    return r


def pooled(U, seat):
    picks = [(None, []), ([2, 0], [1]), (None, None), ([1, 0], ()), ([1, 0], []), (None, [0]), ([0, 1], [])]
    r = Run(U, seat, 2, (0.05,), policy=2, has_outlier=True, stale_size=1, picker=picks)
    for i in range(10):
        r.update(up(i), i, 0, cid=i, n_labels=(10, 12, 7)[i % 3])
    return r


def kardam_callback(U, seat):
    picks = [([0, 1], []), ([1, 0], []), ([0, 1], []), (None, []), ([2, 0], [1]), ([1, 0], [])]
    r = Run(U, seat, 2, policy=1, stale_size=2, picker=picks, kardam=True,
            kardam_model=lambda tau: None if tau >= 2 else text(tau + 7 * r.u.curr_epoch, 40))
    for i, (cid, lag) in enumerate([(1, 0), (2, 0), (1, 0), (2, 1), (1, 0), (1, 1), (3, 0), (2, 0), (1, 3), (2, 2),
                                    (3, 0)]):
        r.update(up(i), i, max(0, r.u.curr_epoch - lag), cid=cid)
    return r


def kardam_models(U, seat, models="host", kardam=True):
    picks = [([0, 1], []), ([1, 0], []), ([0, 1], []), (None, []), ([2, 0], [1]), ([1, 0], [])]
    r = Run(U, seat, 2, size=1, policy=1, stale_size=2, picker=picks, kardam=kardam, kardam_models=models)
    for i, (cid, lag) in enumerate([(1, 0), (2, 0), (1, 0), (2, 1), (1, 0), (1, 1), (3, 0), (2, 0), (1, 3), (2, 2),
                                    (3, 0)]):  # size 1: gated; then worker 1 twice; lags 2 and 3 gated out
        r.update(up(i), i, max(0, r.u.curr_epoch - lag), cid=cid)
    return r


def kardam_models_own_ledger(U, seat):
    return kardam_models(U, seat, kardam="own ledger")


def filtered(U, seat, models="host"):
    picks = [([0, 1], [])] * 6
    r = Run(U, seat, 2, policy=1, stale_size=2, picker=picks, kardam=True, kardam_models=models,
            kardam_filter=True)
    big = 1e9
    r.t.filter_norms = [([1, 1], [1, 1]), ([1, 1], [1, 1]), ([1e-9, big], [1e-9, big]), ([big, big], [big, big]),
                        ([1e-9, 1e-9], [1e-9, 1e-9]), ([big, 1e-9], [big, 1e-9])]
    for i in range(12):  # workers 1 and 2 every round: lips from the second on
        r.update(up(i), i, r.u.curr_epoch - (i % 2 if r.u.curr_epoch else 0), cid=1 + i % 2)
    return r


def filtered_below_stale_size(U, seat, models="host"):
    r = Run(U, seat, 2, size=1, policy=1, stale_size=2, picker=[([0, 1], [])] * 2, kardam=True,
            kardam_models=models, kardam_filter=True)
    for i in range(4):  # modelsSize() < staleSize: accepted without checkByz
        r.update(up(i), i, r.u.curr_epoch, cid=1 + i % 2)
    return r


def vet(U, seat, **kw):
    picks = [([1, 0], []), ([0, 1], [])]
    r = Run(U, seat, 2, policy=1, stale_size=1, picker=picks, vet=True, **kw)
    for i, u in enumerate([up(0), up(1, kind=b"REF"), up(2, kind=b"N3.5;"), up(3, kind=b"N99;"), up(4, kind=b"BAD"),
                           up(5, kind=b"Nnan;"), up(6), up(7)]):
        r.update(u, i, 0, cid=i)
    return r


def vet_max_norm(U, seat):
    return vet(U, seat, vet_max_norm=10.0)


def fail_pool_update(U, seat, **kw):
    picks = [([0, 1], []), ([1, 0], []), ([0, 1], [])]
    r = Run(U, seat, 2, policy=1, stale_size=2, picker=picks, **kw)
    for i, u in enumerate([up(0), up(1, kind=b"BAD"), up(2), up(3), up(4)]):
        r.update(u, i, 0, cid=1 + i)
    return r


def fail_ledger_update(U, seat):
    return fail_pool_update(U, seat, kardam=True, kardam_model=lambda tau: text(tau, 40))


def fail_filter_update(U, seat):
    return fail_pool_update(U, seat, kardam=True, kardam_models="same" if seat == "resident" else "host",
                            kardam_filter=True)


def fail_streaming_push(U, seat):
    r = Run(U, seat, 3, policy=1, streaming=True)
    for i, u in enumerate([up(0), up(1, kind=b"BAD"), up(2), up(3), up(4)]):
        r.update(u, i, 0, cid=i)
    return r


def fail_update_many(U, seat):
    r = Run(U, seat, 3, policy=1, streaming=True)
    good = lambda ids: [(up(i), i, 0, i) for i in ids]  # noqa: E731
    r.update_many(good([0]) + [(up(1, kind=b"BAD"), 1, 0, 1)])                      # an open run
    r.update_many(good([2, 3]) + [(up(4, kind=b"BAD"), 4, 0, 4)] + good([5]))       # a run that would complete
    r.update_many(good([6, 7, 8, 9]) + [(up(10, kind=b"BAD"), 10, 0, 10)] + good([11]))  # the runs before stay
    return r


def fail_full_pool(U, seat):
    r = Run(U, seat, 2, policy=1, stale_size=1, picker=[], pool_slots=2)
    for i in range(4):
        r.update(up(i), i, 0, cid=i)
    return r


def fail_picker_contract(U, seat):
    picks = [([0], []), ([0, 0], []), ([0, 5], []), ([-1, 0], []), (None, [9]), (None, [-1]), ([0, 1], [1]),
             ([0, 1, 2], []), ([7, 6], [0, 3])]
    r = Run(U, seat, 2, policy=1, stale_size=1, picker=picks, pool_slots=16)
    for i in range(11):
        r.update(up(i), i, 0, cid=i)
    return r


def fail_unequal_lengths(U, seat):
    r = Run(U, seat, 3, policy=1)
    for i, n in enumerate([48, 64, 48, 48, 48, 48]):
        r.update(up(i, n), i, 0, cid=i)
    return r


def fail_fifo_update(U, seat):
    r = Run(U, seat, 3, policy=2, has_outlier=True)
    for i, u in enumerate([up(0), up(1, kind=b"BAD"), up(2), up(3), up(4), up(5), up(6)]):
        r.update(u, i, 0, cid=i)
    return r


def fail_version_too_new(U, seat):
    r = Run(U, seat, 2, policy=1, stale_size=2, picker=[([0, 1], []), ([0, 2], [1])], kardam=True,
            kardam_models="same" if seat == "resident" else "host")
    for i, e in enumerate([0, 2, 0, 0]):  # (epoch 1 at epoch 0 already fails in getDampen: 1 / (tau + 1))
        r.update(up(i), i, e, cid=i)
    return r


BOTH = [fifo, fifo_codec_replaced, streaming, update_many, update_many_fifo, pooled, kardam_callback, kardam_models, vet, vet_max_norm,
        filtered, filtered_below_stale_size, fail_pool_update, fail_ledger_update, fail_filter_update,
        fail_streaming_push, fail_update_many, fail_full_pool, fail_picker_contract, fail_fifo_update,
        fail_version_too_new, kardam_models_own_ledger]
RESIDENT_ONLY = [fail_unequal_lengths,
                 lambda U, seat: kardam_models(U, seat, "same"), lambda U, seat: filtered(U, seat, "same"),
                 lambda U, seat: filtered_below_stale_size(U, seat, "same")]
RESIDENT_NAMES = ["fail_unequal_lengths", "kardam_models_same", "filtered_same", "filtered_below_stale_size_same"]


def scenarios():
    out = [(f"{f.__name__}/{seat}", f, seat) for f in BOTH for seat in ("host", "resident")]
    return out + [(f"{n}/resident", f, "resident") for n, f in zip(RESIDENT_NAMES, RESIDENT_ONLY)]


def run_all(U, only=None):
    """{scenario: record} of every scenario (or the one named ``only``) on ``U.FleetUpdater`` /
    ``U.Kardam``, as JSON values."""
    with cpu_tensors():
        out = {name: f(U, seat).record() for name, f, seat in scenarios() if only in (None, name)}
    return json.loads(json.dumps(out))
