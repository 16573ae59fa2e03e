"""The Kardam ledger without a GPU: the C-ABI's fleet_kledger_* symbols and their argument
checks, and FleetUpdater's Kardam mode (CppNNUpdater.java:470-484 over the picks of the
staleSize > 0 branch) against a recording fake codec, pool and ledger."""
import ctypes as C

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import synthetic
from fleet_amd.updater import FleetUpdater, Kardam
from test_pool_cpu import POOL, FakeCodec, FakePool, Script, labels, upload

LEDGER = ["fleet_kledger_create", "fleet_kledger_destroy", "fleet_kledger_workers", "fleet_kledger_has",
          "fleet_kledger_epoch", "fleet_kledger_forget", "fleet_kledger_read", "fleet_kledger_update",
          "fleet_kledger_update_device"]


def test_header_declares_and_library_exports_the_ledger_entry_points():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in LEDGER:
        assert s in declared, s
        assert hasattr(L, s), s
    assert sorted(s for s in declared if s.startswith("fleet_kledger_")) == sorted(LEDGER)
    assert sorted(s for s in declared if s.startswith("fleet_pool_")) == sorted(POOL)  # no new pool name
    assert hasattr(F, "Ledger") and hasattr(F.Pool, "ledger")
    for m in ("update", "update_device", "has", "epoch", "forget", "read", "close", "__enter__", "__exit__"):
        assert hasattr(F.Ledger, m), m


def test_null_and_absent_arguments():
    L = F.lib()
    buf = np.full(64, 0x5A, np.uint8)
    picks = np.array([0, 1], np.int32)
    wk = np.array([0, 1], np.int32)
    ep = np.array([3, 4], np.int32)
    d = np.ones(2, np.float64)
    ng = np.full(2, 7.0)
    nd = np.full(2, 7.0)
    st = np.full(2, 9, np.uint8)
    gbuf = np.full(8, 5.0, np.float32)
    n = C.c_size_t(0)
    e = C.c_int(77)
    h = C.c_void_p(0x1234)
    fake = C.c_void_p(0x10)  # a ledger argument that is never dereferenced: a NULL beside it is found first
    pk, dp, w, epp, out = picks.ctypes.data, d.ctypes.data, wk.ctypes.data, ep.ctypes.data, buf.ctypes.data
    g, dn, s = ng.ctypes.data, nd.ctypes.data, st.ctypes.data
    assert L.fleet_kledger_create(None, 4, 2, C.byref(h)) == F.FLEET_ERR_ARG
    assert h.value == 0x1234
    assert L.fleet_kledger_create(None, 4, 2, None) == F.FLEET_ERR_ARG
    assert L.fleet_kledger_destroy(None) is None
    assert L.fleet_kledger_workers(None) == F.FLEET_ERR_ARG
    assert L.fleet_kledger_has(None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_kledger_epoch(None, 0, C.byref(e)) == F.FLEET_ERR_ARG
    assert L.fleet_kledger_epoch(fake, 0, None) == F.FLEET_ERR_ARG
    assert L.fleet_kledger_forget(None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_kledger_read(None, 0, gbuf.ctypes.data, 8) == F.FLEET_ERR_ARG
    assert L.fleet_kledger_read(fake, 0, None, 8) == F.FLEET_ERR_ARG
    lr = 0.05
    assert L.fleet_kledger_update(None, pk, 2, dp, w, epp, lr, out, 64, C.byref(n), None, g, dn, s) == F.FLEET_ERR_ARG
    assert L.fleet_kledger_update_device(None, pk, 2, dp, w, epp, lr, out, None, g, dn, s, None) == F.FLEET_ERR_ARG
    # each absent argument in turn, beside a ledger that is never looked at
    host = [pk, 2, dp, w, epp, lr, out, 64, C.byref(n), None, g, dn, s]
    for i in (0, 2, 3, 4, 6, 10, 11, 12):
        a = list(host)
        a[i] = None
        assert L.fleet_kledger_update(fake, *a) == F.FLEET_ERR_ARG, i
    dev = [pk, 2, dp, w, epp, lr, out, None, g, dn, s, None]
    for i in (0, 2, 3, 4, 6, 8, 9, 10):
        a = list(dev)
        a[i] = None
        assert L.fleet_kledger_update_device(fake, *a) == F.FLEET_ERR_ARG, i
    for K in (0, -1):
        host[1] = dev[1] = K
        assert L.fleet_kledger_update(fake, *host) == F.FLEET_ERR_ARG
        assert L.fleet_kledger_update_device(fake, *dev) == F.FLEET_ERR_ARG
    assert n.value == 0 and e.value == 77
    assert (buf == 0x5A).all() and (ng == 7.0).all() and (nd == 7.0).all() and (st == 9).all() and (gbuf == 5.0).all()


# ------------------------------------------------------------------ FleetUpdater

class FakeLedger:
    """Plays Kardam.setGrad (Kardam.java:56-71) on (worker, epoch) alone and records the call;
    the difference norm of a set pick is 100 * update number + pick index."""

    def __init__(self, log, workers, max_store):
        self.log, self.workers, self.max_store = log, workers, max_store
        self.grads = {}
        self.updates = 0

    def update(self, picks, dampens, workers, epochs, lr, want_f32=False):
        assert want_f32
        self.log.append(("ledger.update", [int(s) for s in picks], [float(x) for x in dampens], [int(w) for w in workers],
                         [int(e) for e in epochs], float(lr)))
        self.updates += 1
        pool = self.pool
        if pool.fail is not None:
            exc, slots = pool.fail
            pool.fail = None
            e = exc(F.FLEET_ERR_BASE64, "slot: input is not Base64::encode output")
            e.slots = list(slots)
            raise e
        K = len(picks)
        ng, nd, st = np.full(K, 1.0), np.full(K, np.nan), np.zeros(K, bool)
        for k, (w, ep) in enumerate(zip(workers, epochs)):
            if w < 0:
                ng[k] = np.nan
            elif w in self.grads and self.grads[w] != ep:
                st[k], nd[k] = True, 100.0 * self.updates + k
                self.grads[w] = ep
            elif w not in self.grads:
                self.grads[w] = ep
        return b"L%d" % self.updates, np.zeros(8, np.float32), ng, nd, st


class LedgerPool(FakePool):
    def ledger(self, workers, max_store=None):
        self.log.append(("ledger", workers))
        led = FakeLedger(self.log, workers, max_store)
        led.pool = self
        self.ledgers = getattr(self, "ledgers", []) + [led]
        return led


class LedgerCodec(FakeCodec):
    def pool(self, length, header_pos, slots, group_begin=0, group_end=None):
        self.pools.append(LedgerPool(self.log, length, header_pos, slots))
        return self.pools[-1]


class RecordingKardam(Kardam):
    """The real bookkeeping with its calls recorded and the model-difference norm taken from
    the fake texts (b"m<version>"), so no codec is asked."""

    def __init__(self, log, workers):
        super().__init__(None, workers)
        self.log = log

    def set_model(self, worker, model_text):
        self.log.append(("set_model", worker, model_text))
        if worker in self.models:
            norm = abs(float(model_text[1:]) - float(self.models[worker][1:]))
            if norm == 0:
                return
            self.model_diff_norm[worker] = norm
        self.models[worker] = model_text

    def apply(self, worker, set_flag, norm_diff):
        self.log.append(("apply", worker, bool(set_flag), None if norm_diff != norm_diff else float(norm_diff)))
        return super().apply(worker, set_flag, norm_diff)

    def update_lip(self, worker):
        self.log.append(("update_lip", worker))
        super().update_lip(worker)


def make(codec, picker, kardam, kardam_model, M=3, **kw):
    kw.setdefault("policy", 1)
    kw.setdefault("stale_size", 2)
    return FleetUpdater(codec, synthetic(8), M, [0.05, 0.02, 0.01], np.zeros(5, np.float32), np.zeros(0, np.float32),
                        picker=picker, kardam=kardam, kardam_model=kardam_model, **kw)


def state(k):
    return (dict(k.models), dict(k.model_diff_norm), dict(k.grad_diff_norm), {w: list(v) for w, v in k.lips.items()})


def test_constructor_rules():
    mk = lambda **kw: FleetUpdater(LedgerCodec(), synthetic(8), 3, [0.05], np.zeros(5, np.float32),
                                   np.zeros(0, np.float32), **kw)
    k = Kardam(None, 4)
    with pytest.raises(ValueError):
        mk(kardam=k, kardam_model=lambda tau: None)  # no picker
    with pytest.raises(ValueError):
        mk(kardam=k, kardam_model=lambda tau: None, streaming=True)
    with pytest.raises(ValueError):
        mk(kardam=k, picker=lambda p, e: (None, []))  # no kardam_model
    u = mk(kardam=k, kardam_model=lambda tau: None, picker=lambda p, e: (None, []))
    assert u.kardam is k and k.ledger is None  # the ledger comes with the pool, at the first update
    assert mk(picker=lambda p, e: (None, [])).kardam is None
    assert Kardam(None, 4, ledger="L").ledger == "L"


def test_the_ledger_gets_workers_epochs_and_the_rate_and_kardam_runs_in_loop_order():
    c = LedgerCodec()
    pk = Script(([2, 0, 1], []), ([0, 2, 1], []), ([1, 0, 2], []))
    asked = []

    def kardam_model(tau):
        asked.append(tau)
        return None if tau > 1 else b"m%d" % (10 - tau + len(asked))  # a new version each time

    k = RecordingKardam(c.log, 6)
    u = make(c, pk, k, kardam_model)
    # update 1 at epoch 0: all three workers new, every model available
    for i in range(3):
        r = u.update(upload(i), labels(i), 0, i)
    assert r == b"L1" and u.last_merged == b"L1" and k.ledger is c.pools[0].ledgers[0]
    assert [e for e in c.log if e[0] == "ledger"] == [("ledger", 6)]
    call = [e for e in c.log if e[0] == "ledger.update"][0]
    assert call[1] == [2, 0, 1] and call[2] == [1.0, 1.0, 1.0]
    assert call[3] == [2, 0, 1] and call[4] == [0, 0, 0]
    assert call[5] == float(np.float32(0.05))  # getLrate() before descentNative: the initial rate
    assert asked == [0, 0, 0]
    i0 = c.log.index(call)
    assert [e[:2] for e in c.log[i0 + 1: i0 + 7]] == [("set_model", 2), ("apply", 2), ("set_model", 0), ("apply", 0),
                                                     ("set_model", 1), ("apply", 1)]
    assert c.log[i0 + 7] == ("descent", float(np.float32(0.05)))  # Kardam's loop runs before the model step
    assert not any(e[0] == "update" for e in c.log)  # one Ledger.update stands for pool.update
    assert k.grad_diff_norm == {} and k.lips == {} and sorted(k.models) == [0, 1, 2]
    # update 2 at epoch 1: worker 0 again at epoch 1 (set), worker 1 at the old epoch 0 (ignored),
    # worker 3 with an upload of epoch -1: tau = 2, no model, so Kardam does not run for it
    del asked[:]
    u.update(upload(3), labels(3), 1, 0)
    u.update(upload(4), labels(4), 0, 1)
    n0 = len(c.log)
    assert u.update(upload(5), labels(5), -1, 3) == b"L2"
    call = [e for e in c.log[n0:] if e[0] == "ledger.update"][0]
    assert call[1] == [0, 2, 1] and call[3] == [0, -1, 1] and call[4] == [1, -1, 0]
    assert call[2] == [1.0, 1 / 3, 0.5]
    assert call[5] == float(np.float32(0.05))  # the rate descentNative set in update 1 (lrates[0])
    assert asked == [0, 2, 1]
    i0 = c.log.index(call)
    ev = c.log[i0 + 1: c.log.index(("descent", float(np.float32(0.02))))]
    assert [e[:2] for e in ev] == [("set_model", 0), ("apply", 0), ("update_lip", 0), ("set_model", 1), ("apply", 1)]
    assert ev[1] == ("apply", 0, True, 200.0) and ev[4] == ("apply", 1, False, None)
    assert k.grad_diff_norm == {0: 200.0} and list(k.lips) == [0] and len(k.lips[0]) == 1
    assert k.lips[0][0] == 200.0 / k.model_diff_norm[0]
    assert 3 not in k.models


def test_a_worker_twice_in_one_update():
    c = LedgerCodec()
    pk = Script(([0, 1, 2], []), ([0, 1, 2], []))
    ver = iter(range(1, 100))
    k = RecordingKardam(c.log, 4)
    u = make(c, pk, k, lambda tau: b"m%d" % next(ver))
    for i, (cid, ep) in enumerate([(1, 0), (2, 0), (3, 0)]):
        u.update(upload(i), labels(i), ep, cid)
    n0 = len(c.log)
    # worker 1 twice: epochs 1 and 0 (each other than the one before it), worker 2 once at the same epoch
    for i, (cid, ep) in enumerate([(1, 1), (2, 0), (1, 0)]):
        r = u.update(upload(3 + i), labels(i), ep, cid)
    assert r == b"L2"
    call = [e for e in c.log[n0:] if e[0] == "ledger.update"][0]
    assert call[3] == [1, 2, 1] and call[4] == [1, 0, 0]
    ev = [e for e in c.log[c.log.index(call) + 1:] if e[0] in ("set_model", "apply", "update_lip")]
    assert [e[:2] for e in ev] == [("set_model", 1), ("apply", 1), ("update_lip", 1), ("set_model", 2), ("apply", 2),
                                   ("set_model", 1), ("apply", 1), ("update_lip", 1)]
    assert ev[1][2:] == (True, 200.0) and ev[4][2:] == (False, None) and ev[6][2:] == (True, 202.0)
    # models m1..m3 in update 1, m4 (worker 1), m5 (worker 2), m6 (worker 1): differences 3 and 2
    assert k.lips == {1: [200.0 / 3.0, 202.0 / 2.0]}
    assert k.grad_diff_norm == {1: 202.0}


def test_no_kardam_change_when_the_update_raises():
    c = LedgerCodec()
    pk = Script(([0, 1, 2], []), ([0, 1, 2], []), ([0, 1, 2], []))
    ver = iter(range(1, 100))
    k = RecordingKardam(c.log, 8)
    u = make(c, pk, k, lambda tau: b"m%d" % next(ver))
    for i in range(3):
        u.update(upload(i), labels(i), 0, i)
    before = state(k)
    w0, g0, ep0 = u.weights.copy(), list(u.global_labels), u.curr_epoch
    u.update(upload(3), labels(3), 1, 0)
    u.update(upload(4), labels(4), 1, 1)
    c.pools[0].fail = (F.Base64Error, [1])
    n0 = len(c.log)
    with pytest.raises(F.Base64Error) as ei:
        u.update(upload(5), labels(5), 1, 2)
    assert ei.value.slots == [1]
    assert state(k) == before
    assert [e[0] for e in c.log[n0:]] == ["put", "ledger.update", "drop"] and c.log[-1] == ("drop", 1)
    assert np.array_equal(u.weights, w0) and u.global_labels == g0 and u.curr_epoch == ep0
    assert [(p.client_id, p.slot) for p in u.acc] == [(0, 0), (2, 2)]  # the pool behaviour is the plain mode's
    # the next arrival completes a batch again and Kardam goes on from the unchanged state
    assert u.update(upload(6), labels(6), 1, 1) == b"L3"
    assert sorted(k.grad_diff_norm) == [0, 1, 2]


def test_kardam_none_never_touches_a_ledger():
    c = LedgerCodec()
    pk = Script(([0, 1, 2], []))
    u = FleetUpdater(c, synthetic(8), 3, [0.05], np.zeros(5, np.float32), np.zeros(0, np.float32), picker=pk,
                     policy=1, stale_size=2)
    for i in range(3):
        r = u.update(upload(i), labels(i), 0, i)
    assert r == b"M1"
    assert not any(e[0].startswith("ledger") for e in c.log) and not hasattr(c.pools[0], "ledgers")
    assert [e[0] for e in c.log if e[0] == "update"] == ["update"]
