"""The arrival gate without a GPU: the C-ABI's fleet_gate_* symbols and their argument
checks, the header codes against the oracle's float2int, and FleetUpdater's vet mode (an
arrival refused on the request that brought it, CppNNUpdater.java:350-353) against a
recording fake codec, pool and gate."""
import ctypes as C

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import CIFAR10, LAYOUTS, MNIST, synthetic
from fleet_amd.updater import FleetUpdater
from test_pool_cpu import POOL, FakeCodec, FakePool, Script, labels, upload

GATE = ["fleet_gate_header_codes", "fleet_gate_create", "fleet_gate_destroy", "fleet_gate_vet", "fleet_gate_vet_device",
        "fleet_gate_put"]


def test_header_declares_and_library_exports_the_gate_entry_points():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in GATE:
        assert s in declared, s
        assert hasattr(L, s), s
    assert sorted(s for s in declared if s.startswith("fleet_gate_")) == sorted(GATE)
    assert sorted(s for s in declared if s.startswith("fleet_pool_")) == sorted(POOL)  # no new pool name
    assert hasattr(F, "Gate") and hasattr(F, "Vet") and hasattr(F.Pool, "gate") and callable(F.header_codes)
    for m in ("vet", "vet_device", "put", "close", "__enter__", "__exit__"):
        assert hasattr(F.Gate, m), m
    v = F.Vet(2, 9.0, 1.5)
    assert (v.status, v.sumsq, v.max_abs, v.norm) == (2, 9.0, 1.5, 3.0) and tuple(v) == (2, 9.0, 1.5)


def test_null_and_absent_arguments():
    L = F.lib()
    slots = np.array([0, 1], np.int32)
    st = np.full(2, 77, np.int32)
    ss = np.full(2, 7.0)
    mx = np.full(2, 5.0, np.float32)
    text = np.full(64, 0x41, np.uint8)
    h = C.c_void_p(0x1234)
    fake = C.c_void_p(0x10)  # a gate argument that is never dereferenced: a NULL beside it is found first
    sl, s, q, m, up = slots.ctypes.data, st.ctypes.data, ss.ctypes.data, mx.ctypes.data, text.ctypes.data
    assert L.fleet_gate_create(None, None, 0, C.byref(h)) == F.FLEET_ERR_ARG
    assert h.value == 0x1234
    assert L.fleet_gate_create(fake, None, 0, None) == F.FLEET_ERR_ARG
    assert L.fleet_gate_destroy(None) is None
    assert L.fleet_gate_vet(None, sl, 2, s, q, m) == F.FLEET_ERR_ARG
    assert L.fleet_gate_vet_device(None, sl, 2, s, q, m, None) == F.FLEET_ERR_ARG
    assert L.fleet_gate_put(None, 0, up, 64, s, q, m) == F.FLEET_ERR_ARG
    host = [sl, 2, s, q, m]
    for i in (0, 2, 3, 4):
        a = list(host)
        a[i] = None
        assert L.fleet_gate_vet(fake, *a) == F.FLEET_ERR_ARG, i
        assert L.fleet_gate_vet_device(fake, *a, None) == F.FLEET_ERR_ARG, i
    for K in (0, -1):
        assert L.fleet_gate_vet(fake, sl, K, s, q, m) == F.FLEET_ERR_ARG
        assert L.fleet_gate_vet_device(fake, sl, K, s, q, m, None) == F.FLEET_ERR_ARG
    put = [0, up, 64, s, q, m]
    for i in (1, 3, 4, 5):
        a = list(put)
        a[i] = None
        assert L.fleet_gate_put(fake, *a) == F.FLEET_ERR_ARG, i
    codes = np.full(2, 9, np.int32)
    vals = np.ones(2, np.float32)
    assert L.fleet_gate_header_codes(vals.ctypes.data, -1, codes.ctypes.data) == F.FLEET_ERR_ARG
    assert L.fleet_gate_header_codes(None, 2, codes.ctypes.data) == F.FLEET_ERR_ARG
    assert L.fleet_gate_header_codes(vals.ctypes.data, 2, None) == F.FLEET_ERR_ARG
    assert L.fleet_gate_header_codes(None, 0, None) == F.FLEET_OK
    assert (st == 77).all() and (ss == 7.0).all() and (mx == 5.0).all() and (codes == 9).all()


@pytest.mark.parametrize("lay", [MNIST, CIFAR10, LAYOUTS["synth4m"]], ids=lambda l: l.name)
def test_header_codes_are_the_oracles_float2int(oracle, lay):
    vals = np.array(lay.header_values(), np.float32)
    codes = F.header_codes(lay.header_values())
    assert codes.dtype == np.int32 and len(codes) == len(lay.header_positions())
    assert np.array_equal(codes, oracle.float2int(vals))
    # what an upload carries there: the codes of the encoded values at the header positions
    if lay.n_up < 100000:
        v = oracle.synth_upload(3, 0, list(lay.w_sizes), list(lay.b_sizes))
        assert np.array_equal(oracle.decode_ints(oracle.encode_floats(v))[lay.header_positions()], codes)


# ------------------------------------------------------------------ FleetUpdater

class FakeGate:
    """Plays Gate.put: an upload whose text starts with b"bad" is not Base64 (status 1), one
    that starts with b"hdr" carries other header codes (2); the norm is the number between
    the first three characters and the next underscore (default 1)."""

    def __init__(self, log, pool, header_values):
        self.log, self.pool, self.header_values = log, pool, header_values

    def put(self, slot, upload):
        upload = bytes(upload)
        assert 0 <= slot < self.pool.slots and slot not in self.pool.rows
        status = 1 if upload.startswith(b"bad") else 2 if upload.startswith(b"hdr") else 0
        digits = upload[3:].split(b"_")[0]
        norm = float(digits) if digits else 1.0
        self.log.append(("gate.put", slot, upload, status))
        if status == 0:
            self.pool.rows[slot] = upload
        return F.Vet(status, norm * norm, norm)


class GatePool(FakePool):
    def gate(self, header_values=None):
        self.log.append(("gate", None if header_values is None else list(header_values)))
        self.gates = getattr(self, "gates", []) + [FakeGate(self.log, self, header_values)]
        return self.gates[-1]


class GateCodec(FakeCodec):
    def pool(self, length, header_pos, slots, group_begin=0, group_end=None):
        self.pools.append(GatePool(self.log, length, header_pos, slots))
        return self.pools[-1]


def make(codec, picker, M=3, **kw):
    kw.setdefault("policy", 1)
    kw.setdefault("stale_size", 2)
    return FleetUpdater(codec, synthetic(8), M, [0.05, 0.02], np.zeros(5, np.float32), np.zeros(0, np.float32),
                        picker=picker, **kw)


def text(kind, i, norm=""):
    return (kind + str(norm).encode() + b"_%02d" % i).ljust(44, b"x")


def test_vet_needs_a_picker():
    mk = lambda **kw: FleetUpdater(GateCodec(), synthetic(8), 3, [0.05], np.zeros(5, np.float32),
                                   np.zeros(0, np.float32), **kw)
    with pytest.raises(ValueError):
        mk(vet=True)
    with pytest.raises(ValueError):
        mk(vet=True, streaming=True)
    with pytest.raises(ValueError):
        mk(vet_max_norm=3.0, picker=lambda p, e: (None, []))  # a threshold on a norm nobody computes
    u = mk(vet=True, picker=lambda p, e: (None, []))
    assert u.vet and u.vet_max_norm is None and u.refused == []
    assert mk(picker=lambda p, e: (None, [])).vet is False


def test_a_refused_arrival_reaches_neither_acc_nor_the_picker_nor_M():
    c = GateCodec()
    pk = Script(([0, 1, 2], []))
    u = make(c, pk, vet=True)
    assert u.update(text(b"ok_", 0), labels(0), 0, 10) is None
    assert c.log[0] == ("gate", synthetic(8).header_values())  # the layout's header values, once
    assert u.update(text(b"bad", 1), labels(1), 0, 11) is None  # malformed
    assert u.update(text(b"hdr", 2), labels(2), 0, 12) is None  # another model's gradient
    assert u.refused == [(11, 1, 1.0), (12, 2, 1.0)]
    assert [(p.client_id, p.slot) for p in u.acc] == [(10, 0)]
    assert sorted(c.pools[0].rows) == [0] and pk.calls == []
    assert u.update(text(b"ok_", 3), labels(3), 0, 13) is None  # the refused slot 1 is free again
    assert [(p.client_id, p.slot) for p in u.acc] == [(10, 0), (13, 1)] and pk.calls == []
    assert u.update(text(b"bad", 4), labels(4), 0, 14) is None and pk.calls == []  # still two of M = 3
    r = u.update(text(b"ok_", 5), labels(5), 0, 15)
    assert r == b"M1" and len(pk.calls) == 1
    assert [cid for cid, _, _ in pk.calls[0][0]] == [10, 13, 15]  # the picker never saw a refused arrival
    call = [e for e in c.log if e[0] == "update"][0]
    assert call[1] == [0, 1, 2] and all(t.startswith(b"ok_") for t in call[3])
    assert [e[0] for e in c.log if e[0] in ("put", "gate")] == ["gate"]  # every arrival went through the gate
    assert len([e for e in c.log if e[0] == "gate.put"]) == 6
    assert u.refused == [(11, 1, 1.0), (12, 2, 1.0), (14, 1, 1.0)] and u.curr_epoch == 1


def test_vet_max_norm_drops_the_slot():
    c = GateCodec()
    pk = Script(([0, 1, 2], []))
    u = make(c, pk, vet=True, vet_max_norm=5.0)
    assert u.update(text(b"ok_", 0, 5), labels(0), 0, 20) is None  # at the threshold: admitted
    n0 = len(c.log)
    assert u.update(text(b"ok_", 1, 6), labels(1), 0, 21) is None  # over it
    assert [e[0] for e in c.log[n0:]] == ["gate.put", "drop"] and c.log[-1] == ("drop", 1)
    assert u.refused == [(21, 0, 6.0)] and sorted(c.pools[0].rows) == [0]
    assert [(p.client_id, p.slot) for p in u.acc] == [(20, 0)]
    n0 = len(c.log)
    assert u.update(text(b"bad", 2, 9), labels(2), 0, 22) is None  # refused by its text: nothing to drop
    assert [e[0] for e in c.log[n0:]] == ["gate.put"] and u.refused[-1] == (22, 1, 9.0)
    u.update(text(b"ok_", 3, 2), labels(3), 0, 23)
    assert u.update(text(b"ok_", 4, 1), labels(4), 0, 24) == b"M1"
    assert [cid for cid, _, _ in pk.calls[0][0]] == [20, 23, 24]


def test_without_vet_no_gate_is_made():
    c = GateCodec()
    u = make(c, Script(([0, 1, 2], [])))
    for i in range(3):
        r = u.update(upload(i), labels(i), 0, i)
    assert r == b"M1" and u.refused == []
    assert not any(e[0].startswith("gate") for e in c.log) and not hasattr(c.pools[0], "gates")
    assert [e[0] for e in c.log] == ["put", "put", "put", "update", "descent", "drop", "drop", "drop"]
