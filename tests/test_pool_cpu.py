"""The upload pool without a GPU: the C-ABI's fleet_pool_* symbols and their argument
checks, and FleetUpdater's picker mode (the staleSize > 0 branch, CppNNUpdater.java:383-411,
420-421, 463-464) against a recording fake codec and pool."""
import ctypes as C

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import synthetic
from fleet_amd.updater import FleetUpdater, get_dampen, similarity

POOL = ["fleet_pool_create", "fleet_pool_destroy", "fleet_pool_slots", "fleet_pool_occupied", "fleet_pool_put",
        "fleet_pool_put_device", "fleet_pool_drop", "fleet_pool_update", "fleet_pool_update_device",
        "fleet_pool_slot_status"]


def test_header_declares_and_library_exports_the_pool_entry_points():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in POOL:
        assert s in declared, s
        assert hasattr(L, s), s
    assert sorted(s for s in declared if s.startswith("fleet_pool_")) == sorted(POOL)
    assert hasattr(F, "Pool") and hasattr(F.Codec, "pool")


def test_null_and_absent_arguments():
    L = F.lib()
    buf = np.full(64, 0x5A, np.uint8)
    picks = np.array([0, 1], np.int32)
    d = np.ones(2, np.float64)
    n = C.c_size_t(0)
    h = C.c_void_p(0x1234)
    pk, dp, out = picks.ctypes.data, d.ctypes.data, buf.ctypes.data
    # no pool: nothing else is looked at
    assert L.fleet_pool_create(None, 64, None, 0, 0, 4, 2, C.byref(h)) == F.FLEET_ERR_ARG
    assert h.value == 0x1234
    assert L.fleet_pool_destroy(None) is None
    assert L.fleet_pool_slots(None) == F.FLEET_ERR_ARG
    assert L.fleet_pool_occupied(None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_pool_slot_status(None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_pool_put(None, 0, out, 64) == F.FLEET_ERR_ARG
    assert L.fleet_pool_put(None, 0, None, 64) == F.FLEET_ERR_ARG
    assert L.fleet_pool_put_device(None, 0, out, None) == F.FLEET_ERR_ARG
    assert L.fleet_pool_put_device(None, 0, None, None) == F.FLEET_ERR_ARG
    assert L.fleet_pool_drop(None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_pool_update(None, pk, 2, dp, out, 64, C.byref(n), None) == F.FLEET_ERR_ARG
    assert L.fleet_pool_update_device(None, pk, 2, dp, out, None, None) == F.FLEET_ERR_ARG
    for K in (0, -1):
        assert L.fleet_pool_update(None, None, K, None, None, 0, C.byref(n), None) == F.FLEET_ERR_ARG
        assert L.fleet_pool_update(None, None, K, None, out, 64, C.byref(n), None) == F.FLEET_ERR_ARG
        assert L.fleet_pool_update_device(None, None, K, None, None, None, None) == F.FLEET_ERR_ARG
        assert L.fleet_pool_update_device(None, None, K, None, out, None, None) == F.FLEET_ERR_ARG
    assert n.value == 0
    assert (buf == 0x5A).all()


# ------------------------------------------------------------------ FleetUpdater

class FakePool:
    def __init__(self, log, length, header_pos, slots):
        self.log, self.length, self.slots = log, length, slots
        self.header_pos = list(header_pos)
        self.rows = {}
        self.fail = None  # (exception class, slots at fault) for the next update

    def free_slot(self):
        for s in range(self.slots):
            if s not in self.rows:
                return s
        return None

    def occupied(self, slot):
        return slot in self.rows

    def put(self, slot, upload):
        assert 0 <= slot < self.slots
        self.log.append(("put", slot, bytes(upload)))
        self.rows[slot] = bytes(upload)

    def drop(self, slot):
        self.log.append(("drop", slot))
        del self.rows[slot]

    def update(self, picks, dampens, want_f32=False):
        picks = [int(s) for s in picks]
        assert want_f32 and all(s in self.rows for s in picks)
        self.log.append(("update", picks, [float(x) for x in dampens], [self.rows[s] for s in picks]))
        if self.fail is not None:
            exc, slots = self.fail
            self.fail = None
            e = exc(F.FLEET_ERR_BASE64, "slot: input is not Base64::encode output")
            e.slots = list(slots)
            raise e
        return b"M%d" % len([e for e in self.log if e[0] == "update"]), np.zeros(8, np.float32)

    def close(self):
        pass


class FakeCodec:
    """Records what the updater asks of the codec; computes nothing."""

    def __init__(self):
        self.log = []
        self.pools = []

    def pool(self, length, header_pos, slots, group_begin=0, group_end=None):
        self.pools.append(FakePool(self.log, length, header_pos, slots))
        return self.pools[-1]

    def descent(self, weights, fc_bias, grad, layout, lr):
        self.log.append(("descent", float(lr)))
        return weights + 1, fc_bias


class Script:
    """A picker that plays back (picks, discard) results and records its calls."""

    def __init__(self, *results):
        self.results, self.calls = list(results), []

    def __call__(self, pending, curr_epoch):
        self.calls.append(([(p.client_id, p.slot, p.epoch) for p in pending], curr_epoch))
        assert all(p.upload == b"" for p in pending)  # the bytes live in the pool
        return self.results.pop(0)


def upload(i):
    return b"u%02d" % i + b"x" * 40


def labels(i):
    return [(3 * i + j) % 7 for j in range(10)]


def make(codec, picker, M=3, **kw):
    kw.setdefault("policy", 1)
    kw.setdefault("stale_size", 2)
    return FleetUpdater(codec, synthetic(8), M, [0.05, 0.02], np.zeros(5, np.float32), np.zeros(0, np.float32),
                        picker=picker, **kw)


def test_constructor_rules():
    mk = lambda **kw: FleetUpdater(FakeCodec(), synthetic(8), 3, [0.05], np.zeros(5, np.float32),
                                   np.zeros(0, np.float32), **kw)
    with pytest.raises(NotImplementedError):
        mk(stale_size=2)
    with pytest.raises(ValueError):
        mk(picker=lambda p, e: (None, []), streaming=True)
    with pytest.raises(ValueError):
        mk(stale_size=2, picker=lambda p, e: (None, []), streaming=True)
    assert mk(stale_size=2, picker=lambda p, e: (None, [])).pool_slots == 12  # 4 M
    assert mk(picker=lambda p, e: (None, []), pool_slots=5).pool_slots == 5
    assert mk().picker is None


def test_arrivals_go_to_the_lowest_free_slot_and_the_picker_waits_for_m():
    c = FakeCodec()
    pk = Script((None, []), ([2, 0, 3], [1]), ([3, 1, 0], []))
    u = make(c, pk)
    # below M buffered: the upload is put, the picker is not asked
    assert u.update(upload(0), labels(0), 0, 10) is None
    assert u.update(upload(1), labels(1), 0, 11) is None
    assert pk.calls == [] and [e for e in c.log] == [("put", 0, upload(0)), ("put", 1, upload(1))]
    assert len(c.pools) == 1 and c.pools[0].slots == 12 and c.pools[0].header_pos == synthetic(8).header_positions()
    # M buffered, the picker returns None: nothing changes
    before = (u.curr_epoch, list(u.global_labels), u.weights.copy(), u.lr)
    assert u.update(upload(2), labels(2), 0, 12) is None
    assert pk.calls == [([(10, 0, 0), (11, 1, 0), (12, 2, 0)], 0)]
    assert c.log[2:] == [("put", 2, upload(2))]
    assert (u.curr_epoch, u.global_labels, u.lr) == (before[0], before[1], before[3])
    assert np.array_equal(u.weights, before[2]) and [p.slot for p in u.acc] == [0, 1, 2]
    # a non-arrival order: slots in pick order, entry 1 discarded unpicked
    u.curr_epoch = 2
    n0 = len(c.log)
    assert u.update(upload(3), labels(3), 2, 13) == b"M1"
    assert pk.calls[-1] == ([(10, 0, 0), (11, 1, 0), (12, 2, 0), (13, 3, 2)], 2)
    ev = c.log[n0:]
    assert ev[0] == ("put", 3, upload(3)) and ev[1] == ("drop", 1)
    assert ev[2][0] == "update" and ev[2][1] == [2, 0, 3] and ev[2][3] == [upload(2), upload(0), upload(3)]
    # factors from the epoch at pick time (tau = 2, 2, 0), policy 1 = 1 / (tau + 1)
    assert ev[2][2] == [get_dampen(1, 2), get_dampen(1, 2), get_dampen(1, 0)] == [1 / 3, 1 / 3, 1.0]
    assert ev[3] == ("descent", float(np.float32(0.05)))
    assert sorted(ev[4:]) == [("drop", 0), ("drop", 2), ("drop", 3)]
    assert u.acc == [] and u.curr_epoch == 3 and u.last_merged == b"M1"
    # the label vector grows by the picked uploads only
    assert u.global_labels == [labels(2)[j] + labels(0)[j] + labels(3)[j] for j in range(10)]


def test_unpicked_entries_survive_with_their_slots():
    c = FakeCodec()
    pk = Script((None, []), ([3, 1, 0], []), ([2, 0, 1], []))
    u = make(c, pk, pool_slots=6)
    for i in range(3):
        assert u.update(upload(i), labels(i), 0, i) is None
    assert u.update(upload(3), labels(3), 0, 3) == b"M1"
    assert [(p.client_id, p.slot) for p in u.acc] == [(2, 2)] and u.curr_epoch == 1
    # the freed slots are reused lowest first; entry 2 keeps slot 2
    assert u.update(upload(4), labels(4), 1, 4) is None
    assert [(p.client_id, p.slot) for p in u.acc] == [(2, 2), (4, 0)] and len(pk.calls) == 2
    n0 = len(c.log)
    assert u.update(upload(5), labels(5), 0, 5) == b"M2"
    assert pk.calls[-1] == ([(2, 2, 0), (4, 0, 1), (5, 1, 0)], 1)
    ev = c.log[n0:]
    assert ev[0] == ("put", 1, upload(5))
    assert ev[1][:2] == ("update", [1, 2, 0]) and ev[1][3] == [upload(5), upload(2), upload(4)]
    # similarity enters policy 1 nowhere; tau = 1, 1, 0 at epoch 1
    assert ev[1][2] == [0.5, 0.5, 1.0]
    assert u.acc == [] and u.curr_epoch == 2 and c.pools[0].rows == {}
    assert len(c.pools) == 1


def test_factors_read_the_label_vector_as_it_stands_before_the_update():
    """Policy 2 (class-aware): every pick's similarity is against the global label vector of
    before the update (CppNNUpdater.java:463-464; the vector grows after the loop, :502-504)."""
    c = FakeCodec()
    pk = Script(([1, 2, 0], []), ([0, 2, 1], []))
    u = make(c, pk, policy=2, has_outlier=True, stale_size=1)
    for i in range(3):
        u.update(upload(i), labels(i), 0, i)
    g1 = list(u.global_labels)
    assert g1 == [labels(0)[j] + labels(1)[j] + labels(2)[j] for j in range(10)]
    u.curr_epoch = 5
    outlier = [0] * 9 + [40]
    u.update(upload(3), outlier, 0, 3)
    u.update(upload(4), labels(4), 5, 4)
    u.update(upload(5), labels(5), 3, 5)
    ev = [e for e in c.log if e[0] == "update"][-1]
    want = [get_dampen(2, 5, similarity(outlier, g1), 1, 0.0, True), get_dampen(2, 2, similarity(labels(5), g1), 1, 0.0, True),
            get_dampen(2, 0, similarity(labels(4), g1), 1, 0.0, True)]
    assert ev[2] == want and len(set(want)) == 3


def test_discards_are_dropped_also_when_nothing_is_picked():
    c = FakeCodec()
    pk = Script((None, [0, 2]), (None, []), ([1, 0, 2], []))
    u = make(c, pk)
    for i in range(3):
        assert u.update(upload(i), labels(i), 0, i) is None
    assert sorted(c.log[-2:]) == [("drop", 0), ("drop", 2)]  # too old for the simulator: gone whether or not it picks
    assert [(p.client_id, p.slot) for p in u.acc] == [(1, 1)]
    assert u.update(upload(3), labels(3), 0, 3) is None  # 2 buffered: below M again, the picker rests
    assert len(pk.calls) == 1
    assert u.update(upload(4), labels(4), 0, 4) is None
    assert u.update(upload(5), labels(5), 0, 5) == b"M1"
    assert [e for e in c.log if e[0] == "update"][0][1] == [0, 1, 2]  # entries 3, 1, 4 in slots 0, 1, 2
    assert [(p.client_id, p.slot) for p in u.acc] == [(5, 3)]


def test_a_full_pool_raises_before_anything_changes():
    c = FakeCodec()
    pk = Script((None, []))
    u = make(c, pk, pool_slots=3)
    for i in range(3):
        assert u.update(upload(i), labels(i), 0, i) is None
    n0, acc0 = len(c.log), list(u.acc)
    with pytest.raises(RuntimeError):
        u.update(upload(3), labels(3), 0, 3)
    assert len(c.log) == n0 and u.acc == acc0 and len(pk.calls) == 1
    assert sorted(c.pools[0].rows) == [0, 1, 2]


@pytest.mark.parametrize("picks,discard", [([0, 1], []), ([0, 1, 1], []), ([0, 1, 4], []), ([0, 1, 2], [2]), (None, [7])])
def test_a_picker_result_that_is_no_pick_list_is_refused(picks, discard):
    c = FakeCodec()
    u = make(c, Script((picks, discard)))
    for i in range(2):
        u.update(upload(i), labels(i), 0, i)
    with pytest.raises(ValueError):
        u.update(upload(2), labels(2), 0, 2)
    assert [e[0] for e in c.log] == ["put"] * 3 and len(u.acc) == 3


def test_an_update_that_raises_drops_exactly_the_named_slots():
    c = FakeCodec()
    pk = Script((None, []), ([0, 1, 2], []), ([1, 0, 3], []))
    u = make(c, pk)
    for i in range(3):
        assert u.update(upload(i), labels(i), 0, i) is None
    c.pools[0].fail = (F.Base64Error, [1])
    w0, b0, g0 = u.weights.copy(), u.fc_bias.copy(), list(u.global_labels)
    n0 = len(c.log)
    with pytest.raises(F.Base64Error) as ei:
        u.update(upload(3), labels(3), 0, 3)
    assert ei.value.slots == [1]
    ev = c.log[n0:]
    assert [e[0] for e in ev] == ["put", "update", "drop"] and ev[2] == ("drop", 1)
    assert [(p.client_id, p.slot) for p in u.acc] == [(0, 0), (2, 2), (3, 3)]
    assert np.array_equal(u.weights, w0) and np.array_equal(u.fc_bias, b0) and u.global_labels == g0
    assert u.curr_epoch == 0 and u.last_merged is None
    # the survivors are picked at the next arrival, the freed slot is reused
    assert u.update(upload(4), labels(4), 0, 4) == b"M2"
    last = [e for e in c.log if e[0] == "update"][-1]
    assert last[1] == [2, 0, 1] and last[3] == [upload(2), upload(0), upload(4)]
    assert [(p.client_id, p.slot) for p in u.acc] == [(3, 3)]
