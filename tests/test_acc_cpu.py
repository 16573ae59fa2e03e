"""Streaming aggregation without a GPU: the C-ABI's new symbols and their argument
checks, the shim's streaming natives, and FleetUpdater(streaming=True)'s host logic
against a recording fake codec (CppNNUpdater.java:383-391, 463-464)."""
import ctypes as C
import os

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import synthetic
from fleet_amd.updater import FleetUpdater

ACC = ["fleet_acc_create", "fleet_acc_destroy", "fleet_acc_push", "fleet_acc_push_device", "fleet_acc_count",
       "fleet_acc_finish", "fleet_acc_finish_device", "fleet_acc_reset"]
JNI = os.path.join(os.path.dirname(F.LIB_PATH), "libfleet_native.so")


def test_header_declares_and_library_exports_the_accumulator():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in ACC:
        assert s in declared, s
        assert hasattr(L, s), s


def test_null_and_absent_arguments():
    L = F.lib()
    h = C.c_void_p()
    pos = np.zeros(2, np.int32)
    buf = np.zeros(64, np.uint8)
    n = C.c_size_t(0)
    assert L.fleet_acc_create(None, 64, pos.ctypes.data, 2, 0, 4, C.byref(h)) == F.FLEET_ERR_ARG
    assert not h.value
    assert L.fleet_acc_create(None, 64, pos.ctypes.data, 2, 0, 4, None) == F.FLEET_ERR_ARG
    L.fleet_acc_destroy(None)  # a no-op
    assert L.fleet_acc_push(None, buf.ctypes.data, 64, 1.0) == F.FLEET_ERR_ARG
    assert L.fleet_acc_push_device(None, buf.ctypes.data, 1.0, None) == F.FLEET_ERR_ARG
    assert L.fleet_acc_count(None) == F.FLEET_ERR_ARG
    assert L.fleet_acc_finish(None, buf.ctypes.data, 64, C.byref(n), None) == F.FLEET_ERR_ARG
    assert L.fleet_acc_finish_device(None, buf.ctypes.data, None, None) == F.FLEET_ERR_ARG
    assert L.fleet_acc_reset(None) == F.FLEET_ERR_ARG


def test_shim_exports_the_streaming_natives():
    if not os.path.exists(JNI):
        pytest.skip("libfleet_native.so not built")
    F.lib()
    L = C.CDLL(JNI)
    for s in ("pushNative", "finishNative", "pendingNative", "discardNative"):
        assert hasattr(L, "Java_apps_cppNN_FleetUpdater_" + s), s


class FakeAcc:
    def __init__(self, log, length, header_pos):
        self.log, self.length, self.count = log, length, 0
        self.header_pos = list(header_pos)

    def push(self, upload, dampen):
        self.log.append(("push", bytes(upload), dampen))
        self.count += 1

    def finish(self, want_f32=False):
        self.log.append(("finish", self.count))
        self.count = 0
        return b"M%d" % len(self.log), np.zeros(8, np.float32)

    def close(self):
        pass


class FakeCodec:
    """Records what the updater asks of the codec; computes nothing."""

    def __init__(self):
        self.log = []
        self.accs = []

    def accumulator(self, length, header_pos, group_begin=0, group_end=None):
        self.accs.append(FakeAcc(self.log, length, header_pos))
        return self.accs[-1]

    def update(self, picked, dampen, want_f32=False):
        self.log.append(("update", [bytes(p) for p in picked], list(dampen)))
        return b"M%d" % len(self.log), np.zeros(8, np.float32)

    def descent(self, weights, fc_bias, grad, layout, lr):
        self.log.append(("descent", float(lr)))
        return weights + 1, fc_bias


def test_streaming_updater_pushes_the_batch_paths_factors_on_arrival():
    lay = synthetic(8)
    M = 3
    mk = lambda s, c: FleetUpdater(c, lay, M, [0.05, 0.02], np.zeros(5, np.float32), np.zeros(0, np.float32),
                                   policy=2, has_outlier=True, streaming=s)
    cs, cb = FakeCodec(), FakeCodec()
    s, b = mk(True, cs), mk(False, cb)
    rng = np.random.default_rng(5)
    arrivals = []
    for i in range(3 * M):
        up = b"u%02d" % i + b"x" * 40
        labels = [int(x) for x in rng.integers(0, 9, 10)]
        epoch = max(0, i // M - i % 3)
        arrivals.append(up)
        before = len(cs.log)
        rs, rb = s.update(up, labels, epoch, i), b.update(up, labels, epoch, i)
        new = cs.log[before:]
        # every arrival is pushed at once; only the M-th also finishes and steps the model
        assert new[0][0] == "push" and new[0][1] == up
        if i % M == M - 1:
            assert [e[0] for e in new] == ["push", "finish", "descent"] and new[1] == ("finish", M)
            assert rs is not None and rb is not None
        else:
            assert len(new) == 1 and rs is None and rb is None
        assert s.curr_epoch == b.curr_epoch and s.global_labels == b.global_labels and s.lr == b.lr
        assert np.array_equal(s.weights, b.weights) and len(s.acc) == len(b.acc)
    pushes = [e for e in cs.log if e[0] == "push"]
    batches = [e for e in cb.log if e[0] == "update"]
    assert len(batches) == 3 and len(pushes) == 3 * M
    for r, (_, picked, dampen) in enumerate(batches):
        assert picked == arrivals[M * r: M * r + M]
        # bit for bit the factor the batch loop computes for that pick at the M-th call
        assert [p[2] for p in pushes[M * r: M * r + M]] == dampen
    assert len({f for _, _, d in batches for f in d}) > 3  # the class-aware policy dampened stale picks
    assert [e for e in cs.log if e[0] == "update"] == []  # the streaming object never calls the batch update
    assert len(cs.accs) == 1 and cs.accs[0].header_pos == lay.header_positions() and cs.accs[0].length == len(arrivals[0])
    assert [e[1] for e in cs.log if e[0] == "descent"] == [e[1] for e in cb.log if e[0] == "descent"]
