"""Bursts of the streaming aggregation without a GPU: the C-ABI's burst symbols and their
argument checks, the shim's pushBatchNative, and FleetUpdater.update_many's host logic
against a recording fake accumulator (CppNNUpdater.java:383-391, 463-464)."""
import ctypes as C
import os

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import synthetic
from fleet_amd.updater import FleetUpdater

BURST = ["fleet_acc_push_many", "fleet_acc_push_many_device", "fleet_acc_push_finish", "fleet_acc_push_finish_device",
         "fleet_acc_burst"]
JNI = os.path.join(os.path.dirname(F.LIB_PATH), "libfleet_native.so")


def test_header_declares_and_library_exports_the_burst_entry_points():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in BURST:
        assert s in declared, s
        assert hasattr(L, s), s
    assert F.ACC_BURST == L.fleet_acc_burst() and 1 < F.ACC_BURST <= 64  # 64 doubles travel in the kernel arguments


def test_null_and_absent_arguments():
    L = F.lib()
    buf = np.zeros(64, np.uint8)
    rows = (C.c_char_p * 2)(b"x" * 64, b"y" * 64)
    lens = np.array([64, 64], np.uint64)
    d = np.ones(2, np.float64)
    n = C.c_size_t(0)
    up, ln, dp, out = rows, lens.ctypes.data, d.ctypes.data, buf.ctypes.data
    # no accumulator: nothing else is looked at
    assert L.fleet_acc_push_many(None, up, ln, 2, dp) == F.FLEET_ERR_ARG
    assert L.fleet_acc_push_many(None, None, None, 0, None) == F.FLEET_ERR_ARG
    assert L.fleet_acc_push_many_device(None, out, 64, 2, dp, None) == F.FLEET_ERR_ARG
    assert L.fleet_acc_push_many_device(None, None, 64, 2, None, None) == F.FLEET_ERR_ARG
    assert L.fleet_acc_push_finish(None, up, ln, 2, dp, out, 64, C.byref(n), None) == F.FLEET_ERR_ARG
    assert L.fleet_acc_push_finish(None, None, None, 2, None, None, 0, None, None) == F.FLEET_ERR_ARG
    assert L.fleet_acc_push_finish_device(None, out, 64, 2, dp, out, None, None) == F.FLEET_ERR_ARG
    assert L.fleet_acc_push_finish_device(None, None, 64, -1, None, None, None, None) == F.FLEET_ERR_ARG
    assert n.value == 0


def test_shim_exports_push_batch_native():
    if not os.path.exists(JNI):
        pytest.skip("libfleet_native.so not built")
    F.lib()
    L = C.CDLL(JNI)
    assert hasattr(L, "Java_apps_cppNN_FleetUpdater_pushBatchNative")


class FakeAcc:
    def __init__(self, log, length, header_pos):
        self.log, self.length, self.count = log, length, 0
        self.header_pos = list(header_pos)

    def push(self, upload, dampen):
        self.log.append(("push", bytes(upload), dampen))
        self.count += 1

    def push_many(self, uploads, dampens):
        self.log.append(("push_many", [bytes(u) for u in uploads], list(dampens)))
        self.count += len(uploads)

    def finish(self, want_f32=False):
        self.log.append(("finish", self.count))
        self.count = 0
        return b"M%d" % len([e for e in self.log if e[0] in ("finish", "push_finish")]), np.zeros(8, np.float32)

    def push_finish(self, uploads, dampens, want_f32=False):
        self.log.append(("push_finish", [bytes(u) for u in uploads], list(dampens), self.count + len(uploads)))
        self.count = 0
        return b"M%d" % len([e for e in self.log if e[0] in ("finish", "push_finish")]), np.zeros(8, np.float32)

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

    def descent(self, weights, fc_bias, grad, layout, lr):
        self.log.append(("descent", float(lr)))
        return weights + 1, fc_bias


def folded(log):
    """(upload, factor) in the order the accumulator saw them, whatever the call."""
    out = []
    for e in log:
        if e[0] == "push":
            out.append((e[1], e[2]))
        elif e[0] in ("push_many", "push_finish"):
            out += list(zip(e[1], e[2]))
    return out


def make_arrivals(n, M):
    rng = np.random.default_rng(5)
    arr = []
    for i in range(n):
        labels = [int(x) for x in rng.integers(0, 9, 10)]
        arr.append((b"u%02d" % i + b"x" * 40, labels, max(0, i // M - i % 3), i))
    return arr


@pytest.mark.parametrize("cuts", [[11], [2, 1, 4, 4], [3, 3, 3, 2], [1] * 11, [4, 7]])
def test_update_many_cuts_at_the_batch_boundary_with_factors_of_arrival(cuts):
    lay = synthetic(8)
    M = 3
    mk = lambda c: FleetUpdater(c, lay, M, [0.05, 0.02], np.zeros(5, np.float32), np.zeros(0, np.float32),
                                policy=2, has_outlier=True, streaming=True)
    cm, cu = FakeCodec(), FakeCodec()
    many, single = mk(cm), mk(cu)
    arrivals = make_arrivals(sum(cuts), M)
    got, i = [], 0
    for k in cuts:
        before, pend = len(cm.log), len(many.acc)
        res = many.update_many(arrivals[i: i + k])
        assert len(res) == k
        got += res
        # the call's runs: up to the batch boundary, then whole batches, then the rest
        sizes, left, room = [], k, M - pend
        while left:
            sizes.append(min(left, room))
            left -= sizes[-1]
            room = M
        calls = [e for e in cm.log[before:] if e[0] != "descent"]
        assert [len(e[1]) for e in calls] == sizes
        fill = pend
        for e, sz in zip(calls, sizes):
            fill += sz
            # push_finish for the run that completes a batch and for no other
            assert e[0] == ("push_finish" if fill == M else "push_many")
            if fill == M:
                assert e[3] == M
                fill = 0
        # each completing run is followed at once by the model step
        kinds = [e[0] for e in cm.log[before:]]
        assert all(kinds[j + 1] == "descent" for j, x in enumerate(kinds) if x == "push_finish")
        assert kinds.count("descent") == kinds.count("push_finish")
        i += k
    want = [single.update(*a) for a in arrivals]
    assert got == want and any(w is not None for w in want)
    # the same uploads with bit for bit the same factors, in the same order: the factors of
    # a run after a model step were computed after that step, as update computes them
    assert folded(cm.log) == folded(cu.log)
    assert len({f for _, f in folded(cm.log)}) > 3  # the class-aware policy dampened stale picks
    assert many.curr_epoch == single.curr_epoch and many.global_labels == single.global_labels
    assert many.lr == single.lr and np.array_equal(many.weights, single.weights)
    assert len(many.acc) == len(single.acc) and many.last_merged == single.last_merged
    assert [e for e in cm.log if e[0] in ("push", "finish")] == []
    assert len(cm.accs) == 1 and cm.accs[0].header_pos == lay.header_positions()


def test_update_many_without_streaming_is_update_in_turn():
    class Batch(FakeCodec):
        def update(self, picked, dampen, want_f32=False):
            self.log.append(("update", [bytes(p) for p in picked], list(dampen)))
            return b"M%d" % len(self.log), np.zeros(8, np.float32)

    lay = synthetic(8)
    mk = lambda c: FleetUpdater(c, lay, 3, [0.05], np.zeros(5, np.float32), np.zeros(0, np.float32), policy=1)
    ca, cb = Batch(), Batch()
    a, b = mk(ca), mk(cb)
    arrivals = make_arrivals(7, 3)
    assert a.update_many(arrivals) == [b.update(*x) for x in arrivals]
    assert ca.log == cb.log and ca.accs == []
