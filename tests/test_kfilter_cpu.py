"""Kardam's Byzantine filter without a GPU: the C-ABI's fleet_kfilter_* symbols and their NULL
checks, updater.percentile (commons-math3 3.6.1's default Percentile) on hand-worked cases,
Kardam.check_byz against a line-by-line transcription of Kardam.java:136-185 kept here, and
FleetUpdater's argument checks for kardam_filter."""
import ctypes as C
import math

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import MNIST
from fleet_amd.updater import FleetUpdater, Kardam, percentile
from test_kledger_cpu import LEDGER
from test_pool_cpu import POOL

FILTER = ["fleet_kfilter_create", "fleet_kfilter_destroy", "fleet_kfilter_has_last", "fleet_kfilter_set_model",
          "fleet_kfilter_set_model_device", "fleet_kfilter_update", "fleet_kfilter_update_device",
          "fleet_kfilter_resolve", "fleet_kfilter_resolve_device"]


def test_header_declares_and_library_exports_the_filter_entry_points():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in FILTER:
        assert s in declared, s
        assert hasattr(L, s), s
    assert sorted(s for s in declared if s.startswith("fleet_kfilter_")) == sorted(FILTER)
    assert sorted(s for s in declared if s.startswith("fleet_kledger_")) == sorted(LEDGER)  # no new ledger name
    assert sorted(s for s in declared if s.startswith("fleet_pool_")) == sorted(POOL)
    assert hasattr(F, "KardamFilter") and hasattr(F.Ledger, "filter")
    for m in ("set_model", "set_model_device", "update", "update_device", "resolve", "resolve_device", "has_last",
              "close", "__enter__", "__exit__"):
        assert hasattr(F.KardamFilter, m), m


def test_null_and_absent_arguments():
    L = F.lib()
    h = C.c_void_p(0x1234)
    n = C.c_size_t(7)
    a2 = np.zeros(2)
    i2 = np.zeros(2, np.int32)
    u2 = np.ones(2, np.uint8)
    buf = np.zeros(64, np.uint8)
    nm, nd = C.c_double(5.0), C.c_double(5.0)
    fake = C.c_void_p(0x10)  # never dereferenced: a NULL beside it is found first
    assert L.fleet_kfilter_create(None, 4, 2, 1, C.byref(h)) == F.FLEET_ERR_ARG
    assert h.value == 0x1234
    assert L.fleet_kfilter_create(fake, 4, 2, 1, None) == F.FLEET_ERR_ARG
    assert L.fleet_kfilter_destroy(None) is None
    assert L.fleet_kfilter_has_last(None) == F.FLEET_ERR_ARG
    assert L.fleet_kfilter_set_model(None, buf.ctypes.data, buf.ctypes.data, C.byref(nm), C.byref(nd)) == F.FLEET_ERR_ARG
    assert L.fleet_kfilter_set_model_device(None, buf.ctypes.data, buf.ctypes.data, C.byref(nm), C.byref(nd),
                                            None) == F.FLEET_ERR_ARG
    assert nm.value == 5.0 and nd.value == 5.0
    pk, dp, w, ep, out = i2.ctypes.data, a2.ctypes.data, i2.ctypes.data, i2.ctypes.data, buf.ctypes.data
    g, s = a2.ctypes.data, u2.ctypes.data
    host = [pk, 2, dp, w, ep, 0.05, out, 64, C.byref(n), None, g, g, s, g, g]
    assert L.fleet_kfilter_update(None, *host) == F.FLEET_ERR_ARG
    for i in (0, 2, 3, 4, 6, 10, 11, 12, 13, 14):
        a = list(host)
        a[i] = None
        assert L.fleet_kfilter_update(fake, *a) == F.FLEET_ERR_ARG, i
    a = list(host)
    a[1] = 0
    assert L.fleet_kfilter_update(fake, *a) == F.FLEET_ERR_ARG
    dev = [pk, 2, dp, w, ep, 0.05, out, None, g, g, s, g, g, None]
    assert L.fleet_kfilter_update_device(None, *dev) == F.FLEET_ERR_ARG
    for i in (0, 2, 3, 4, 6, 8, 9, 10, 11, 12):
        a = list(dev)
        a[i] = None
        assert L.fleet_kfilter_update_device(fake, *a) == F.FLEET_ERR_ARG, i
    res = [s, 2, out, 64, C.byref(n), None]
    assert L.fleet_kfilter_resolve(None, *res) == F.FLEET_ERR_ARG
    for i in (0, 2, 4):
        a = list(res)
        a[i] = None
        assert L.fleet_kfilter_resolve(fake, *a) == F.FLEET_ERR_ARG, i
    rdev = [s, 2, out, None, C.byref(n), None]
    assert L.fleet_kfilter_resolve_device(None, *rdev) == F.FLEET_ERR_ARG
    for i in (0, 2, 4):
        a = list(rdev)
        a[i] = None
        assert L.fleet_kfilter_resolve_device(fake, *a) == F.FLEET_ERR_ARG, i
    assert n.value == 7 and (buf == 0).all()


# ------------------------------------------------------------------------ percentile

def test_percentile_hand_worked():
    """Percentile.evaluate, estimation LEGACY: pos = p (n + 1) / 100; below 1 the minimum, at
    or above n the maximum, else lower + (pos - floor(pos)) (upper - lower) at ranks floor(pos),
    floor(pos) + 1 counted from 1."""
    assert percentile([7.5], 1) == 7.5 and percentile([7.5], 100) == 7.5          # n = 1
    assert percentile([3.0, 1.0, 2.0, 9.0], 10) == 1.0                              # pos = 0.5 < 1
    assert percentile([3.0, 1.0, 2.0, 9.0], 80) == 9.0                              # pos = 4 >= n
    assert percentile([3.0, 1.0, 2.0, 9.0], 99) == 9.0
    # n = 4, p = 50: pos = 2.5, ranks 2 and 3 of (1, 2, 3, 9): 2 + 0.5 (3 - 2)
    assert percentile([3.0, 1.0, 2.0, 9.0], 50) == 2.5
    # n = 5, p = 30: pos = 1.8 (computed: 30 * 6 / 100), ranks 1 and 2 of (10, 20, 40, 80, 160)
    pos = 30 * 6 / 100
    assert percentile([160.0, 10.0, 80.0, 20.0, 40.0], 30) == 10.0 + (pos - 1) * (20.0 - 10.0)
    p = 200 / 3.0
    # n = 2: pos = p * 3 / 100 = 2.0000000000000004 or 2 >= n: the maximum
    assert p * 3 / 100 >= 2 and percentile([4.0, 1.0], p) == 4.0
    # n = 3: pos = p * 4 / 100 = 2.66..., ranks 2 and 3 of (1, 4, 16)
    pos = p * 4 / 100
    assert math.floor(pos) == 2 and percentile([16.0, 1.0, 4.0], p) == 4.0 + (pos - 2) * (16.0 - 4.0)
    # n = 4: pos = p * 5 / 100 = 3.33..., ranks 3 and 4 of (1, 4, 16, 64)
    pos = p * 5 / 100
    assert math.floor(pos) == 3 and percentile([64.0, 16.0, 1.0, 4.0], p) == 16.0 + (pos - 3) * (64.0 - 16.0)
    assert math.isnan(percentile([], 50))
    for bad in (0, -1, 100.5):
        with pytest.raises(ValueError):
            percentile([1.0, 2.0], bad)
    v = [3.0, 1.0, 2.0]
    percentile(v, 50)
    assert v == [3.0, 1.0, 2.0]  # the caller's list is left alone (Helpers.percentile sorts a copy `l`)


# ------------------------------------------------------------------------- check_byz

class JavaKardam:
    """Kardam.java:136-203 line by line (checkByz, updateLip), on norms in place of vectors."""

    def __init__(self, workers):
        self.workers = workers
        self.lips = {}
        self.gradDiffNorm, self.modelDiffNorm = {}, {}
        self.subsequentRejects = 0
        self.last = None  # (checkNorm, high) of the last decision that read the norms

    @staticmethod
    def div(a, b):
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))

    @staticmethod
    def percentile(lst, p):  # Helpers.java:52-59 + Percentile.evaluate (LEGACY)
        lst.sort()
        n = len(lst)
        if n == 1:
            return lst[0]
        pos = p * (n + 1) / 100
        fpos = math.floor(pos)
        int_pos = int(fpos)
        dif = pos - fpos
        if pos < 1:
            return lst[0]
        if pos >= n:
            return lst[n - 1]
        lower = lst[int_pos - 1]
        upper = lst[int_pos]
        return lower + dif * (upper - lower)

    def checkByz(self, g_norm, g_diff_norm, m_norm, m_diff_norm, lastGrad_is_null):  # noqa: N802
        self.last = None
        l = []                                               # :137
        if not self.lips:                                    # :138
            self.subsequentRejects = 0
            return True
        for worker in self.lips:                             # :142
            l.append(max(self.lips[worker]))                 # :145
            self.lips[worker].sort()                         # :149
        high = self.percentile(l, 200 / 3.0)                 # :156
        if lastGrad_is_null:                                 # :159
            checkNorm = self.div(g_norm, m_norm)             # :161
        else:
            checkNorm = self.div(g_diff_norm, m_diff_norm)   # :165-167
        self.last = (checkNorm, high)
        if checkNorm <= high:                                # :170
            self.subsequentRejects = 0
            return True
        elif self.subsequentRejects == self.workers:         # :174
            self.subsequentRejects = 0
            return True
        else:
            self.subsequentRejects += 1                      # :180
            return False

    def updateLip(self, w):  # noqa: N802
        lip = self.gradDiffNorm[w] / self.modelDiffNorm[w]   # :193
        if w not in self.lips:
            self.lips[w] = []
        if len(self.lips[w]) > 25:                           # :199
            self.lips[w].pop(0)                              # remove(0)
        self.lips[w].append(lip)


def both(workers):
    return Kardam(None, workers), JavaKardam(workers)


def push_lip(k, j, w, gd, md):
    k.grad_diff_norm[w], k.model_diff_norm[w] = gd, md
    j.gradDiffNorm[w], j.modelDiffNorm[w] = gd, md
    k.update_lip(w)
    j.updateLip(w)


def same_state(k, j):
    assert k.lips == j.lips and [list(v) for v in k.lips.values()] == [list(v) for v in j.lips.values()]
    assert k.subsequent_rejects == j.subsequentRejects


def test_empty_lips_accept_and_reset():
    k, j = both(3)
    k.subsequent_rejects = j.subsequentRejects = 2
    assert k.check_byz(0, 1e9, 1e9, 1.0, 1.0, False) is True and j.checkByz(1e9, 1e9, 1.0, 1.0, True) is True
    same_state(k, j)
    assert k.subsequent_rejects == 0


def test_the_sort_changes_which_lip_the_27th_drops():
    """26 descending lips, a check_byz (which sorts them ascending in place, :149), a 27th:
    remove(0) then drops the smallest value, not the oldest, which was the largest."""
    k, j = both(4)
    for i in range(26):
        push_lip(k, j, 1, float(100 - i), 1.0)
    assert k.lips[1][0] == 100.0 and len(k.lips[1]) == 26
    unsorted = Kardam(None, 4)
    unsorted.lips[1] = list(k.lips[1])
    assert k.check_byz(1, 50.0, 0.0, 1.0, 0.0, False) == j.checkByz(50.0, 0.0, 1.0, 0.0, True)
    assert k.lips[1] == sorted(k.lips[1]) and k.lips[1][0] == 75.0
    same_state(k, j)
    push_lip(k, j, 1, 7.0, 1.0)
    same_state(k, j)
    assert len(k.lips[1]) == 26 and 75.0 not in k.lips[1] and 100.0 in k.lips[1] and k.lips[1][-1] == 7.0
    unsorted.grad_diff_norm[1], unsorted.model_diff_norm[1] = 7.0, 1.0
    unsorted.update_lip(1)
    assert 100.0 not in unsorted.lips[1] and 75.0 in unsorted.lips[1]  # what no sort would have left


def test_rejects_count_up_to_workers_then_one_accept():
    k, j = both(3)
    for w, lip in ((0, 1.0), (1, 2.0), (2, 4.0), (0, 3.0)):
        push_lip(k, j, w, lip, 1.0)
    decisions = []
    for i in range(9):  # checkNorm 50 > high for every call: 3 rejects, the escape, 3 rejects, ...
        has_last = bool(i % 2)
        a = k.check_byz(i % 3, 50.0, 100.0, 1.0, 2.0, has_last)
        assert a == j.checkByz(50.0, 100.0, 1.0, 2.0, not has_last)
        assert j.last[0] == 50.0 and j.last[1] < 50.0
        decisions.append(a)
        same_state(k, j)
    assert decisions == [False, False, False, True, False, False, False, True, False]
    assert k.subsequent_rejects == 1
    # an accept by the norm resets the counter
    assert k.check_byz(0, 1.0, 0.0, 1.0, 0.0, False) is True and j.checkByz(1.0, 0.0, 1.0, 0.0, True) is True
    same_state(k, j)
    assert k.subsequent_rejects == 0


def test_division_by_zero_rejects():
    k, j = both(5)
    push_lip(k, j, 0, 2.0, 1.0)
    push_lip(k, j, 1, 8.0, 1.0)
    cases = [(3.0, 0.0, 0.0, 0.0, False),    # x / 0 = +inf without a last gradient
             (0.0, 0.0, 0.0, 0.0, False),    # 0 / 0 = NaN
             (1.0, 3.0, 1.0, 0.0, True),     # x / 0 with one
             (1.0, 0.0, 1.0, 0.0, True),     # 0 / 0 with one
             (1.0, float("nan"), 1.0, 2.0, True)]
    for n, (gp, gd, mm, md, has_last) in enumerate(cases):
        a = k.check_byz(0, gp, gd, mm, md, has_last)
        assert a is False and j.checkByz(gp, gd, mm, md, not has_last) is False, n
        assert not (j.last[0] <= j.last[1])
        same_state(k, j)
    assert k.subsequent_rejects == 5
    assert k.check_byz(0, 3.0, 0.0, 0.0, 0.0, False) is True and j.checkByz(3.0, 0.0, 0.0, 0.0, True) is True  # == workers
    same_state(k, j)


def test_scripted_sequence_matches_the_transcription():
    rng = np.random.default_rng(17)
    k, j = both(4)
    for step in range(300):
        w = int(rng.integers(0, 6))
        if rng.random() < 0.5:
            push_lip(k, j, w, float(rng.uniform(0.1, 10)), float(rng.uniform(0.1, 10)))
        else:
            gp, gd, mm, md = (float(x) for x in rng.uniform(0.0, 10, 4))
            has_last = bool(rng.integers(0, 2))
            assert k.check_byz(w, gp, gd, mm, md, has_last) == j.checkByz(gp, gd, mm, md, not has_last), step
        same_state(k, j)
    assert any(len(v) == 26 for v in k.lips.values())


# --------------------------------------------------------------- FleetUpdater's checks

def test_updater_argument_checks():
    w = np.zeros(MNIST.n_weights, np.float32)
    b = np.zeros(MNIST.n_fc_bias, np.float32)
    kd = Kardam(None, 4)
    model = object()

    def pick(p, e):
        return None, []
    ok = FleetUpdater(None, MNIST, 2, [0.1], w, b, stale_size=2, picker=pick, kardam=kd, kardam_models=model,
                      kardam_filter=True)
    assert ok.kardam_filter and ok.last_accept is None
    plain = FleetUpdater(None, MNIST, 2, [0.1], w, b, stale_size=2, picker=pick, kardam=kd, kardam_models=model)
    assert not plain.kardam_filter
    for kw in (dict(),                                                      # not the pooled branch
               dict(streaming=True),
               dict(picker=pick),                                           # no kardam
               dict(picker=pick, kardam=kd, kardam_model=lambda tau: None),  # texts, not a model
               dict(kardam=kd, kardam_models=model)):                        # kardam without a picker
        with pytest.raises(ValueError):
            FleetUpdater(None, MNIST, 2, [0.1], w, b, kardam_filter=True, **kw)
    assert "checkByz`` is not rebuilt" not in Kardam.__doc__ and "check_byz" in Kardam.__doc__
