"""The Kardam model ledger without a GPU: the host bookkeeping (mledger_table.cpp) against a
literal restatement of Kardam.setModel (tests/native/check_mledger_table.cpp, built and run
stand-alone, plainly and under the host sanitizers), the C-ABI's fleet_mledger_* symbols and
their argument checks, and FleetUpdater's ``kardam_models`` mode (CppNNUpdater.java:470-484)
against a recording fake codec, pool, ledgers and model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import synthetic
from fleet_amd.updater import FleetUpdater, Kardam
from test_kledger_cpu import LedgerCodec, RecordingKardam
from test_native_math import _clang
from test_pool_cpu import Script, labels, upload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MLEDGER = ["fleet_mledger_create", "fleet_mledger_destroy", "fleet_mledger_shape", "fleet_mledger_launch_shape",
           "fleet_mledger_stage", "fleet_mledger_stage_device", "fleet_mledger_stage_model", "fleet_mledger_resident",
           "fleet_mledger_update", "fleet_mledger_has", "fleet_mledger_version", "fleet_mledger_forget",
           "fleet_mledger_read", "fleet_mledger_read_version"]


# ------------------------------------------------------------------ the table unit

def build_checker(tmp_path_factory, flags):
    clang = _clang()
    if clang is None:
        pytest.skip("no clang++ for the host build of mledger_table.cpp")
    exe = tmp_path_factory.mktemp("native") / "check_mledger_table"
    cmd = [clang, "-std=c++17", "-O1", "-g", *flags, os.path.join(ROOT, "tests", "native", "check_mledger_table.cpp"),
           os.path.join(ROOT, "fleet_amd", "csrc", "mledger_table.cpp"), "-o", str(exe)]
    return cmd, str(exe)


def run_checker(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ALL OK" in r.stdout


def test_table_matches_the_reference_loop(tmp_path_factory):
    cmd, exe = build_checker(tmp_path_factory, [])
    subprocess.check_call(cmd)
    run_checker(exe)


def test_table_matches_the_reference_loop_under_sanitizers(tmp_path_factory):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
    cmd, exe = build_checker(tmp_path_factory, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitizer" in r.stderr.lower()):
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-4000:]
    run_checker(exe)


# ------------------------------------------------------------------------ the C-ABI

def test_header_declares_and_library_exports_the_model_ledger():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in MLEDGER + ["fleet_model_version_id"]:
        assert s in declared, s
        assert hasattr(L, s), s
    assert sorted(s for s in declared if s.startswith("fleet_mledger_")) == sorted(MLEDGER)
    assert hasattr(F, "ModelLedger") and hasattr(F.Codec, "model_ledger")
    assert hasattr(F.Model, "version_id") and hasattr(F.Model, "kardam_ledger")
    for m in ("stage", "stage_model", "resident", "update", "has", "version", "forget", "read", "close", "__enter__",
              "__exit__"):
        assert hasattr(F.ModelLedger, m), m
    assert F.ModelLedger.launch_shape() == (64, 1024, 64)  # host-only: no device is asked


def test_null_arguments():
    L = F.lib()
    h = C.c_void_p(0x1234)
    ids = np.array([1, 2], np.int64)
    wk = np.array([0, 1], np.int32)
    nm, nd, st = np.full(2, 7.0), np.full(2, 7.0), np.full(2, 9, np.uint8)
    buf = np.full(8, 5.0, np.float32)
    vid = C.c_int64(77)
    assert L.fleet_mledger_create(None, 4, 2, 1, 4, 2, C.byref(h)) == F.FLEET_ERR_ARG and h.value == 0x1234
    assert L.fleet_mledger_destroy(None) is None
    assert L.fleet_mledger_shape(None, None, None, None, None, None) == F.FLEET_ERR_ARG
    assert L.fleet_mledger_stage(None, 1, buf.ctypes.data, buf.ctypes.data) == F.FLEET_ERR_ARG
    assert L.fleet_mledger_stage_device(None, 1, buf.ctypes.data, buf.ctypes.data, None) == F.FLEET_ERR_ARG
    assert L.fleet_mledger_stage_model(None, None, 0, C.byref(vid)) == F.FLEET_ERR_ARG
    assert L.fleet_mledger_resident(None, 1) == F.FLEET_ERR_ARG
    assert L.fleet_mledger_has(None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_mledger_version(None, 0, C.byref(vid)) == F.FLEET_ERR_ARG
    assert L.fleet_mledger_forget(None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_mledger_read(None, 0, buf.ctypes.data, 8) == F.FLEET_ERR_ARG
    assert L.fleet_mledger_read_version(None, 0, buf.ctypes.data, 8) == F.FLEET_ERR_ARG
    assert L.fleet_model_version_id(None, 0, C.byref(vid)) == F.FLEET_ERR_ARG
    fake = C.c_void_p(0x10)  # never dereferenced: a NULL or a negative K beside it is found first
    good = [ids.ctypes.data, wk.ctypes.data, 2, nm.ctypes.data, nd.ctypes.data, st.ctypes.data]
    assert L.fleet_mledger_update(None, *good) == F.FLEET_ERR_ARG
    for i in (0, 1, 3, 4, 5):
        a = list(good)
        a[i] = None
        assert L.fleet_mledger_update(fake, *a) == F.FLEET_ERR_ARG, i
    good[2] = -1
    assert L.fleet_mledger_update(fake, *good) == F.FLEET_ERR_ARG
    assert vid.value == 77 and (buf == 5.0).all() and (nm == 7.0).all() and (nd == 7.0).all() and (st == 9).all()


# ------------------------------------------------------------------ FleetUpdater

class FakeModelLedger:
    """Plays Kardam.setModel (Kardam.java:114-125) on version ids alone and records the calls;
    the difference norm of two versions is the difference of their ids."""

    def __init__(self, log, workers, max_versions):
        self.log, self.workers, self.max_versions = log, workers, max_versions
        self.models = {}

    def stage_model(self, model, version):
        self.log.append(("stage_model", version))
        return model.version_id(version)

    def update(self, ids, workers):
        self.log.append(("mledger.update", [int(i) for i in ids], [int(w) for w in workers]))
        K = len(ids)
        nm, nd, st = np.full(K, np.nan), np.full(K, np.nan), np.zeros(K, np.uint8)
        for k, (i, w) in enumerate(zip(ids, workers)):
            if w < 0:
                continue
            nm[k] = 1.0
            if w in self.models:
                nd[k] = abs(float(i) - float(self.models[w]))
                if nd[k] == 0:
                    st[k] = 2
                    continue
                st[k] = 3
            else:
                st[k] = 1
            self.models[w] = int(i)
        return nm, nd, st


class FakeModel:
    """`models` as ids first .. first + size - 1: what fleet_amd.Model tells the updater."""

    def __init__(self, log, size, first=100):
        self.log, self.size, self.first = log, size, first
        self.ledgers = []

    def modelsSize(self):  # noqa: N802
        return self.size

    def version_id(self, v):
        assert 0 <= v < self.size
        return self.first + v

    def kardam_ledger(self, workers, max_versions=None):
        self.log.append(("model_ledger", workers, max_versions))
        self.ledgers.append(FakeModelLedger(self.log, workers, max_versions))
        return self.ledgers[-1]

    def step(self):  # descentNative at staleSize: a new version in, the oldest out
        self.first += 1


class ModelKardam(RecordingKardam):
    def apply_model(self, worker, status, norm_diff):
        self.log.append(("apply_model", worker, int(status), None if norm_diff != norm_diff else float(norm_diff)))
        return super().apply_model(worker, status, norm_diff)


def make(codec, picker, kardam, model, M=3, **kw):
    kw.setdefault("policy", 1)
    kw.setdefault("stale_size", 2)
    return FleetUpdater(codec, synthetic(8), M, [0.05, 0.02, 0.01], np.zeros(5, np.float32), np.zeros(0, np.float32),
                        picker=picker, kardam=kardam, kardam_models=model, **kw)


def test_constructor_rules():
    mk = lambda **kw: FleetUpdater(LedgerCodec(), synthetic(8), 3, [0.05], np.zeros(5, np.float32),
                                   np.zeros(0, np.float32), **kw)
    k = Kardam(None, 4)
    model = FakeModel([], 2)
    pk = lambda p, e: (None, [])
    with pytest.raises(ValueError):
        mk(kardam=k, kardam_models=model)  # no picker
    with pytest.raises(ValueError):
        mk(kardam=k, kardam_models=model, picker=pk, streaming=True)
    with pytest.raises(ValueError):
        mk(kardam=k, picker=pk)  # neither way to the models
    with pytest.raises(ValueError):
        mk(kardam=k, picker=pk, kardam_model=lambda tau: None, kardam_models=model)  # both
    with pytest.raises(ValueError):
        mk(picker=pk, kardam_model=lambda tau: None, kardam_models=model)
    u = mk(kardam=k, kardam_models=model, picker=pk)
    assert u.kardam is k and u.kardam_models is model and u.kardam_model is None
    assert k.ledger is None and k.model_ledger is None and model.log == []  # the ledgers come at the first update
    assert mk(kardam=k, kardam_model=lambda tau: None, picker=pk).kardam_models is None
    assert Kardam(None, 4, model_ledger="M").model_ledger == "M" and Kardam(None, 4, ledger="L").model_ledger is None


def test_apply_model_records_only_a_set():
    k = Kardam(None, 4)
    assert k.apply_model(1, 1, float("nan")) == 1 and k.apply_model(1, 2, 0.0) == 2 and k.apply_model(2, 0, float("nan")) == 0
    assert k.model_diff_norm == {}
    assert k.apply_model(1, 3, 2.5) == 3 and k.model_diff_norm == {1: 2.5}
    assert k.apply_model(3, 3, float("nan")) == 3 and k.model_diff_norm[3] != k.model_diff_norm[3]  # a NaN norm stores
    assert k.models == {}


def test_call_order_and_the_gate():
    c = LedgerCodec()
    pk = Script(([2, 0, 1], []), ([0, 2, 1], []), ([1, 0, 2], []))
    k = ModelKardam(c.log, 6)
    model = FakeModel(c.log, 2)
    u = make(c, pk, k, model)
    # update 1 at epoch 0: three new workers at tau 0, the newest version (index 1, id 101)
    for i in range(3):
        r = u.update(upload(i), labels(i), 0, i)
    assert r == b"L1"
    assert [e for e in c.log if e[0] == "model_ledger"] == [("model_ledger", 6, 2)]
    assert k.model_ledger is model.ledgers[0] and k.ledger is c.pools[0].ledgers[0]
    names = [e[0] for e in c.log if e[0] in ("ledger.update", "stage_model", "mledger.update", "apply_model", "apply",
                                              "update_lip", "descent")]
    # the gradient ledger first (it can reject a slot), one stage per distinct version, one
    # model-ledger update, then per pick apply_model before apply; the model step last
    assert names == ["ledger.update", "stage_model", "mledger.update"] + ["apply_model", "apply"] * 3 + ["descent"]
    assert [e for e in c.log if e[0] == "stage_model"] == [("stage_model", 1)]
    assert [e for e in c.log if e[0] == "mledger.update"] == [("mledger.update", [101, 101, 101], [2, 0, 1])]
    gl = [e for e in c.log if e[0] == "ledger.update"][0]
    assert gl[3] == [2, 0, 1]
    assert not any(e[0] == "set_model" for e in c.log)  # no text is asked for or subtracted
    model.step()
    # update 2 at epoch 1: worker 0 at tau 0 (index 1, id 102), worker 1 at tau 1 (index 0, id 101: the
    # version it holds, ignored), worker 3 at tau 2: index -1, Kardam does not run
    n0 = len(c.log)
    u.update(upload(3), labels(3), 1, 0)
    u.update(upload(4), labels(4), 0, 1)
    assert u.update(upload(5), labels(5), -1, 3) == b"L2"
    ev = c.log[n0:]
    gl = [e for e in ev if e[0] == "ledger.update"][0]
    assert gl[1] == [0, 2, 1] and gl[3] == [0, -1, 1]  # the same gate for both ledgers
    assert [e for e in ev if e[0] == "stage_model"] == [("stage_model", 1), ("stage_model", 0)]
    assert [e for e in ev if e[0] == "mledger.update"] == [("mledger.update", [102, -1, 101], [0, -1, 1])]
    loop = [e for e in ev if e[0] in ("apply_model", "apply", "update_lip")]
    assert [e[:2] for e in loop] == [("apply_model", 0), ("apply", 0), ("update_lip", 0), ("apply_model", 1), ("apply", 1)]
    assert loop[0] == ("apply_model", 0, 3, 1.0) and loop[3] == ("apply_model", 1, 2, 0.0)
    assert k.model_diff_norm == {0: 1.0} and k.lips == {0: [200.0 / 1.0]} and k.models == {}
    assert ev.index(gl) < ev.index(("stage_model", 1)) < ev.index(loop[0]) < ev.index(("descent", float(np.float32(0.02))))
    model.step()
    # update 3 at epoch 2 with one version fewer than staleSize: the gate is closed for every pick
    model.size = 1
    n0 = len(c.log)
    for i, (cid, ep) in enumerate([(0, 2), (1, 2), (2, 1)]):
        r = u.update(upload(6 + i), labels(i), ep, cid)
    assert r == b"L3"
    ev = c.log[n0:]
    gl = [e for e in ev if e[0] == "ledger.update"][0]
    assert gl[3] == [-1, -1, -1]
    assert [e for e in ev if e[0] == "mledger.update"] == [("mledger.update", [-1, -1, -1], [-1, -1, -1])]
    assert not any(e[0] in ("stage_model", "apply_model", "apply", "update_lip") for e in ev)


def test_a_worker_twice_in_one_update():
    c = LedgerCodec()
    pk = Script(([0, 1, 2], []), ([0, 1, 2], []))
    k = ModelKardam(c.log, 4)
    model = FakeModel(c.log, 2)
    u = make(c, pk, k, model)
    for i, (cid, ep) in enumerate([(1, 0), (2, 0), (3, 0)]):
        u.update(upload(i), labels(i), ep, cid)
    model.step()
    n0 = len(c.log)
    # worker 1 twice: at epoch 1 (id 102) and at epoch 0 (id 101, which it held before this update)
    for i, (cid, ep) in enumerate([(1, 1), (2, 0), (1, 0)]):
        r = u.update(upload(3 + i), labels(i), ep, cid)
    assert r == b"L2"
    ev = c.log[n0:]
    assert [e for e in ev if e[0] == "mledger.update"] == [("mledger.update", [102, 101, 101], [1, 2, 1])]
    assert [e for e in ev if e[0] == "stage_model"] == [("stage_model", 1), ("stage_model", 0)]
    loop = [e for e in ev if e[0] in ("apply_model", "apply", "update_lip")]
    assert [e[:2] for e in loop] == [("apply_model", 1), ("apply", 1), ("update_lip", 1), ("apply_model", 2), ("apply", 2),
                                     ("apply_model", 1), ("apply", 1), ("update_lip", 1)]
    # the later pick of worker 1 sees the model its earlier pick left: both differences are 1
    assert loop[0][2:] == (3, 1.0) and loop[3][2:] == (2, 0.0) and loop[5][2:] == (3, 1.0)
    assert k.lips == {1: [200.0 / 1.0, 202.0 / 1.0]}


def test_a_rejected_pool_update_leaves_the_model_ledger_untouched():
    c = LedgerCodec()
    pk = Script(([0, 1, 2], []), ([0, 1, 2], []), ([0, 1, 2], []))
    k = ModelKardam(c.log, 8)
    model = FakeModel(c.log, 2)
    u = make(c, pk, k, model)
    for i in range(3):
        u.update(upload(i), labels(i), 0, i)
    model.step()
    held = dict(model.ledgers[0].models)
    before = (dict(k.model_diff_norm), dict(k.grad_diff_norm), {w: list(v) for w, v in k.lips.items()})
    u.update(upload(3), labels(3), 1, 0)
    u.update(upload(4), labels(4), 1, 1)
    c.pools[0].fail = (F.Base64Error, [1])
    n0 = len(c.log)
    with pytest.raises(F.Base64Error):
        u.update(upload(5), labels(5), 1, 2)
    assert [e[0] for e in c.log[n0:]] == ["put", "ledger.update", "drop"]  # no stage, no model-ledger update
    assert model.ledgers[0].models == held
    assert (k.model_diff_norm, k.grad_diff_norm, k.lips) == before
    assert u.update(upload(6), labels(6), 1, 1) == b"L3"
    assert sorted(k.model_diff_norm) == [0, 1, 2]


def test_an_upload_from_a_later_epoch_is_refused_before_anything_changes():
    c = LedgerCodec()
    pk = Script(([0, 1, 2], []))
    k = ModelKardam(c.log, 4)
    u = make(c, pk, k, FakeModel(c.log, 2), policy=0)  # (policy 1 divides by tau + 1 = 0 first)
    u.update(upload(0), labels(0), 0, 0)
    u.update(upload(1), labels(1), 0, 1)
    with pytest.raises(ValueError):
        u.update(upload(2), labels(2), 1, 2)  # epoch 1 at epoch 0: modelsSize()-1-tau names no version
    assert not any(e[0] in ("ledger.update", "mledger.update", "descent") for e in c.log) and u.curr_epoch == 0
