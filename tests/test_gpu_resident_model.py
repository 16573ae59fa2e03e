"""The model resident in HBM (fleet_rmodel, fleet_amd.ResidentModel) against the unchanged
host model (fleet_amd.Model) and the reference's own session (session_mnist.npz): every
text, every version's bits, the ring, the errors, the allocation rule, the Kardam ledger."""
import os

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import CIFAR10, MNIST

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W_BLOCKS = [s for s in MNIST.w_sizes if s]  # the non-null W of the MNIST model
B_BLOCKS = [8, 16, 48, 10]                  # its use_bias() layers: C1, C2i, C2, FC2


@pytest.fixture(scope="module")
def session():
    return np.load(os.path.join(HERE, "golden", "session_mnist.npz"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _g(x):
    """`ostream << float` of one value, as libc's '%g' (nan spelled with its sign)"""
    x = np.float32(x)
    if np.isnan(x):
        return "-nan" if _bits([x])[0] >> 31 else "nan"
    return "%g" % float(x)


def _lines(values, blocks):
    out, o = [], 0
    for n in blocks:
        out.append("".join(_g(v) + " " for v in values[o:o + n]) + "\n")
        o += n
    return "".join(out)


def _mode0_text(session, codec, weights=None, biases=None):
    """The fixture's model as a DISTILLATION_MODE=0 text: its header, its biases and '%g' weights."""
    init = bytes(session["init"])
    hm = F.Model(codec, init, distillation_mode=1)
    w, b = hm.export(-1)
    hm.close()
    cut = init.index(b" \n%d\n" % len(w)) + 2     # the weights section starts with the weight count
    header = init[:cut]
    n_bias_lines = len(B_BLOCKS)
    lines = header.split(b"\n")
    head = b"\n".join(lines[: len(lines) - 1 - n_bias_lines]) + b"\n"
    w = w if weights is None else weights
    b = b if biases is None else biases
    return head + _lines(b, B_BLOCKS).encode() + _lines(w, W_BLOCKS).encode(), head


def _same(rm, hm):
    """every observable of the two models is equal, bit for bit"""
    assert rm.modelsSize() == hm.modelsSize()
    assert rm.getCurrEpoch() == hm.getCurrEpoch() and rm.getLrate() == hm.getLrate()
    for v in [-1] + list(range(hm.modelsSize())):
        (rw, rb), (hw, hb) = rm.export(v), hm.export(v)
        assert np.array_equal(_bits(rw), _bits(hw)), f"weights of version {v}"
        assert np.array_equal(_bits(rb), _bits(hb)), f"biases of version {v}"
        if v >= 0:
            assert rm.version_id(v) == hm.version_id(v)


def _same_texts(rm, hm, versions=None):
    for v in (range(hm.modelsSize()) if versions is None else versions):
        assert rm.getParametersNative(v) == hm.getParametersNative(v)
        assert rm.getModelParametersNative(v) == hm.getModelParametersNative(v)


def _decode_device(codec, text):
    import torch
    t = np.frombuffer(bytes(text), np.uint8)
    pitch = (len(t) + 15) // 16 * 16 + 16
    d = torch.zeros((1, pitch), dtype=torch.uint8, device="cuda")
    d[0, : len(t)] = torch.from_numpy(t.copy()).cuda()
    n = F.b64_count(len(t))
    out = torch.zeros((1, n + 3), dtype=torch.float32, device="cuda")
    codec.decode_device(d, len(t), out)
    codec.check()
    return out[0], n


# -- 1. the reference's session, DISTILLATION_MODE=1 ----------------------------------------

@pytest.mark.parametrize("device_form", [False, True])
def test_session_mode1(codec, oracle, session, device_form):
    s = session
    rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1, max_versions=3)
    hm = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    rm.initUpdater(s["lrates"])
    hm.initUpdater(s["lrates"])
    assert rm.modelsSize() == 1 and rm.getCurrEpoch() == 0

    def check(state):
        newest = rm.modelsSize() - 1
        assert rm.getParametersNative(newest) == bytes(s[f"newest_text{state}"])
        assert rm.getParametersNative(0) == bytes(s[f"oldest_text{state}"])
        for v, key in ((newest, "newest"), (0, "oldest")):
            assert rm.getModelParametersNative(v) == oracle.encode_floats(s[f"{key}_params{state}"])
        _same(rm, hm)
        _same_texts(rm, hm)
    check(0)
    for i in range(3):
        hm.descentNative(bytes(s[f"merged{i}"]), int(s["batch"]), int(s["stale"]))
        if device_form:
            g, n = _decode_device(codec, s[f"merged{i}"])
            rm.descent_device(g, int(s["stale"]), n_values=n)
        else:
            rm.descentNative(bytes(s[f"merged{i}"]), int(s["batch"]), int(s["stale"]))
        check(i + 1)
    assert rm.modelsSize() == int(s["n_models"]) and rm.getCurrEpoch() == 3
    assert rm.getLrate() == float(np.float32(s["lrates"][2]))
    import torch
    out = torch.zeros(len(hm.getModelParametersNative(0)) + 32, dtype=torch.uint8, device="cuda")
    n = rm.getModelParametersNative_device(0, out)   # on torch's current stream, as torch.zeros above
    torch.cuda.current_stream().synchronize()          # that stream alone orders the output
    assert out[:n].cpu().numpy().tobytes() == hm.getModelParametersNative(0)
    rm.close()
    hm.close()


# -- 2. the same session, DISTILLATION_MODE=0 ------------------------------------------------

def test_session_mode0(codec, session):
    s = session
    text, head = _mode0_text(s, codec)
    rm = F.ResidentModel(codec, text, distillation_mode=0, max_versions=3)
    hm = F.Model(codec, text, distillation_mode=0)
    rm.initUpdater(s["lrates"])
    hm.initUpdater(s["lrates"])
    _same(rm, hm)
    _same_texts(rm, hm)
    for i in range(3):
        hm.descentNative(bytes(s[f"merged{i}"]), int(s["batch"]), int(s["stale"]))
        if i == 1:
            g, n = _decode_device(codec, s[f"merged{i}"])
            rm.descent_device(g, int(s["stale"]), n_values=n)
        else:
            rm.descentNative(bytes(s[f"merged{i}"]), int(s["batch"]), int(s["stale"]))
        _same(rm, hm)
        _same_texts(rm, hm)
        # the bias and weight lines directly against Python's '%g'
        for v in range(rm.modelsSize()):
            w, b = rm.export(v)
            assert rm.getParametersNative(v) == head + (_lines(b, B_BLOCKS) + _lines(w, W_BLOCKS)).encode()
    rm.close()
    hm.close()


# -- 4. the ring -----------------------------------------------------------------------------

@pytest.mark.parametrize("stale", [0, 1, 2, 3])
def test_ring(codec, session, stale):
    s = session
    rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1, max_versions=3)
    hm = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    rm.initUpdater(s["lrates"])
    hm.initUpdater(s["lrates"])
    seen = {rm.version_id(0)}
    for i in range(stale + 3):
        m = bytes(s[f"merged{i % 3}"])
        ids_before = [rm.version_id(v) for v in range(rm.modelsSize())]
        hm.descentNative(m, 8, stale)
        rm.descentNative(m, 8, stale)
        _same(rm, hm)
        newest = rm.modelsSize() - 1
        _same_texts(rm, hm, versions={0, newest})
        tw, tb = rm.version_tensors(newest)
        assert np.array_equal(_bits(tw.cpu().numpy()), _bits(hm.export(newest)[0]))
        assert np.array_equal(_bits(tb.cpu().numpy()), _bits(hm.export(newest)[1]))
        # versions are addressed by index: the one the step popped has no index any more (its
        # id is gone from the ring, the others keep theirs), and the index past the ring raises
        ids = [rm.version_id(v) for v in range(rm.modelsSize())]
        assert ids == sorted(ids) and ids[-1] == i + 1 and ids[-1] not in seen
        kept = max(1, stale)
        assert ids == (ids_before + [i + 1])[-kept:]
        for gone in set(ids_before) - set(ids):
            assert gone == ids_before[0] and gone not in ids
        seen.update(ids)
        with pytest.raises(F.FleetError):
            rm.version_tensors(rm.modelsSize())
    assert rm.modelsSize() == max(1, stale)
    with pytest.raises(F.FleetError):
        rm.version_id(rm.modelsSize())
    rm.close()
    hm.close()


@pytest.mark.parametrize("max_versions", [1, 2, 3])
def test_step_beyond_max_versions_is_refused(codec, session, max_versions):
    """With the ring full (max_versions versions), a step at a larger stale_size would keep one
    more: FLEET_ERR_ARG from both forms and from initUpdater, with epoch, count and cnn unchanged."""
    s = session
    rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1, max_versions=max_versions)
    rm.initUpdater(s["lrates"])
    for i in range(max_versions - 1):
        rm.descentNative(bytes(s[f"merged{i}"]), 8, max_versions)
    assert rm.modelsSize() == max_versions
    before = _snapshot(rm)
    d, n = _decode_device(codec, s["merged2"])
    for call in (lambda: rm.descentNative(bytes(s["merged2"]), 8, max_versions + 1),
                 lambda: rm.descent_device(d, max_versions + 1, n_values=n),
                 lambda: rm.initUpdater(s["lrates"])):
        with pytest.raises(F.FleetError) as e:
            call()
        assert e.value.code == F.FLEET_ERR_ARG
        _unchanged(before, _snapshot(rm))
    rm.descent_device(d, max_versions, n_values=n)     # at its own stale_size it steps on
    assert rm.modelsSize() == max_versions and rm.getCurrEpoch() == max_versions
    rm.close()


def test_device_arguments_are_checked(codec, session):
    """descent_device and getModelParametersNative_device hand data_ptr() to kernels: a tensor of
    another type, on the host or not contiguous is refused before anything is launched; so is a
    ledger of another context."""
    import torch
    s = session
    rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1, max_versions=2)
    rm.initUpdater(s["lrates"])
    d, n = _decode_device(codec, s["merged0"])
    before = _snapshot(rm)
    for bad in (d.cpu(), d.double(), d.to(torch.int32), torch.zeros((n + 3, 2), device="cuda")[:, 0], np.zeros(n, np.float32)):
        with pytest.raises(ValueError):
            rm.descent_device(bad, 2, n_values=n)
    out = torch.zeros(F.b64_len(21940) + 32, dtype=torch.uint8, device="cuda")
    for bad in (out.cpu(), out.float(), out[::2]):
        with pytest.raises(ValueError):
            rm.getModelParametersNative_device(0, bad)
    with pytest.raises(ValueError):
        rm.getModelParametersNative_device(0, out[:100])
    _unchanged(before, _snapshot(rm))
    other = F.Codec(0)
    led = other.model_ledger(21448, 82, 6, 2)
    with pytest.raises(F.FleetError) as e:
        led.stage_model(rm, 0)
    assert e.value.code == F.FLEET_ERR_ARG and not led.resident(rm.version_id(0))
    led.close()
    other.close()
    rm.close()


# -- 5. errors ---------------------------------------------------------------------------------

def _snapshot(rm):
    return [rm.getCurrEpoch(), rm.modelsSize()] + [
        _bits(x).copy() for v in [-1] + list(range(rm.modelsSize())) for x in rm.export(v)]


def _unchanged(a, b):
    assert a[:2] == b[:2]
    for x, y in zip(a[2:], b[2:]):
        assert np.array_equal(x, y)


def test_refused_gradients_change_nothing(codec, oracle, session):
    s = session
    rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1, max_versions=3)
    rm.initUpdater(s["lrates"])
    rm.descentNative(bytes(s["merged0"]), 8, 2)
    snap = _snapshot(rm)
    # a merged gradient of another layout (CIFAR-10), as text and on the device
    g = oracle.encode_floats(oracle.synth_upload(3, 0, list(CIFAR10.w_sizes), list(CIFAR10.b_sizes)))
    with pytest.raises(F.LayoutError):
        rm.descentNative(g, 8, 2)
    _unchanged(snap, _snapshot(rm))
    d, n = _decode_device(codec, g)
    with pytest.raises(F.LayoutError):
        rm.descent_device(d, 2, n_values=n)
    _unchanged(snap, _snapshot(rm))
    # a wrong n_values: too short for the model (refused on the host), one short, one long
    d, n = _decode_device(codec, s["merged1"])
    for bad_n in (100, n - 1, n + 1):
        with pytest.raises(F.FleetError) as e:
            rm.descent_device(d, 2, n_values=bad_n)
        assert e.value.code in (F.FLEET_ERR_ARG, F.FLEET_ERR_LAYOUT)
        _unchanged(snap, _snapshot(rm))
    # a header slot altered on the device: the weight-block count, a block size, a bias size, a fraction
    pos = MNIST.header_positions()
    for p, delta in ((pos[0], 1.0), (pos[1], 1.0), (pos[3], -1.0), (pos[-1], 1.0), (pos[1], 0.5)):
        bad = d.clone()
        bad[p] += delta
        with pytest.raises(F.FleetError) as e:
            rm.descent_device(bad, 2, n_values=n)
        assert e.value.code in (F.FLEET_ERR_ARG, F.FLEET_ERR_LAYOUT)
        _unchanged(snap, _snapshot(rm))
    # not Base64
    with pytest.raises(F.Base64Error):
        rm.descentNative(b"!" + bytes(s["merged1"])[1:], 8, 2)
    _unchanged(snap, _snapshot(rm))
    # and the model still steps as the host model does
    hm = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    hm.initUpdater(s["lrates"])
    hm.descentNative(bytes(s["merged0"]), 8, 2)
    hm.descentNative(bytes(s["merged1"]), 8, 2)
    rm.descent_device(d, 2, n_values=n)
    _same(rm, hm)
    rm.close()
    hm.close()


def test_mode1_inf_weight_after_the_step(codec, session):
    """lr * g overflows for one weight: the model copy's text read fails in the reference; both
    models return the same code and are left in the same state (cnn stepped, epoch advanced,
    no version pushed)."""
    s = session
    g = codec.decode_floats(bytes(s["merged0"])).copy()
    g[2] = 2.0                      # the first weight's gradient
    merged = codec.encode_floats(g)
    rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1, max_versions=3)
    hm = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    codes = []
    for m in (rm, hm):
        m.initUpdater([3e38])
        with pytest.raises(F.FleetError) as e:
            m.descentNative(merged, 8, 2)
        codes.append(e.value.code)
    assert codes[0] == codes[1] == F.FLEET_ERR_ARG
    assert np.isinf(hm.export(-1)[0][0]) and hm.getCurrEpoch() == 1 and hm.modelsSize() == 1
    _same(rm, hm)
    rm.close()
    hm.close()


def test_mode0_nonfinite_values(codec, session):
    s = session
    hm1 = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    w, b = hm1.export(-1)
    hm1.close()
    w, b = w.copy(), b.copy()
    w[[0, 1, 2, 3, 250, 21447]] = _u2f([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFF800000])
    b[[0, 9, 72, 73, 81]] = _u2f([0x7F800000, 0xFFC00000, 0x7FC00000, 0xFF800000, 0x7F800000])  # conv and fc biases
    text, head = _mode0_text(s, codec, w, b)
    rm = F.ResidentModel(codec, text, distillation_mode=0, max_versions=3)
    hm = F.Model(codec, text, distillation_mode=0)
    rm.initUpdater(s["lrates"])
    hm.initUpdater(s["lrates"])
    _same(rm, hm)
    _same_texts(rm, hm)
    for i in range(2):
        m = bytes(s[f"merged{i}"])
        hm.descentNative(m, 8, 2)
        rm.descentNative(m, 8, 2)
        _same(rm, hm)
        _same_texts(rm, hm)
    # (an inf weight steps to NaN: 0 * inf; a convolution's inf bias is never stepped and stays)
    assert np.isnan(rm.export(1)[0][0]) and np.isnan(rm.export(1)[0][2]) and np.isinf(rm.export(1)[1][0])
    rm.close()
    hm.close()


def _u2f(bits):
    return np.array(bits, np.uint32).view(np.float32)


# -- 6. the allocation rule ----------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 0])
def test_no_allocation_after_warm_up(codec, session, mode):
    s = session
    text = bytes(s["init"]) if mode else _mode0_text(s, codec)[0]
    rm = F.ResidentModel(codec, text, distillation_mode=mode, max_versions=3)
    nw, nb, _, _ = rm.shape()
    assert (nw, nb) == (21448, 82)
    assert rm.stats()["resident_bytes"] == 4 * ((nw + nb + 63) // 64 * 64) * (3 + 2)   # the docstring's formula
    rm.initUpdater(s["lrates"])
    led = rm.kardam_ledger(4)
    d, n = _decode_device(codec, s["merged0"])

    def each_entry(i):
        rm.descentNative(bytes(s[f"merged{i % 3}"]), 8, 2)
        rm.descent_device(d, 2, n_values=n)
        newest = rm.modelsSize() - 1
        rm.getParametersNative(newest)
        rm.getModelParametersNative(newest)
        rm.version_tensors(newest)
        rm.export(0)
        led.stage_model(rm, newest)
    each_entry(0)                       # the warm-up
    allocs = rm.stats()["device_allocs"]
    for i in range(5):
        each_entry(i + 1)
    assert rm.stats()["device_allocs"] == allocs
    led.close()
    rm.close()


# -- 7. the Kardam model ledger --------------------------------------------------------------------

def test_ledger_stages_device_to_device(codec, session):
    s = session
    rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1, max_versions=3)
    hm = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    for m in (rm, hm):
        m.initUpdater(s["lrates"])
        m.descentNative(bytes(s["merged0"]), 8, 2)
        m.descentNative(bytes(s["merged1"]), 8, 2)
    lr, lh = rm.kardam_ledger(3), hm.kardam_ledger(3)
    for v in range(rm.modelsSize()):
        vid = lr.stage_model(rm, v)
        assert vid == lh.stage_model(hm, v) == hm.version_id(v)
        assert np.array_equal(_bits(lr.read_version(vid)), _bits(lh.read_version(vid)))
    ids = [rm.version_id(0), rm.version_id(1), rm.version_id(1)]
    a, b = lr.update(ids, [0, 1, 0]), lh.update(ids, [0, 1, 0])
    assert np.array_equal(a[2], b[2])
    for x, y in zip(a[:2], b[:2]):
        assert np.allclose(x, y, rtol=1e-12, atol=0, equal_nan=True)
    with pytest.raises(F.FleetError):
        lr.stage_model(rm, 7)
    for x in (lr, lh, rm, hm):
        x.close()


def test_updater_on_a_resident_model(codec, oracle, session):
    """The same arrivals and picker through FleetUpdater on numpy weights with the host Model as
    kardam_models, and through FleetUpdater(model=rm, kardam_models=rm, weights=None): the pooled
    path then runs Ledger.update_device into the updater's tensors and rm.descent_device, and
    the model ledger stages device to device. Merged bytes equal; Kardam's state equal (norms
    of the model differences to 1e-12, the rest exactly); the final weights bit for bit."""
    from fleet_amd.updater import FleetUpdater, Kardam
    from test_gpu_pool import uploads_for
    s, lay = session, MNIST
    lrates = [0.05, 0.02, 0.01, 0.01]
    hm = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1, max_versions=2)
    for m in (hm, rm):
        m.initUpdater(lrates)
        m.descentNative(bytes(s["merged0"]), 8, 2)   # two versions: Kardam's gate (modelsSize == staleSize) opens
        m.setCurrEpoch(0)                            # the updaters count their epochs from 0
    w, b = hm.export(-1)
    ups = uploads_for(oracle, lay, 12, seed=909)
    arrivals = [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1), (1, 0), (3, 2), (2, 1), (4, 0), (1, 3), (3, 3), (1, 2)]
    scripts = [[([2, 0, 1], []), ([1, 0, 2], []), ([0, 2, 1], []), ([0, 1, 2], [])] for _ in range(2)]
    ka, kb = Kardam(codec, 6), Kardam(codec, 6)
    ua = FleetUpdater(codec, lay, 3, lrates, w, b[-lay.n_fc_bias:], policy=1, stale_size=2,
                      picker=lambda p, e: scripts[0].pop(0), kardam=ka, kardam_models=hm)
    ub = FleetUpdater(codec, lay, 3, lrates, None, None, policy=1, stale_size=2,
                      picker=lambda p, e: scripts[1].pop(0), kardam=kb, kardam_models=rm, model=rm)
    allocs = None
    for i, (cid, ep) in enumerate(arrivals):
        ga = ua.update(ups[i], [i % 10] * 10, ep, client_id=cid)
        gb = ub.update(ups[i], [i % 10] * 10, ep, client_id=cid)
        assert ga == gb and (ga is None) == (i % 3 != 2)
        if ga is None:
            continue
        hm.descentNative(ga, 8, 2)       # the host path's model steps beside its updater
        assert kb.grad_diff_norm == ka.grad_diff_norm and kb.lips.keys() == ka.lips.keys()
        assert kb.model_diff_norm.keys() == ka.model_diff_norm.keys()
        for wk in ka.model_diff_norm:
            np.testing.assert_allclose(kb.model_diff_norm[wk], ka.model_diff_norm[wk], rtol=1e-12, atol=0)
        for wk in ka.lips:
            np.testing.assert_allclose(kb.lips[wk], ka.lips[wk], rtol=1e-12, atol=0)
        for wk in range(6):
            assert kb.model_ledger.has(wk) == ka.model_ledger.has(wk)
            if ka.model_ledger.has(wk):
                assert kb.model_ledger.version(wk) == ka.model_ledger.version(wk)
                assert np.array_equal(_bits(kb.model_ledger.read(wk)), _bits(ka.model_ledger.read(wk)))
        rw, rb = rm.export(-1)
        assert np.array_equal(_bits(ua.weights), _bits(rw))
        assert np.array_equal(_bits(ua.fc_bias), _bits(rb[-lay.n_fc_bias:]))
        _same(rm, hm)
        assert ub.curr_epoch == ua.curr_epoch == rm.getCurrEpoch()
        if allocs is None:
            allocs = rm.stats()["device_allocs"]
    assert scripts == [[], []] and sorted(ka.lips) == [1, 2, 3]
    assert rm.stats()["device_allocs"] == allocs      # nothing allocated on the model's behalf after the first round
    assert ub.weights is None and ub.fc_bias is None
    for x in (ua._mledger, ub._mledger, hm, rm):
        x.close()


@pytest.mark.parametrize("streaming", [False, True])
def test_updater_fifo_and_streaming_on_a_resident_model(codec, oracle, session, streaming):
    from fleet_amd.updater import FleetUpdater
    from test_gpu_pool import uploads_for
    s, lay = session, MNIST
    lrates = [0.05, 0.02]
    hm = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1, max_versions=1)
    hm.initUpdater(lrates)
    w, b = hm.export(-1)
    ups = uploads_for(oracle, lay, 6, seed=31)
    ua = FleetUpdater(codec, lay, 3, lrates, w, b[-lay.n_fc_bias:], policy=1, streaming=streaming)
    ub = FleetUpdater(codec, lay, 3, lrates, None, None, policy=1, streaming=streaming, model=rm)   # initUpdater is the updater's
    for i in range(6):
        ga = ua.update(ups[i], [i % 10] * 10, i // 3, client_id=i)
        gb = ub.update(ups[i], [i % 10] * 10, i // 3, client_id=i)
        assert ga == gb and (ga is None) == (i % 3 != 2)
        if ga is not None:
            hm.descentNative(ga, 8, 0)
            _same(rm, hm)
            assert np.array_equal(_bits(ua.weights), _bits(rm.export(-1)[0]))
    hm.close()
    rm.close()


@pytest.mark.parametrize("side_stream", [False, True])
def test_device_forms_run_on_the_callers_stream(codec, session, side_stream):
    """The gradient is produced by torch work queued on the current stream (torch's default: the
    null stream, or a side stream) right before descent_device, with no synchronise between;
    the a20 text is consumed by torch work on that stream right after. Both order with the
    model's kernels only if those run on the stream the caller passed."""
    import contextlib
    import torch
    s = session
    mode = 0 if side_stream else 1
    text0 = _mode0_text(s, codec)[0] if mode == 0 else bytes(s["init"])
    rm = F.ResidentModel(codec, text0, distillation_mode=mode, max_versions=2)
    hm = F.Model(codec, text0, distillation_mode=mode)
    rm.initUpdater(s["lrates"])
    hm.initUpdater(s["lrates"])
    g, n = _decode_device(codec, s["merged0"])
    big = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream() if side_stream else None
    if st is not None:
        st.wait_stream(torch.cuda.current_stream())
    with (torch.cuda.stream(st) if st is not None else contextlib.nullcontext()):
        big.add_(1.0)                       # some queued work ahead of the copy
        g2 = torch.zeros_like(g)
        g2.copy_(g)                         # zeros until this lands: a gradient the check refuses
        rm.descent_device(g2, 2, n_values=n)
        out = torch.zeros(F.b64_len(21940) + 32, dtype=torch.uint8, device="cuda")
        k = rm.getModelParametersNative_device(rm.modelsSize() - 1, out)
        text = out[:k].clone()              # the caller's next use of the output, same stream
        torch.cuda.current_stream().synchronize()
    hm.descentNative(bytes(s["merged0"]), 8, 2)
    _same(rm, hm)
    assert text.cpu().numpy().tobytes() == hm.getModelParametersNative(hm.modelsSize() - 1)
    rm.close()
    hm.close()
