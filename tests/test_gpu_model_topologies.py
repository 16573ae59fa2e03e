"""The model natives beyond the MNIST network's one trailing fc layer (tests/model_nets.py):
fleet_amd.Model and ResidentModel, their solver steps, the text emitters and the ledger
staging on networks with three fully-connected layers behind a non-fc bias block (fc3), with
an fc bias block across a 256-thread block (fc3_wide) and with a non-fc block between two fc
blocks (fc_mid). fc3 against the reference's own sessions (tests/golden/session_fc3.npz, whose
conditions tests/test_model_nets_inputs.py proves on the CPU); every net against the
restatements (oracle.descent, solver_ref.descent, the oracle's dictionary, libc's '%g' and
strtof). Bit equality throughout."""
import os

import numpy as np
import pytest

import fleet_amd as F

import model_nets as N
import solver_ref as R
from test_gpu_resident_model import _bits, _decode_device, _same, _same_texts, _snapshot, _unchanged

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
f = np.float32
NEW = R.SOLVERS[1:]


def _eq(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def fc3():
    z = np.load(os.path.join(HERE, "golden", N.GOLDEN["fc3"]))
    return {ses: {k[len(ses) + 1:]: z[k] for k in z.files if k.startswith(ses + "_")} for ses in N.SESSIONS["fc3"]}


@pytest.fixture(scope="module")
def nets(oracle):
    """per net: seeded weights and biases as a model reads them from its mode-1 text, the
    texts of both modes, two merged gradients (text, decodeFloat of it)"""
    out = {}
    for name, net in N.NETS.items():
        w0, b0 = net.seeded(31 + len(name))
        dims = list(net.dims)
        w = oracle.read_weights_section(oracle.weights_section(oracle.quantize(w0, dims), dims), dims)
        b = N.roundtrip(b0)
        out[name] = {"net": net, "w": w, "b": b, "text": {1: net.text(1, w0, b0, oracle), 0: net.text(0, w, b)},
                     "grads": R.network_gradients(net.layout, oracle, steps=2)}
    return out


def _step(m, text, device, codec, stale=2):
    if device:
        g, n = _decode_device(codec, text)
        m.descent_device(g, stale, n_values=n)
    else:
        m.descentNative(bytes(text), 8, stale)


def _models(codec, text, mode, solver="sgd", max_versions=3):
    return (F.Model(codec, text, distillation_mode=mode, solver=solver),
            F.ResidentModel(codec, text, distillation_mode=mode, max_versions=max_versions, solver=solver))


def _version_of(oracle, mode, w, b):
    """descentNative's model copy of cnn, restated"""
    if not mode:
        return N.roundtrip(w), N.roundtrip(b)
    d, idx = oracle.dictionary(w)
    return N.roundtrip(d)[idx], N.roundtrip(b)


def _a20_device(rm, v, size):
    import torch
    out = torch.zeros(size + 32, dtype=torch.uint8, device="cuda")
    n = rm.getModelParametersNative_device(v, out)
    torch.cuda.current_stream().synchronize()
    return out[:n].cpu().numpy().tobytes()


# -- a. the reference's sessions, DISTILLATION_MODE=1 ----------------------------------------

@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("ses", N.SESSIONS["fc3"])
def test_reference_session_mode1(codec, oracle, fc3, ses, device_form):
    s = fc3[ses]
    hm, rm = _models(codec, bytes(s["init"]), 1)
    for m in (hm, rm):
        m.initUpdater(s["lrates"])
        assert m.shape() == (N.FC3.n_w, N.FC3.n_b, N.FC3.edges, len(N.FC3.layers))
        assert m.modelsSize() == 1 and m.getCurrEpoch() == 0

    def check(state):
        newest = rm.modelsSize() - 1
        for m in (hm, rm):
            assert m.getParametersNative(newest) == bytes(s[f"newest_text{state}"]), (state, type(m).__name__)
            assert m.getParametersNative(0) == bytes(s[f"oldest_text{state}"]), (state, type(m).__name__)
        for v, key in ((newest, "newest"), (0, "oldest")):
            want = oracle.encode_floats(s[f"{key}_params{state}"])
            assert hm.getModelParametersNative(v) == want and rm.getModelParametersNative(v) == want, (state, key)
            assert _a20_device(rm, v, len(want)) == want, (state, key)
            w, b = rm.export(v)
            assert _eq(np.concatenate([np.tile(b, N.FC3.edges), w]), s[f"{key}_params{state}"]), (state, key)
        _same(rm, hm)
        _same_texts(rm, hm)
    check(0)
    for i in range(N.STEPS):
        hm.descentNative(bytes(s[f"merged{i}"]), int(s["batch"]), int(s["stale"]))
        _step(rm, s[f"merged{i}"], device_form, codec, int(s["stale"]))
        check(i + 1)
    assert rm.modelsSize() == hm.modelsSize() == int(s["n_models"]) and rm.getCurrEpoch() == N.STEPS
    assert rm.getLrate() == hm.getLrate() == float(f(s["lrates"][2]))
    rm.close()
    hm.close()


# -- b, e. the same gradients on DISTILLATION_MODE=0 texts; fc_mid ------------------------------

def _mode0_session(codec, oracle, net, w, b, merged, lrates, device_form):
    """both models on the net's mode-0 text: equal to each other, their lines to '%g' by block,
    cnn to oracle.descent, every version to the round trip of the cnn it copied"""
    lay, fc = net.layout, net.fc_mask()
    text = net.text(0, w, b)
    head = N.header(net.layers)
    hm, rm = _models(codec, text, 0)
    for m in (hm, rm):
        m.initUpdater(lrates)
        assert m.shape()[:3] == (net.n_w, net.n_b, net.edges)
    w, b = N.roundtrip(w), N.roundtrip(b)        # what a model reads from the text
    b_first = b.copy()
    assert _eq(hm.export(-1)[0], w) and _eq(hm.export(-1)[1], b)
    versions = [_version_of(oracle, 0, w, b)]
    _same(rm, hm)
    _same_texts(rm, hm)
    for i, mtext in enumerate(merged):
        hm.descentNative(bytes(mtext), 8, 2)
        _step(rm, mtext, device_form, codec)
        g = oracle.decode_floats(bytes(mtext))
        w, b[fc] = oracle.descent(w, b[fc], g, lay.w_present(), lay.fc_flags(), f(lrates[i]))
        versions = (versions + [_version_of(oracle, 0, w, b)])[-2:]
        _same(rm, hm)
        _same_texts(rm, hm)
        for m in (hm, rm):
            cw, cb = m.export(-1)
            assert _eq(cw, w) and _eq(cb, b), (net.name, i, type(m).__name__)
            assert _eq(cb[~fc], b_first[~fc])                      # the non-fc biases never move in cnn
            for sl in net.fc_slices():
                assert (_bits(cb[sl]) != _bits(b_first[sl])).any(), (net.name, i, sl)
            assert m.modelsSize() == len(versions)
            for v, (vw, vb) in enumerate(versions):
                ew, eb = m.export(v)
                assert _eq(ew, vw) and _eq(eb, vb), (net.name, i, v, type(m).__name__)
                assert m.getParametersNative(v) == head + N.lines(eb, net.b_blocks) + N.lines(ew, net.w_blocks)
    rm.close()
    hm.close()


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("ses", N.SESSIONS["fc3"])
def test_session_gradients_mode0(codec, oracle, fc3, ses, device_form):
    s = fc3[ses]
    hm = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    w, b = hm.export(-1)
    hm.close()
    _mode0_session(codec, oracle, N.FC3, w, b, [s[f"merged{i}"] for i in range(N.STEPS)], s["lrates"], device_form)


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("name", ["fc3_wide", "fc_mid"])
def test_other_nets_mode0(codec, oracle, nets, name, device_form):
    n = nets[name]
    _mode0_session(codec, oracle, n["net"], n["w"], n["b"], [t for t, _ in n["grads"]], R.NET_LRS, device_form)


@pytest.mark.parametrize("name", ["fc3_wide", "fc_mid"])
def test_other_nets_mode1_version_copy(codec, oracle, nets, name):
    """one sgd step in mode 1: cnn is oracle.descent's, the version the oracle's first-occurrence
    dictionary of it, round-tripped; the a20 text is the oracle's encoding of that version"""
    n = nets[name]
    net, lay, fc = n["net"], n["net"].layout, n["net"].fc_mask()
    hm, rm = _models(codec, n["text"][1], 1)
    for m in (hm, rm):
        m.initUpdater(R.NET_LRS)
    assert _eq(hm.export(-1)[0], n["w"]) and _eq(hm.export(-1)[1], n["b"])
    mtext, g = n["grads"][0]
    hm.descentNative(mtext, 8, 2)
    _step(rm, mtext, True, codec)
    w, b = n["w"].copy(), n["b"].copy()
    w, b[fc] = oracle.descent(w, b[fc], g, lay.w_present(), lay.fc_flags(), f(R.NET_LRS[0]))
    vw, vb = _version_of(oracle, 1, w, b)
    want = oracle.encode_floats(np.concatenate([np.tile(vb, net.edges), vw]))
    for m in (hm, rm):
        assert _eq(m.export(-1)[0], w) and _eq(m.export(-1)[1], b), type(m).__name__
        assert _eq(m.export(1)[0], vw) and _eq(m.export(1)[1], vb), type(m).__name__
        assert m.getModelParametersNative(1) == want
    assert _a20_device(rm, 1, len(want)) == want
    _same(rm, hm)
    _same_texts(rm, hm)
    rm.close()
    hm.close()


# -- c, e. the solvers -------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(N.NETS))
@pytest.mark.parametrize("solver", NEW)
def test_solvers(codec, oracle, nets, solver, name, mode):
    """two steps (the host model from the text, the resident one from the device): weights, both
    state rows and the fc biases at their offsets equal solver_ref.descent; the other biases are
    cnn's first ones, bit for bit"""
    n = nets[name]
    net, lay, fc = n["net"], n["net"].layout, n["net"].fc_mask()
    hm, rm = _models(codec, n["text"][mode], mode, solver)
    for m in (hm, rm):
        m.initUpdater(R.NET_LRS)
    w, b = n["w"].copy(), n["b"].copy()
    assert _eq(hm.export(-1)[0], w) and _eq(hm.export(-1)[1], b)
    g1 = np.zeros_like(w)
    g2 = np.zeros_like(w) if solver == "adam" else None
    for i, (mtext, g) in enumerate(n["grads"]):
        hm.descentNative(mtext, 8, 2)
        _step(rm, mtext, True, codec)
        w, g1, g2, fcb = R.descent(solver, lay, w, g1, g2, b[fc], g, f(R.NET_LRS[i]), R.SESSION)
        b[fc] = fcb
        for m in (hm, rm):
            mw, mb = m.export(-1)
            who = (solver, name, mode, i, type(m).__name__)
            assert _eq(mw, w), who
            for sl in net.fc_slices():
                assert _eq(mb[sl], b[sl]), who + (sl,)
                assert (_bits(mb[sl]) != _bits(n["b"][sl])).any(), who + (sl,)
            assert _eq(mb[~fc], n["b"][~fc]), who
            assert _eq(m.solver_state(0), g1), who
            if solver == "adam":
                assert _eq(m.solver_state(1), g2), who
        _same(rm, hm)
        _same_texts(rm, hm)
        if name != "fc3_wide" or not mode:      # (the wide net's mode-1 copy: test_other_nets_mode1_version_copy)
            vw, vb = _version_of(oracle, mode, w, b)
            newest = hm.modelsSize() - 1
            assert _eq(hm.export(newest)[0], vw) and _eq(hm.export(newest)[1], vb), (solver, name, mode, i)
    rm.close()
    hm.close()


# -- d. gradients whose blocks are split otherwise than the model's layers -----------------------

SPLITS = {
    "fc_21_0_0": ((72, 0, 900, 63, 35), (288, 0, 100, 21, 0, 0)),
    "fc_0_16_5": ((72, 0, 900, 63, 35), (288, 0, 100, 0, 16, 5)),
    "fc_1_1_19": ((72, 0, 900, 63, 35), (288, 0, 100, 1, 1, 19)),
    "w_72_0_0_998_0": ((72, 0, 0, 998, 0), (288, 0, 100, 9, 7, 5)),
}


def _observables(m):
    return _snapshot(m), [m.getParametersNative(v) for v in range(m.modelsSize())], \
        [m.version_id(v) for v in range(m.modelsSize())], m.getLrate()


def _observables_unchanged(a, b):
    _unchanged(a[0], b[0])
    assert a[1:] == b[1:]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("split", list(SPLITS))
def test_blocks_split_otherwise(codec, oracle, nets, split, mode):
    """The sums are the model's (1070 weights, 21 fc biases), the blocks are not. Whatever the
    host model does, the resident model does from the text and from the device; a step equals
    oracle.descent over those blocks, a refusal changes nothing."""
    n = nets["fc3"]
    net, fc = n["net"], n["net"].fc_mask()
    ws, bs = SPLITS[split]
    lay = R.GradLayout(ws, bs, net.layout.fc_layers)
    r = np.random.RandomState(len(split))
    raw = lay.gradient((r.normal(0, 1, lay.n_flat) * 10.0 ** r.uniform(-4, -1, lay.n_flat)).astype(f))
    mtext = bytes(oracle.encode_floats(raw))
    g = oracle.decode_floats(mtext)
    assert len(g) == net.layout.n_up
    hm = F.Model(codec, n["text"][mode], distillation_mode=mode)
    rms = [F.ResidentModel(codec, n["text"][mode], distillation_mode=mode, max_versions=3) for _ in range(2)]
    for m in [hm] + rms:
        m.initUpdater(R.NET_LRS)
    before = [_observables(m) for m in [hm] + rms]
    code = None
    try:
        hm.descentNative(mtext, 8, 2)
    except F.FleetError as e:
        code = e.code
    for rm, device in zip(rms, (False, True)):
        if code is None:
            _step(rm, mtext, device, codec)
        else:
            with pytest.raises(F.FleetError) as e:
                _step(rm, mtext, device, codec)
            assert e.value.code == code, (split, device)
    if code is None:
        w, b = n["w"].copy(), n["b"].copy()
        w, b[fc] = oracle.descent(w, b[fc], g, net.layout.w_present(), net.layout.fc_flags(), f(R.NET_LRS[0]))
        vw, vb = _version_of(oracle, mode, w, b)
        for m in [hm] + rms:
            assert _eq(m.export(-1)[0], w) and _eq(m.export(-1)[1], b), (split, type(m).__name__)
            assert _eq(m.export(1)[0], vw) and _eq(m.export(1)[1], vb), (split, type(m).__name__)
            assert m.getCurrEpoch() == 1 and m.modelsSize() == 2
        for rm in rms:
            _same(rm, hm)
            _same_texts(rm, hm)
    else:
        assert code in (F.FLEET_ERR_LAYOUT, F.FLEET_ERR_ARG)
        for m, was in zip([hm] + rms, before):
            _observables_unchanged(was, _observables(m))
    for m in [hm] + rms:
        m.close()


# -- f. what consumes a model ------------------------------------------------------------------

def test_ledger_rows_and_norms(codec, oracle, fc3):
    s = fc3["a"]
    hm, rm = _models(codec, bytes(s["init"]), 1)
    for m in (rm, hm):
        m.initUpdater(s["lrates"])
        m.descentNative(bytes(s["merged0"]), 8, 2)
        m.descentNative(bytes(s["merged1"]), 8, 2)
    lr, lh = rm.kardam_ledger(3), hm.kardam_ledger(3)
    for v in range(rm.modelsSize()):
        vid = lr.stage_model(rm, v)
        assert vid == lh.stage_model(hm, v) == hm.version_id(v)
        assert _eq(lr.read_version(vid), lh.read_version(vid))
        assert _eq(lr.read_version(vid), oracle.decode_floats(hm.getModelParametersNative(v)))
    assert _eq(lr.read_version(rm.version_id(1)), oracle.decode_floats(oracle.encode_floats(s["newest_params2"])))
    ids = [rm.version_id(0), rm.version_id(1), rm.version_id(1)]
    a, b = lr.update(ids, [0, 1, 0]), lh.update(ids, [0, 1, 0])
    assert np.array_equal(a[2], b[2])
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(np.asarray(x, np.float64).view(np.uint64), np.asarray(y, np.float64).view(np.uint64))
    for x in (lr, lh, rm, hm):
        x.close()


def test_values_text_of_the_nets_blocks(codec, nets):
    import torch
    for name in ("fc3", "fc_mid"):
        n = nets[name]
        net = n["net"]
        assert codec.values_text(n["b"], list(net.b_blocks)) == N.lines(n["b"], net.b_blocks)
        assert codec.values_text(n["w"], list(net.w_blocks)) == N.lines(n["w"], net.w_blocks)
        row = torch.from_numpy(np.concatenate([n["w"], n["b"]])).cuda()
        blocks = list(net.w_blocks) + list(net.b_blocks)
        assert codec.values_text(row, blocks) == N.lines(np.concatenate([n["w"], n["b"]]), blocks)


def test_evaluation_and_client_gradients_refuse_the_net(codec, fc3):
    import torch
    from fleet_amd import client as K
    x, lab = np.zeros((4, 784), f), np.zeros(4, np.int32)
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    hm, rm = _models(codec, bytes(fc3["a"]["init"]), 1)
    for m in (hm, rm):
        m.initUpdater([0.1])
        with pytest.raises(F.FleetError) as e:
            m.evaluate(x, lab, version=-1)
        assert e.value.code == F.FLEET_ERR_ARG and "layer 0 is I1 input 12 12 2" in str(e.value), str(e.value)
    before = _snapshot(rm)
    with pytest.raises(F.FleetError) as e:
        rm.evaluate_device(dx, dl, version=0)
    assert e.value.code == F.FLEET_ERR_ARG and "layer 0 is I1" in str(e.value), str(e.value)
    with pytest.raises(F.FleetError) as e:
        K.resident_client_gradients_device(rm, -1, dx, dl, C=2, B=2)
    assert e.value.code == F.FLEET_ERR_ARG and "layer 0 is I1" in str(e.value), str(e.value)
    codec.check()  # nothing was launched that could have set the word
    _unchanged(before, _snapshot(rm))
    rm.close()
    hm.close()


# -- g. the allocation rule ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 0])
def test_no_allocation_after_warm_up(codec, fc3, nets, mode):
    s = fc3["a"]
    text = bytes(s["init"]) if mode else nets["fc3"]["text"][0]
    rm = F.ResidentModel(codec, text, distillation_mode=mode, max_versions=3)
    nw, nb, _, _ = rm.shape()
    assert (nw, nb) == (1070, 25)
    assert rm.stats()["resident_bytes"] == 4 * ((nw + nb + 63) // 64 * 64) * (3 + 2)
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
