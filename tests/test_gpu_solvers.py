"""The server optimizers on the GPU (adagrad, rmsprop, adam; commonLib/cppNN/solver.h:97-195):
the device arithmetic's digests, the stateless step at the layouts where a thread-per-element
kernel can go wrong, edge values through the kernel, the host and the resident model against
each other, against the NumPy restatement (tests/solver_ref.py, proven equal to the reference's
recorded bits in tests/test_solver_math.py) and against the reference's network-level
recording, the unchanged default, the refusals and the JNI shim's FLEET_SOLVER."""
import json
import os

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import MNIST

import solver_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NEW = R.SOLVERS[1:]
MNIST_FC = slice(72, 82)
W_BLOCKS = [s for s in MNIST.w_sizes if s]
B_BLOCKS = [8, 16, 48, 10]
f = np.float32


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(HERE, "golden", "solver_ref.npz"))


@pytest.fixture(scope="module")
def seeded():
    return np.load(os.path.join(HERE, "golden", "model_mnist_seeded.npz"))


@pytest.fixture(scope="module")
def grads(oracle):
    """(merged text, decodeFloat of it) of the reference's network-level recording"""
    return R.network_gradients(MNIST, oracle)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, f).copy()).cuda()


def _eq(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


# -- digests -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", [25, 26, 27, 28, 29, 30])
def test_device_arithmetic_digest(codec, fn):
    """sqrtf, adam's binary64 denominator, its numerator's division and a / b, with the x86 NaN
    rule, over all 2^32 inputs (fn 28: 2^32 hashed pairs and the edge grid) equal the CPU's."""
    want = json.load(open(os.path.join(HERE, "golden", "solver_digests.json")))
    assert f"{codec.selftest_digest(fn):016x}" == want[f"fn{fn}"]


def test_digest_range(codec):
    with pytest.raises(F.FleetError):
        codec.selftest_digest(31)


# -- the stateless step ------------------------------------------------------------------------

LAYOUTS = {
    "w1": R.GradLayout((1,), (3,), (0,)),
    "w255": R.GradLayout((255,), (3,), (0,)),
    "w256": R.GradLayout((256,), (3,), (0,)),
    "w257": R.GradLayout((257,), (0, 5), (1,)),
    "w513": R.GradLayout((513,), (2,), ()),
    # boundaries inside a 256-thread block, an absent (though sized) W between present ones,
    # fc and non-fc bias blocks, a bias block of size 0
    "blocks": R.GradLayout((100, 0, 77, 300, 41), (7, 0, 5, 10), (2, 3), absent=(2,)),
    "mnist": MNIST,
}


def _run_stateless(codec, solver, lay, steps=3, seed=5):
    import torch
    r = np.random.RandomState(seed)
    nw = lay.n_weights
    w = r.normal(0, 0.3, nw).astype(f)
    b = r.normal(0, 0.3, lay.n_fc_bias).astype(f)
    g1, g2 = np.zeros(nw, f), (np.zeros(nw, f) if solver == "adam" else None)
    dw, d1, db = _dev(w), _dev(g1), _dev(b)
    d2 = _dev(g2) if g2 is not None else None
    hw, h1, h2, hb = w, g1, g2, b
    for i in range(steps):
        vals = (r.normal(0, 1, lay.n_flat) * 10.0 ** r.uniform(-5, 1, lay.n_flat)).astype(f)
        g = R.layout_gradient(lay, vals) if not isinstance(lay, R.GradLayout) else lay.gradient(vals)
        L = f(0.05 / (i + 1))
        w, g1, g2, b = R.descent(solver, lay, w, g1, g2, b, g, L)
        codec.descent_solver_device(solver, dw, d1, d2, db, _dev(g), lay, float(L))
        torch.cuda.synchronize()
        hw, h1, h2, hb = codec.descent_solver(solver, hw, h1, h2, hb, g, lay, float(L))
        for name, want, dev, host in (("w", w, dw, hw), ("g1", g1, d1, h1), ("g2", g2, d2, h2), ("fc_bias", b, db, hb)):
            if want is None:
                continue
            assert _eq(dev.cpu().numpy(), want), (solver, i, name, "device form")
            assert _eq(host, want), (solver, i, name, "host form")


@pytest.mark.parametrize("lay", list(LAYOUTS))
@pytest.mark.parametrize("solver", NEW)
def test_stateless_step(codec, solver, lay):
    _run_stateless(codec, solver, LAYOUTS[lay])


def test_stateless_sgd_is_fleet_descent(codec):
    import torch
    lay = LAYOUTS["blocks"]
    r = np.random.RandomState(9)
    w, b = r.normal(0, 1, lay.n_weights).astype(f), r.normal(0, 1, lay.n_fc_bias).astype(f)
    g = lay.gradient(r.normal(0, 1, lay.n_flat).astype(f))
    a_w, a_b, b_w, b_b = _dev(w), _dev(b), _dev(w), _dev(b)
    codec.descent_device(a_w, a_b, _dev(g), lay, 0.03)
    codec.descent_solver_device("sgd", b_w, None, None, b_b, _dev(g), lay, 0.03)
    torch.cuda.synchronize()
    assert _eq(a_w.cpu().numpy(), b_w.cpu().numpy()) and _eq(a_b.cpu().numpy(), b_b.cpu().numpy())
    hw, _, _, hb = codec.descent_solver(0, w, None, None, b, g, lay, 0.03)
    ow, ob = codec.descent(w, b, g, lay, 0.03)
    assert _eq(hw, ow) and _eq(hb, ob) and _eq(hw, a_w.cpu().numpy())


# -- edge values through the kernel ----------------------------------------------------------

def _edge_session(codec, solver, w, g1, g2, ds, L=0.05):
    import torch
    n = len(w)
    lay = R.GradLayout((n,), (), ())
    dw, d1 = _dev(w), _dev(g1)
    d2 = _dev(g2) if solver == "adam" else None
    out = []
    for d in ds:
        codec.descent_solver_device(solver, dw, d1, d2, None, _dev(lay.gradient(d)), lay, L)
        torch.cuda.synchronize()
        out.append((dw.cpu().numpy(), d1.cpu().numpy(), d2.cpu().numpy() if d2 is not None else None))
    return out


@pytest.mark.parametrize("solver", NEW)
def test_edge_values_without_nan_inputs(codec, solver, ref):
    """The class-level recording of the reference through the kernel: +-0, denormal gradients,
    squares that overflow, +-inf gradients and weights; every NaN is 0xFFC00000 and the next
    step starts from that NaN state. Then the session continued on denormal state."""
    w0, d = R.class_inputs()
    zero = np.zeros_like(w0)
    got = _edge_session(codec, solver, w0, zero, zero, d, float(R.CLASS_L))
    for i, (w, g1, g2) in enumerate(got):
        assert _eq(w, ref[f"a_{solver}_w"][i]) and _eq(g1, ref[f"a_{solver}_g1"][i]), (solver, i)
        if solver == "adam":
            assert _eq(g2, ref["a_adam_g2"][i])
        nan = np.isnan(w)
        assert (R.bits(w)[nan] == 0xFFC00000).all()
    assert np.isnan(got[-1][0]).any()
    cw0, cg1, cg2, cd = R.continued_inputs()
    s1, s2 = R.continued_state(solver, cg1, cg2)
    got = _edge_session(codec, solver, cw0, s1, s2, cd, float(R.CONT_L))
    for i, (w, g1, g2) in enumerate(got):
        assert _eq(w, ref[f"c_{solver}_w"][i]) and _eq(g1, ref[f"c_{solver}_g1"][i]), (solver, i)
        if solver == "adam":
            assert _eq(g2, ref["c_adam_g2"][i])


@pytest.mark.parametrize("solver", NEW)
def test_edge_values_eps_dominates_and_nan_inputs(codec, solver):
    n = 600
    r = np.random.RandomState(3)
    # state so small that eps dominates the denominator
    w = r.normal(0, 1, n).astype(f)
    g1 = (10.0 ** r.uniform(-30, -20, n)).astype(f)
    g2 = (10.0 ** r.uniform(-30, -20, n)).astype(f)
    ds = [(10.0 ** r.uniform(-14, -10, n) * r.choice([-1, 1], n)).astype(f) for _ in range(2)]
    got = _edge_session(codec, solver, w, g1, g2, ds)
    ew, e1, e2 = w, g1, g2
    for i, d in enumerate(ds):
        ew, e1, e2 = R.increment_w(solver, ew, d, e1, e2, f(0.05))
        assert _eq(got[i][0], ew) and _eq(got[i][1], e1), (solver, i)
        assert not np.array_equal(ew, w)
    # NaN among gradient, weights and state: positions and every non-NaN value, no payload
    w = r.normal(0, 1, n).astype(f)
    g1, g2 = np.abs(r.normal(0, 1, n)).astype(f), np.abs(r.normal(0, 1, n)).astype(f)
    d = r.normal(0, 1, n).astype(f)
    nan = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffabcdef], np.uint32).view(f)
    w[5:9], d[20:24], g1[40:44], g2[60:64] = nan, nan, nan, nan
    w[100], d[100] = nan[2], nan[3]
    got = _edge_session(codec, solver, w, g1, g2, [d, d])
    ew, e1, e2 = w, g1, g2
    for i in range(2):
        ew, e1, e2 = R.increment_w(solver, ew, d, e1, e2, f(0.05))
        assert R.same_but_nan_payloads(got[i][0], ew) and R.same_but_nan_payloads(got[i][1], e1), (solver, i)
        if solver == "adam":
            assert R.same_but_nan_payloads(got[i][2], e2)
    assert np.isnan(ew).sum() >= 9


# -- the models ------------------------------------------------------------------------------

def _g(x):
    x = f(x)
    if np.isnan(x):
        return "-nan" if R.bits([x])[0] >> 31 else "nan"
    return "%g" % float(x)


def _lines(values, blocks):
    out, o = [], 0
    for n in blocks:
        out.append("".join(_g(v) + " " for v in values[o:o + n]) + "\n")
        o += n
    return "".join(out)


def _text(seeded, codec, mode):
    """the seeded MNIST model as a getParams text of DISTILLATION_MODE `mode`"""
    init = bytes(seeded["text"])
    if mode:
        return init
    hm = F.Model(codec, init, distillation_mode=1)
    w, b = hm.export(-1)
    hm.close()
    cut = init.index(b" \n%d\n" % len(w)) + 2
    lines = init[:cut].split(b"\n")
    head = b"\n".join(lines[: len(lines) - 1 - len(B_BLOCKS)]) + b"\n"
    return head + _lines(b, B_BLOCKS).encode() + _lines(w, W_BLOCKS).encode()


def _merged(codec, upload):
    """(merged text, merged_f32 on the device) of a real Codec.update_device over two uploads"""
    import torch
    ups = [upload, upload]
    length = len(ups[0])
    pitch = (length + 15) // 16 * 16 + 16
    d = torch.zeros((2, pitch), dtype=torch.uint8, device="cuda")
    for c, u in enumerate(ups):
        d[c, :length] = torch.from_numpy(np.frombuffer(u, np.uint8).copy()).cuda()
    groups = (F.b64_count(length) + 2) // 3
    out = torch.zeros(16 * groups + 16, dtype=torch.uint8, device="cuda")
    f32 = torch.zeros(3 * groups + 3, dtype=torch.float32, device="cuda")
    codec.update_device(d, length, [1.0, 0.5], MNIST.header_positions(), out, f32)
    torch.cuda.synchronize()
    return out[:length].cpu().numpy().tobytes(), f32, F.b64_count(length)


@pytest.fixture(scope="module")
def merged(codec, grads):
    return [_merged(codec, t) for t, _ in grads]


def _models(codec, text, mode, solver):
    return (F.Model(codec, text, distillation_mode=mode, solver=solver),
            F.ResidentModel(codec, text, distillation_mode=mode, max_versions=3, solver=solver))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("solver", NEW)
def test_models_session(codec, seeded, merged, solver, mode):
    """initUpdater with a schedule that changes the rate, three descents (the host model from
    the merged text, the resident one from merged_f32 on the device): both models equal each
    other and the restatement in weights, both state rows and every text; versions carry no state."""
    text = _text(seeded, codec, mode)
    hm, rm = _models(codec, text, mode, solver)
    sgd = F.Model(codec, text, distillation_mode=mode)
    assert hm.solver == rm.solver == solver and sgd.solver == "sgd"
    base = rm.stats()["resident_bytes"]
    plain = F.ResidentModel(codec, text, distillation_mode=mode, max_versions=3)
    rows = 2 if solver == "adam" else 1
    assert base - plain.stats()["resident_bytes"] == 4 * rows * hm.shape()[0]
    plain.close()
    for m in (hm, rm, sgd):
        m.initUpdater(R.NET_LRS)
    w, b = hm.export(-1)
    g1 = np.zeros_like(w)
    g2 = np.zeros_like(w) if solver == "adam" else None
    assert _eq(hm.solver_state(0), g1) and _eq(rm.solver_state(0), g1)
    first_text = hm.getParametersNative(0)
    for i, (mtext, f32, n) in enumerate(merged):
        hm.descentNative(mtext, 8, 2)
        sgd.descentNative(mtext, 8, 2)
        rm.descent_device(f32, 2, n_values=n)
        g = codec.decode_floats(mtext)
        w, g1, g2, fcb = R.descent(solver, MNIST, w, g1, g2, b[MNIST_FC], g, f(R.NET_LRS[i]), R.SESSION)
        b[MNIST_FC] = fcb
        for m in (hm, rm):
            mw, mb = m.export(-1)
            assert _eq(mw, w) and _eq(mb, b), (solver, mode, i, type(m).__name__)
            assert _eq(m.solver_state(0), g1)
            if solver == "adam":
                assert _eq(m.solver_state(1), g2)
            else:
                with pytest.raises(F.FleetError):
                    m.solver_state(1)
        # versions, priorities and the ring behave as with sgd
        assert hm.modelsSize() == rm.modelsSize() == sgd.modelsSize() == min(i + 2, 2)
        assert hm.getCurrEpoch() == rm.getCurrEpoch() == sgd.getCurrEpoch() == i + 1
        assert hm.getLrate() == rm.getLrate() == sgd.getLrate()
        for v in range(hm.modelsSize()):
            assert hm.getParametersNative(v) == rm.getParametersNative(v)
            assert hm.getModelParametersNative(v) == rm.getModelParametersNative(v)
            assert hm.version_id(v) == rm.version_id(v) == sgd.version_id(v)
            (hw, hb), (rw, rb) = hm.export(v), rm.export(v)
            assert _eq(hw, rw) and _eq(hb, rb)
        if i == 0:  # the older version's text is the one initUpdater pushed: it saw no solver
            assert hm.getParametersNative(0) == first_text == sgd.getParametersNative(0)
        assert hm.getParametersNative(hm.modelsSize() - 1) != sgd.getParametersNative(sgd.modelsSize() - 1)
    for m in (hm, rm, sgd):
        m.close()


@pytest.mark.parametrize("solver", NEW)
def test_models_equal_reference_network_recording(codec, seeded, ref, grads, solver):
    """DISTILLATION_MODE=0 models stepped with the recording's own gradients and rates equal the
    reference's mojo::network(solver) after every step (solver_ref.npz part b)."""
    import torch
    text = _text(seeded, codec, 0)
    hm, rm = _models(codec, text, 0, solver)
    for m in (hm, rm):
        m.initUpdater(R.NET_LRS)
    w0, b0 = hm.export(-1)
    assert _eq(w0, ref["b_w0"]) and _eq(b0, ref["b_b0"])
    for i, (gtext, g) in enumerate(grads):
        assert _eq(codec.decode_floats(gtext), g)
        hm.descentNative(gtext, 8, 1)
        rm.descent_device(_dev(g), 1)
        torch.cuda.synchronize()
        for m in (hm, rm):
            w, b = m.export(-1)
            assert _eq(w[::R.NET_STRIDE], ref[f"b_{solver}_w_sub"][i]) and _eq(b, ref[f"b_{solver}_b"][i]), (solver, i)
    for m in (hm, rm):
        assert _eq(m.export(-1)[0], ref[f"b_{solver}_w_last"])
        m.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_default_is_unchanged(codec, seeded, merged, mode):
    text = _text(seeded, codec, mode)
    for cls, kw in ((F.Model, {}), (F.ResidentModel, {"max_versions": 3})):
        a, b = cls(codec, text, distillation_mode=mode, **kw), cls(codec, text, distillation_mode=mode, solver="sgd", **kw)
        c = cls(codec, text, distillation_mode=mode, **kw)
        c.set_solver("adam")
        c.set_solver("sgd")  # back before the first descent
        for m in (a, b, c):
            m.initUpdater(R.NET_LRS)
            for mtext, _, _ in merged[:2]:
                m.descentNative(mtext, 8, 2)
        for m in (b, c):
            assert m.solver == "sgd"
            for v in range(a.modelsSize()):
                assert a.getParametersNative(v) == m.getParametersNative(v)
                assert a.getModelParametersNative(v) == m.getModelParametersNative(v)
            assert _eq(a.export(-1)[0], m.export(-1)[0]) and _eq(a.export(-1)[1], m.export(-1)[1])
            with pytest.raises(F.FleetError):
                m.solver_state(0)
        for m in (a, b, c):
            m.close()


# -- refusals --------------------------------------------------------------------------------

def test_refusals(codec, seeded, merged, grads):
    import torch
    text = _text(seeded, codec, 1)
    with pytest.raises(ValueError):
        codec.descent_solver_device("adamw", None, None, None, None, None, MNIST, 0.1)
    with pytest.raises(F.FleetError):
        codec.descent_solver_device(7, _dev(np.zeros(4)), None, None, None, _dev(np.zeros(8)), R.GradLayout((4,), (), ()), 0.1)
    lay = R.GradLayout((4,), (), ())
    w, g1 = _dev(np.ones(4)), _dev(np.zeros(4))
    with pytest.raises(F.FleetError):  # adam without g2
        codec.descent_solver_device("adam", w, g1, None, None, _dev(lay.gradient(np.ones(4, f))), lay, 0.1)
    with pytest.raises(F.FleetError):  # rmsprop without g1
        codec.descent_solver_device("rmsprop", w, None, None, None, _dev(lay.gradient(np.ones(4, f))), lay, 0.1)
    with pytest.raises(F.FleetError):
        codec.descent_solver("adam", np.ones(4, f), np.zeros(4, f), None, np.zeros(0, f), lay.gradient(np.ones(4, f)), lay, 0.1)
    torch.cuda.synchronize()
    assert _eq(w.cpu().numpy(), np.ones(4)) and _eq(g1.cpu().numpy(), np.zeros(4))
    for cls, kw in ((F.Model, {}), (F.ResidentModel, {"max_versions": 1})):
        with pytest.raises(F.FleetError):
            cls(codec, text, solver="nadam", **kw)
        m = cls(codec, text, solver="adam", **kw)
        with pytest.raises(F.FleetError):
            m.set_solver("momentum")
        assert m.solver == "adam"
        m.initUpdater(R.NET_LRS)
        before = m.export(-1), m.solver_state(0), m.solver_state(1), m.getCurrEpoch(), m.modelsSize()

        def unchanged():
            now = m.export(-1), m.solver_state(0), m.solver_state(1), m.getCurrEpoch(), m.modelsSize()
            return (_eq(now[0][0], before[0][0]) and _eq(now[0][1], before[0][1]) and _eq(now[1], before[1])
                    and _eq(now[2], before[2]) and now[3:] == before[3:])
        # a gradient whose header is wrong (a block size changed; a count that is no integer)
        for pos, val in ((1, 201.0), (0, 6.5)):
            bad = grads[0][1].copy()
            bad[pos] = val
            with pytest.raises(F.LayoutError):
                m.descentNative(codec.encode_floats(bad), 8, 1)
            assert unchanged()
            if cls is F.ResidentModel:
                with pytest.raises(F.LayoutError):
                    m.descent_device(_dev(bad), 1)
                assert unchanged()
        with pytest.raises(F.Base64Error):
            m.descentNative(b"abc", 8, 1)
        assert unchanged()
        if cls is F.ResidentModel:
            with pytest.raises(F.FleetError):  # it would keep more versions than the model holds
                m.descentNative(merged[0][0], 8, 2)
            assert unchanged()
        m.descentNative(merged[0][0], 8, 1)
        assert not unchanged()
        with pytest.raises(F.FleetError):  # after a descent
            m.set_solver("rmsprop")
        assert m.solver == "adam" and np.any(m.solver_state(0) != 0)
        if cls is F.ResidentModel:
            # DISTILLATION_MODE=1 with a weight left non-finite: the version copy fails with cnn
            # stepped and the epoch advanced, as with sgd; the state is advanced like cnn
            g = grads[1][1].copy()
            g[5] = np.inf
            e, c, s0 = m.getCurrEpoch(), m.modelsSize(), m.solver_state(0)
            with pytest.raises(F.FleetError):
                m.descent_device(_dev(g), 1)
            assert m.getCurrEpoch() == e + 1 and m.modelsSize() == c and not _eq(m.solver_state(0), s0)
            assert np.isnan(m.export(-1)[0][3]) and np.isinf(m.solver_state(1)[3])
        m.close()


# -- the JNI shim ------------------------------------------------------------------------------

def test_shim_reads_fleet_solver(codec, seeded, merged, monkeypatch):
    import jnifake as J
    from test_jni_shim import check_rules, load
    L = load()
    env = J.env()
    text = bytes(seeded["text"])
    up = "Java_apps_cppNN_CppNNUpdater_"

    def session():
        getattr(L, up + "fetchParamsNative")(env, None, J.new_bytes(text))
        getattr(L, up + "initUpdater")(env, None, J.new_doubles(R.NET_LRS), 1, 0.0, 0.0)
        for mtext, _, _ in merged[:2]:
            getattr(L, up + "descentNative")(env, None, J.new_bytes(mtext), 8, 2)
        n = getattr(L, up + "modelsSize")(env, None)
        return [J.read_bytes(getattr(L, up + "getParametersNative")(env, None, v)) for v in range(n)]

    def model(solver):
        m = F.Model(codec, text, distillation_mode=1, solver=solver)
        m.initUpdater(R.NET_LRS)
        for mtext, _, _ in merged[:2]:
            m.descentNative(mtext, 8, 2)
        out = [m.getParametersNative(v) for v in range(m.modelsSize())]
        m.close()
        return out

    J.begin()
    monkeypatch.delenv("FLEET_SOLVER", raising=False)
    assert session() == model("sgd")
    monkeypatch.setenv("FLEET_SOLVER", "adam")
    got = session()
    assert got == model("adam") and got != model("sgd")
    # an unknown name fails the native: the text is not loaded, the earlier model stays
    monkeypatch.setenv("FLEET_SOLVER", "adamax")
    getattr(L, up + "fetchParamsNative")(env, None, J.new_bytes(text))
    assert [J.read_bytes(getattr(L, up + "getParametersNative")(env, None, v)) for v in range(2)] == got
    monkeypatch.delenv("FLEET_SOLVER")
    assert session() == model("sgd")
    check_rules(J)
