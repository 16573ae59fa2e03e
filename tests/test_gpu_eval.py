"""The Driver's test() on the GPU (Driver/src/main/c++/cppNN_backend.cpp:53-75) against
tests/golden/eval_ref.npz, recorded from the reference's own network class: every entry
point, bit for bit, at the set sizes where the forward kernel's image groups and its
grid-stride walk can go wrong; index lists; the host and the resident model, also after a
step of each solver; the device path; the refusals; the edge inputs; the workspace."""
import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import MNIST

import eval_ref as R
import solver_ref as S

pytestmark = pytest.mark.gpu
f = np.float32


def _sizes():
    n = F.evaluate_block_images()
    out = []
    for b in (1, 2, n - 1, n, n + 1, 2 * n + 1, R.B_A):
        if b >= 1 and b not in out:
            out.append(b)
    return out


@pytest.fixture(scope="module")
def z():
    return R.load()


@pytest.fixture(scope="module")
def data():
    return R.images_a(), R.labels_a(), R.model_a()


@pytest.fixture(scope="module")
def dev(data):
    import torch
    x, lab, (w, b) = data
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return t(x), t(lab), t(w), t(b)


def _same(ev, c, B, contract=1, what=""):
    """an Evaluation against the first B images of a recorded case"""
    for got, want, name in ((ev.predictions, c["pred"][:B], "pred"), (ev.probabilities, c["p"][:B], "p"),
                            (ev.error, c["error"][B - 1], "error"), (ev.accuracy, c["accuracy"][B - 1], "accuracy")):
        bad = R.mismatch(contract, np.atleast_1d(got), np.atleast_1d(want))
        assert not bad, (what, B, name, bad)
    assert ev.correct == c["correct"][B - 1], (what, B)


# -- parity at the group and grid edges ----------------------------------------------------------

@pytest.mark.parametrize("B", _sizes())
def test_parity_with_the_reference(codec, z, data, dev, B):
    """pred, p, cost, error, accuracy and correct of the first B images, host and device forms"""
    import torch
    x, lab, (w, b) = data
    a = R.case(z, "a")
    _same(codec.evaluate(w, b, x[:B], lab[:B]), a, B, what="host")
    dx, dl, dw, db = dev
    out = {"costs": torch.empty(B, dtype=torch.float32, device="cuda"),
           "probs10": torch.empty(B, 10, dtype=torch.float32, device="cuda")}
    out = codec.evaluate_device(dw, db, dx[:B], dl[:B], out=out)
    codec.check()
    _same(F.evaluation_from_device(out), a, B, what="device")
    assert not R.mismatch(1, out["costs"].cpu().numpy(), a["cost"][:B])
    k = min(B, R.N_PROBS)
    assert not R.mismatch(1, out["probs10"].cpu().numpy()[:k], a["probs"][:k])


@pytest.mark.parametrize("grid", [1, 2])
def test_grid_stride_passes(codec, z, data, grid):
    """one image more than a pass of `grid` blocks covers, and a set of many passes"""
    x, lab, (w, b) = data
    a = R.case(z, "a")
    n = F.evaluate_block_images()
    with F.evaluate_grid_override(grid):
        for B in (grid * n + 1, 5 * grid * n + 2):
            _same(codec.evaluate(w, b, x[:B], lab[:B]), a, B, what=f"grid {grid}")


# -- index lists -----------------------------------------------------------------------------------

def test_permutation_gives_its_own_error(codec, z, data):
    x, lab, (w, b) = data
    a = R.case(z, "a")
    ev = codec.evaluate(w, b, x, lab, idx=R.PERM)
    assert R.bits(ev.error) == R.bits(z["a_perm_error"])[0] != R.bits(a["error"][-1])
    assert R.bits(ev.accuracy) == R.bits(z["a_perm_accuracy"])[0] and ev.correct == int(z["a_perm_correct"].reshape(-1)[0])
    assert np.array_equal(ev.predictions, a["pred"][R.PERM])
    assert not R.mismatch(1, ev.probabilities, a["p"][R.PERM])


def test_repeated_and_short_index_lists(codec, z, data):
    x, lab, (w, b) = data
    a = R.case(z, "a")
    for idx in ([7, 7, 7, 3, 7], [599], [5, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5, 599]):
        idx = np.array(idx, np.int32)
        ev = codec.evaluate(w, b, x, lab, idx=idx)
        assert np.array_equal(ev.predictions, a["pred"][idx])
        assert not R.mismatch(1, ev.probabilities, a["p"][idx])
        assert R.bits(ev.error) == R.bits(R.ordered_error(a["cost"][idx]))
        correct = int((a["pred"][idx] == lab[idx]).sum())
        assert ev.correct == correct and R.bits(ev.accuracy) == R.bits(R.accuracy_of(correct, len(idx)))


def test_index_out_of_range(codec, data, dev):
    import torch
    x, lab, (w, b) = data
    for bad in ([0, 600], [-1], [3, 2 ** 31 - 1]):
        with pytest.raises(F.FleetError) as e:
            codec.evaluate(w, b, x, lab, idx=np.array(bad, np.int32))
        assert e.value.code == F.FLEET_ERR_ARG
    dx, dl, dw, db = dev
    codec.evaluate_device(dw, db, dx[:16], dl[:16], idx_i32=torch.tensor([1, 16, 2], dtype=torch.int32, device="cuda"))
    with pytest.raises(F.FleetError) as e:
        codec.check()
    assert e.value.code == F.FLEET_ERR_ARG
    codec.check()  # the word is cleared


# -- the models ------------------------------------------------------------------------------------

def _models(codec, text, mode=1, solver="sgd"):
    return (F.Model(codec, text, distillation_mode=mode, solver=solver),
            F.ResidentModel(codec, text, distillation_mode=mode, max_versions=3, solver=solver))


def test_models_equal_the_text_level_recording(codec, z, data, dev):
    """cnn (version -1) is what cnn.read of the text holds, the newest version the server's copy of it"""
    x, lab, _ = data
    dx, dl, _, _ = dev
    hm, rm = _models(codec, R.seeded_text())
    for m in (hm, rm):
        with pytest.raises(ValueError):
            m.evaluate(x, lab)  # no version yet
        m.initUpdater(S.NET_LRS)
    B = 200
    for version, name in ((-1, "b_text"), (None, "b_copy"), (0, "b_copy")):
        c = R.case(z, name)
        _same(hm.evaluate(x[:B], lab[:B], version=version), c, B, what=f"host model {name}")
        _same(rm.evaluate(x[:B], lab[:B], version=version), c, B, what=f"resident model {name}")
        out = rm.evaluate_device(dx[:B], dl[:B], version=version)
        _same(F.evaluation_from_device(out), c, B, what=f"resident model, device {name}")
    _same(rm.evaluate(x, lab), R.case(z, "b_copy"), R.B_A, what="resident model, every image")
    for m in (hm, rm):
        with pytest.raises(F.FleetError) as e:
            m.evaluate(x[:4], lab[:4], version=1)
        assert e.value.code == F.FLEET_ERR_ARG
        m.close()


def test_mode_1_driver_view(codec, z, data):
    """The Driver evaluates the broadcast text: a Model of getParametersNative's text, its cnn"""
    x, lab, _ = data
    rm = F.ResidentModel(codec, R.seeded_text(), distillation_mode=1, max_versions=2)
    rm.initUpdater(S.NET_LRS)
    view = F.Model(codec, rm.getParametersNative(0), 1)
    c = R.case(z, "b_bcast")
    _same(view.evaluate(x[:200], lab[:200], version=-1), c, 200, what="driver view")
    w, b = view.export(-1)
    assert np.array_equal(R.bits(w), R.bits(z["b_bcast_w"])) and np.array_equal(R.bits(b), R.bits(z["b_bcast_b"]))
    assert R.bits(c["error"][199]) != R.bits(R.case(z, "b_copy")["error"][199])  # not the stored version's
    view.close()
    rm.close()


@pytest.mark.parametrize("solver", S.SOLVERS)
def test_after_a_step(codec, oracle, data, solver):
    """one descent: the host and the resident model evaluate to the same bits, other than before"""
    x, lab, _ = data
    B = 64
    gtext, _ = S.network_gradients(MNIST, oracle, steps=1)[0]
    hm, rm = _models(codec, R.seeded_text(), solver=solver)
    for m in (hm, rm):
        m.initUpdater([0.5])
    before = hm.evaluate(x[:B], lab[:B])
    for m in (hm, rm):
        m.descentNative(gtext, 8, 2)
    for version in (None, -1, 0):
        h, r = hm.evaluate(x[:B], lab[:B], version=version), rm.evaluate(x[:B], lab[:B], version=version)
        assert R.bits(h.error) == R.bits(r.error) and R.bits(h.accuracy) == R.bits(r.accuracy) and h.correct == r.correct
        assert np.array_equal(h.predictions, r.predictions) and not R.mismatch(1, h.probabilities, r.probabilities)
        if version == 0:  # the version initUpdater pushed is still what it was
            assert R.bits(h.error) == R.bits(before.error)
        else:
            assert R.bits(h.error) != R.bits(before.error)
            assert (R.bits(h.probabilities) != R.bits(before.probabilities)).any()
    hm.close()
    rm.close()


# -- the device path -------------------------------------------------------------------------------

def test_device_path_stream_padding_and_null_outputs(codec, z, data):
    import torch
    x, lab, (w, b) = data
    a = R.case(z, "a")
    B, Fp = 37, 800
    xp = np.full((B, Fp), np.nan, f)  # padding columns are never read
    xp[:, :784] = x[:B]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dx, dl = torch.from_numpy(xp).cuda(), torch.from_numpy(lab[:B].copy()).cuda()
        dw, db = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
        full = codec.evaluate_device(dw, db, dx, dl, stream=s.cuda_stream)
        bare = codec.evaluate_device(dw, db, dx, dl, out={"predictions": None, "probabilities": None}, stream=s.cuda_stream)
    s.synchronize()
    codec.check(s.cuda_stream)
    _same(F.evaluation_from_device(full), a, B, what="stream, F = 800")
    ev = F.evaluation_from_device(bare)
    assert ev.predictions is None and ev.probabilities is None
    assert R.bits(ev.error) == R.bits(a["error"][B - 1]) and ev.correct == a["correct"][B - 1]
    rm = F.ResidentModel(codec, R.seeded_text(), 1, max_versions=2)
    with torch.cuda.stream(s):
        out = rm.evaluate_device(dx, dl, version=-1, out={"probabilities": None}, stream=s.cuda_stream)
    s.synchronize()
    ev = F.evaluation_from_device(out)
    assert ev.probabilities is None
    c = R.case(z, "b_text")
    assert np.array_equal(ev.predictions, c["pred"][:B]) and R.bits(ev.error) == R.bits(c["error"][B - 1])
    rm.close()


# -- refusals --------------------------------------------------------------------------------------

def test_refusals(codec, data):
    x, lab, (w, b) = data
    for bad in (lambda: codec.evaluate(w[:-1], b, x[:4], lab[:4]),          # a wrong n_w
                lambda: codec.evaluate(w, b[:-1], x[:4], lab[:4]),
                lambda: codec.evaluate(w, b, x[:0], lab[:0]),                 # B = 0
                lambda: codec.evaluate(w, b, x[:4], lab[:4], idx=np.zeros(0, np.int32)),
                lambda: codec.evaluate(w, b, x[:4, :783], lab[:4])):          # F < 784
        with pytest.raises(F.FleetError) as e:
            bad()
        assert e.value.code == F.FLEET_ERR_ARG
    # models that are not the MNIST network: the same shapes and weights, another layer list
    text = R.seeded_text()
    for old, new, where in ((b"semi_stochastic_pool 3 3", b"max_pool 3 3", "P1"),
                            (b"convolution 5 48 1 elu", b"convolution 5 48 1 relu", "C2"),
                            (b"fully_connected 10 softmax", b"fully_connected 10 tanh", "FC2")):
        assert text.count(old) == 1
        hm, rm = _models(codec, text.replace(old, new))
        for m in (hm, rm):
            with pytest.raises(F.FleetError) as e:
                m.evaluate(x[:4], lab[:4], version=-1)
            assert e.value.code == F.FLEET_ERR_ARG and where in str(e.value), str(e.value)
            m.close()
    codec.check()  # nothing was launched that could have set the word


# -- edges -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c[0] for c in R.edge_cases()])
def test_edges(codec, z, case):
    import torch
    name, contract, w, b, x, lab = next(c for c in R.edge_cases() if c[0] == case)
    c = R.case(z, name)
    B = len(lab)
    _same(codec.evaluate(w, b, x, lab), c, B, contract, what=name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = codec.evaluate_device(t(w), t(b), t(x), t(lab), out={
        "costs": torch.empty(B, dtype=torch.float32, device="cuda"),
        "probs10": torch.empty(B, 10, dtype=torch.float32, device="cuda")})
    codec.check()
    _same(F.evaluation_from_device(out), c, B, contract, what=name + " device")
    assert not R.mismatch(contract, out["costs"].cpu().numpy(), c["cost"])
    assert not R.mismatch(contract, out["probs10"].cpu().numpy(), c["probs"])


# -- allocation ------------------------------------------------------------------------------------

def test_workspace_is_allocated_once(codec, data, dev):
    x, lab, _ = data
    dx, dl, _, _ = dev
    rm = F.ResidentModel(codec, R.seeded_text(), 1, max_versions=2)
    base = rm.stats()["device_allocs"]
    rm.evaluate_device(dx[:100], dl[:100], version=-1)
    once = rm.stats()["device_allocs"]
    assert once == base + 1
    rm.evaluate_device(dx[:100], dl[:100], version=-1)
    rm.evaluate_device(dx[:40], dl[:40], version=-1)
    assert rm.stats()["device_allocs"] == once
    rm.evaluate(x[:100], lab[:100], version=-1)   # the host form stages its images: a larger need
    grown = rm.stats()["device_allocs"]
    assert grown == once + 1
    rm.evaluate(x[:100], lab[:100], version=-1)
    rm.evaluate_device(dx[:100], dl[:100], version=-1)
    assert rm.stats()["device_allocs"] == grown
    rm.close()
