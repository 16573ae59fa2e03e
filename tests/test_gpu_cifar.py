"""The Driver's test() on the reference's CIFAR network on the GPU (Driver/src/main/c++/
cppNN_backend.cpp:53-75, 128-138): the fixture's cases against tests/golden/cifar_ref.npz,
recorded from the reference's own network class, and every other shape against the host mirror
of the kernel (tests/native/check_cifar_forward.cpp --mirror, which test_cifar_inputs.py holds
to the same recording). Every comparison is on bits."""
import numpy as np
import pytest

import fleet_amd as F
from fleet_amd import cifar

import cifar_ref as R
import model_nets as N

pytestmark = pytest.mark.gpu
f = np.float32

LAYERS = lambda n: (("I1", "input 32 32 3 identity"), ("C1", "convolution 3 16 1 elu"), ("P1", "max_pool 3 2"),  # noqa: E731
                    ("C2", "convolution 3 64 1 elu"), ("P2", "max_pool 4 4"), ("local4", "fully_connected 384 relu"),
                    ("local5", "fully_connected 192 relu"), ("FC2", f"fully_connected {n} softmax"))


@pytest.fixture(scope="module")
def z():
    return R.load()


@pytest.fixture(scope="module")
def main():
    return {n: R.main_case(n) for n in (10, 100)}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("cifar_mirror")
    exe = R.build_checker(d)
    assert exe is not None, "no clang++ for the host mirror"
    return exe, d


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(ev, c, B, contract=1, what=""):
    """an Evaluation against the first B images of a recorded case"""
    for got, want, name in ((ev.predictions, c["pred"][:B], "pred"), (ev.probabilities, c["p"][:B], "p"),
                            (ev.error, c["error"][B - 1], "error"), (ev.accuracy, c["accuracy"][B - 1], "accuracy")):
        bad = R.mismatch(contract, np.atleast_1d(got), np.atleast_1d(want))
        assert not bad, (what, B, name, bad)
    assert ev.correct == c["correct"][B - 1], (what, B)


def _same_mirror(ev, m, what=""):
    """an Evaluation against a mirror job's result"""
    for got, want, name in ((ev.predictions, m["pred"], "pred"), (ev.probabilities, m["p"], "p"),
                            (ev.error, m["error"], "error"), (ev.accuracy, m["accuracy"], "accuracy")):
        bad = R.mismatch(1, np.atleast_1d(got), np.atleast_1d(want))
        assert not bad, (what, name, bad)
    assert ev.correct == m["correct"], what


def _device(codec, classes, w, b, x, lab, idx=None, stream=None):
    import torch
    B = len(lab) if idx is None else len(idx)
    out = {"costs": torch.empty(B, dtype=torch.float32, device="cuda"),
           "probsN": torch.empty(B, classes, dtype=torch.float32, device="cuda")}
    return cifar.evaluate_device(codec, _t(w), _t(b), _t(x), _t(lab), None if idx is None else _t(idx), classes=classes,
                                 out=out, stream=stream)


# -- the recorded cases ----------------------------------------------------------------------------

@pytest.mark.parametrize("classes", [10, 100])
def test_main_case_whole(codec, z, main, classes):
    """a10 / a100 through the vector form and the device form, costs and probsN taken"""
    w, b, x, lab = main[classes]
    a = R.case(z, f"a{classes}")
    B = len(lab)
    taken = {}
    _same(cifar.evaluate(codec, w, b, x, lab, classes=classes, out=taken), a, B, what="vector form")
    assert not R.mismatch(1, taken["costs"], a["cost"])
    assert not R.mismatch(1, taken["probsN"][:R.N_PROBS], a["probs"])
    out = _device(codec, classes, w, b, x, lab)
    codec.check()
    _same(F.evaluation_from_device(out), a, B, what="device form")
    assert not R.mismatch(1, out["costs"].cpu().numpy(), a["cost"])
    assert not R.mismatch(1, out["probsN"].cpu().numpy()[:R.N_PROBS], a["probs"])
    assert np.array_equal(R.bits(out["probsN"].cpu().numpy()), R.bits(taken["probsN"]))


def test_group_edges(codec, z, main):
    """B at 1, G - 1, G, G + 1 and 2G + 1: prefixes of a10"""
    w, b, x, lab = main[10]
    a = R.case(z, "a10")
    G = cifar.block_images()
    for B in sorted({1, max(G - 1, 1), G, G + 1, 2 * G + 1}):
        _same(cifar.evaluate(codec, w, b, x[:B], lab[:B]), a, B, what="group edge")


@pytest.mark.parametrize("grid", [1, 2])
def test_grid_stride_passes(codec, z, main, grid):
    """B = 3G + 1 under a capped grid: several grid-stride passes, a ragged last group"""
    w, b, x, lab = main[10]
    B = 3 * cifar.block_images() + 1
    with cifar.grid_override(grid):
        _same(cifar.evaluate(codec, w, b, x[:B], lab[:B]), R.case(z, "a10"), B, what=f"grid {grid}")


def test_permutation_and_repeats(codec, z, main):
    w, b, x, lab = main[10]
    a = R.case(z, "a10")
    ev = cifar.evaluate(codec, w, b, x, lab, idx=R.PERM)
    assert R.bits(ev.error) == R.bits(z["a10_perm_error"])[0] != R.bits(a["error"][-1])
    assert R.bits(ev.accuracy) == R.bits(z["a10_perm_accuracy"])[0] and ev.correct == int(z["a10_perm_correct"].reshape(-1)[0])
    assert np.array_equal(ev.predictions, a["pred"][R.PERM]) and not R.mismatch(1, ev.probabilities, a["p"][R.PERM])
    for idx in ([7, 7, 7, 3, 7], [159], [5, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5, 159]):
        idx = np.array(idx, np.int32)
        for ev in (cifar.evaluate(codec, w, b, x, lab, idx=idx), F.evaluation_from_device(_device(codec, 10, w, b, x, lab, idx))):
            assert np.array_equal(ev.predictions, a["pred"][idx]) and not R.mismatch(1, ev.probabilities, a["p"][idx])
            assert R.bits(ev.error) == R.bits(R.ordered_error(a["cost"][idx]))
            correct = int((a["pred"][idx] == lab[idx]).sum())
            assert ev.correct == correct and R.bits(ev.accuracy) == R.bits(R.accuracy_of(correct, len(idx)))
    codec.check()


def test_index_out_of_range(codec, main):
    import torch
    w, b, x, lab = main[10]
    for bad in ([0, 160], [-1], [3, 2 ** 31 - 1]):
        with pytest.raises(F.FleetError) as e:
            cifar.evaluate(codec, w, b, x, lab, idx=np.array(bad, np.int32))
        assert e.value.code == F.FLEET_ERR_ARG
    cifar.evaluate_device(codec, _t(w), _t(b), _t(x[:16]), _t(lab[:16]),
                          torch.tensor([1, 16, 2], dtype=torch.int32, device="cuda"))
    with pytest.raises(F.FleetError) as e:
        codec.check()
    assert e.value.code == F.FLEET_ERR_ARG
    codec.check()  # the word is cleared


def test_pitched_rows_on_a_callers_stream(codec, z, main):
    """rows 3080 floats apart, the padding never read; the caller's stream; outputs not taken"""
    import torch
    w, b, x, lab = main[10]
    a = R.case(z, "a10")
    B, Fp = 19, 3080
    xp = np.full((B, Fp), np.nan, f)
    xp[:, :3072] = x[:B]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dw, db, dx, dl = _t(w), _t(b), _t(xp), _t(lab[:B].copy())
        full = cifar.evaluate_device(codec, dw, db, dx, dl, stream=s.cuda_stream)
        bare = cifar.evaluate_device(codec, dw, db, dx, dl, out={"predictions": None, "probabilities": None},
                                     stream=s.cuda_stream)
    s.synchronize()
    codec.check(s.cuda_stream)
    _same(F.evaluation_from_device(full), a, B, what="stream, F = 3080")
    ev = F.evaluation_from_device(bare)
    assert ev.predictions is None and ev.probabilities is None
    assert R.bits(ev.error) == R.bits(a["error"][B - 1]) and ev.correct == a["correct"][B - 1]
    _same(cifar.evaluate(codec, w, b, xp, lab[:B]), a, B, what="vector form, F = 3080")


@pytest.mark.parametrize("case", [c[0] for c in R.edge_cases()])
def test_edges(codec, z, case):
    name, contract, w, b, x, lab = next(c for c in R.edge_cases() if c[0] == case)
    c = R.case(z, name)
    B = len(lab)
    taken = {}
    _same(cifar.evaluate(codec, w, b, x, lab, out=taken), c, B, contract, what=name)
    assert not R.mismatch(contract, taken["costs"], c["cost"])
    assert not R.mismatch(contract, taken["probsN"], c["probs"])
    out = _device(codec, 10, w, b, x, lab)
    codec.check()
    _same(F.evaluation_from_device(out), c, B, contract, what=name + " device")
    assert not R.mismatch(contract, out["costs"].cpu().numpy(), c["cost"])
    assert not R.mismatch(contract, out["probsN"].cpu().numpy(), c["probs"])


# -- the models ------------------------------------------------------------------------------------

def _seeded_text(classes=10, seed=5):
    w, b = R.model(classes, seed)
    return N.mode0_text(LAYERS(classes), R.B_SIZES[classes], R.W_SIZES[classes], w, b)


def _merged_gradient(seed):
    """a merged CIFAR-10 gradient as decodeFloat delivers it (fleet_amd.layouts.CIFAR10: the
    gradients() vector of this network), seeded"""
    from fleet_amd.layouts import CIFAR10
    values = np.random.RandomState(seed).normal(0, 0.02, CIFAR10.n_flat).astype(f)
    return N.layout_gradient(CIFAR10, values)


def test_models_equal_the_vector_form(codec, main, checker):
    """a mode-0 CIFAR-10 text: Model and ResidentModel, host and device forms, every version, before
    and after one descent_device, against the vector form and the mirror on the exported weights"""
    import torch
    _, _, x, lab = main[10]
    B = 21
    x, lab = x[:B], lab[:B]
    text = _seeded_text()
    hm = F.Model(codec, text, distillation_mode=0)
    rm = F.ResidentModel(codec, text, 0, max_versions=3)
    for m in (hm, rm):
        m.initUpdater([0.05, 0.02])
    dx, dl = _t(x), _t(lab)
    w0, b0 = rm.export(-1)
    assert len(w0) == cifar.weight_count(10) and len(b0) == cifar.bias_count(10)
    want = cifar.evaluate(codec, w0, b0, x, lab)
    _same_mirror(want, R.mirror(*checker, [(10, w0, b0, x, lab, None)])[0], "vector form on the model's weights")
    for version in (None, -1, 0):
        for ev in (cifar.model_evaluate(hm, x, lab, version=version), cifar.resident_evaluate(rm, x, lab, version=version),
                   F.evaluation_from_device(cifar.resident_evaluate_device(rm, dx, dl, version=version))):
            assert R.bits(ev.error) == R.bits(want.error) and ev.correct == want.correct
            assert np.array_equal(ev.predictions, want.predictions) and not R.mismatch(1, ev.probabilities, want.probabilities)
    grad = _merged_gradient(77)
    rm.descent_device(torch.from_numpy(grad).cuda(), 2)
    assert rm.modelsSize() >= 2
    errors = {}
    for version in (None, -1) + tuple(range(rm.modelsSize())):
        w, b = rm.export(rm.modelsSize() - 1 if version is None else version)
        want = cifar.evaluate(codec, w, b, x, lab)
        errors[version] = int(R.bits(want.error).reshape(-1)[0])
        for ev in (cifar.resident_evaluate(rm, x, lab, version=version),
                   F.evaluation_from_device(cifar.resident_evaluate_device(rm, dx, dl, version=version))):
            assert R.bits(ev.error) == R.bits(want.error) and R.bits(ev.accuracy) == R.bits(want.accuracy)
            assert ev.correct == want.correct and np.array_equal(ev.predictions, want.predictions)
            assert not R.mismatch(1, ev.probabilities, want.probabilities)
    # version 0 is the loaded model; the newest is the stepped one (a copy of cnn through its text)
    assert errors[0] != errors[None] and errors[0] != errors[-1]
    codec.check()
    # the existing evaluation still refuses this network
    for m in (hm, rm):
        with pytest.raises(F.FleetError) as e:
            m.evaluate(np.zeros((2, 784), f), np.zeros(2, np.int32), version=-1)
        assert e.value.code == F.FLEET_ERR_ARG
        with pytest.raises(F.FleetError) as e:
            cifar.model_evaluate(hm, x, lab, version=5) if m is hm else cifar.resident_evaluate(rm, x, lab, version=5)
        assert e.value.code == F.FLEET_ERR_ARG
        m.close()


def test_a_cifar100_model_reads_its_head(codec, main, checker):
    _, _, x, lab = main[100]
    x, lab = x[:9], lab[:9]
    rm = F.ResidentModel(codec, _seeded_text(100, seed=6), 0, max_versions=2)
    w, b = rm.export(-1)
    ev = cifar.resident_evaluate(rm, x, lab, version=-1)
    _same_mirror(ev, R.mirror(*checker, [(100, w, b, x, lab, None)])[0], "CIFAR-100 resident model")
    assert ev.predictions.max() >= 10
    rm.close()


def test_shapes_the_fixture_does_not_hold(codec, main, checker):
    """another model and other images at B = 2G + 3 with an index list, both heads: the mirror"""
    G = cifar.block_images()
    jobs = []
    for classes in (10, 100):
        w, b = R.model(classes, 400 + classes)
        x = R.images(2 * G + 3, 500 + classes)
        lab = np.random.RandomState(classes).randint(0, classes, len(x)).astype(np.int32)
        idx = np.random.RandomState(classes + 1).randint(0, len(x), G + 2).astype(np.int32)
        jobs += [(classes, w, b, x, lab, None), (classes, w, b, x, lab, idx)]
    for job, m in zip(jobs, R.mirror(*checker, jobs)):
        classes, w, b, x, lab, idx = job
        taken = {}
        _same_mirror(cifar.evaluate(codec, w, b, x, lab, idx=idx, classes=classes, out=taken), m, f"{classes} vector form")
        assert not R.mismatch(1, taken["costs"], m["cost"]) and not R.mismatch(1, taken["probsN"], m["probs"])


# -- refusals --------------------------------------------------------------------------------------

def test_refusals(codec, main):
    w, b, x, lab = main[10]
    w100, b100 = main[100][:2]
    for bad in (lambda: cifar.evaluate(codec, w[:-1], b, x[:4], lab[:4]),             # a wrong n_w
                lambda: cifar.evaluate(codec, w, b[:-1], x[:4], lab[:4]),
                lambda: cifar.evaluate(codec, w, b, x[:4], lab[:4], classes=100),     # the other head's sizes
                lambda: cifar.evaluate(codec, w100, b100, x[:4], lab[:4], classes=10),
                lambda: cifar.evaluate(codec, w, b, x[:4], lab[:4], classes=7),
                lambda: cifar.evaluate(codec, w, b, x[:0], lab[:0]),                  # B = 0
                lambda: cifar.evaluate(codec, w, b, x[:4], lab[:4], idx=np.zeros(0, np.int32)),
                lambda: cifar.evaluate(codec, w, b, x[:4, :3071], lab[:4])):          # F < 3072
        with pytest.raises(F.FleetError) as e:
            bad()
        assert e.value.code == F.FLEET_ERR_ARG
    with pytest.raises(ValueError):
        cifar.evaluate_device(codec, _t(w), _t(b), _t(x[:4]), _t(lab[:4]), classes=7)
    # models that are not the CIFAR network
    import eval_ref
    text = _seeded_text()
    texts = [(eval_ref.seeded_text(), 1, "I1")]
    for old, new, where in ((b"max_pool 3 2", b"max_pool 3 3", "P1"),
                            (b"fully_connected 192 relu", b"fully_connected 192 elu", "local5"),
                            (b"fully_connected 10 softmax", b"fully_connected 10 tanh", "FC2")):
        assert text.count(old) == 1
        texts.append((text.replace(old, new), 0, where))
    for bad_text, mode, where in texts:
        if where == "P1":
            # another stride gives another P1 and another local4: sizes that follow from the layer list
            lay = list(LAYERS(10))
            lay[2] = ("P1", "max_pool 3 3")
            ws = (432, 9216, 64 * 2 * 2 * 384, 73728, 1920)
            r = np.random.RandomState(3)
            bad_text = N.mode0_text(tuple(lay), R.B_SIZES[10], ws, r.normal(0, 0.1, sum(ws)).astype(f),
                                    r.normal(0, 0.1, 666).astype(f))
        hm = F.Model(codec, bad_text, distillation_mode=mode)
        rm = F.ResidentModel(codec, bad_text, mode, max_versions=2)
        for call in (lambda: cifar.model_evaluate(hm, x[:4], lab[:4], version=-1),
                     lambda: cifar.resident_evaluate(rm, x[:4], lab[:4], version=-1),
                     lambda: cifar.resident_evaluate_device(rm, _t(x[:4]), _t(lab[:4]), version=-1)):
            with pytest.raises(F.FleetError) as e:
                call()
            assert e.value.code == F.FLEET_ERR_ARG and where in str(e.value), str(e.value)
        hm.close()
        rm.close()
    codec.check()  # nothing was launched that could have set the word


# -- allocation ------------------------------------------------------------------------------------

def test_workspace_is_allocated_once(codec, main):
    _, _, x, lab = main[10]
    dx, dl = _t(x), _t(lab)
    rm = F.ResidentModel(codec, _seeded_text(), 0, max_versions=2)
    base = rm.stats()["device_allocs"]
    cifar.resident_evaluate_device(rm, dx[:50], dl[:50], version=-1)
    once = rm.stats()["device_allocs"]
    assert once == base + 1
    cifar.resident_evaluate_device(rm, dx[:50], dl[:50], version=-1)
    cifar.resident_evaluate_device(rm, dx[:20], dl[:20], version=-1)
    assert rm.stats()["device_allocs"] == once
    cifar.resident_evaluate(rm, x[:50], lab[:50], version=-1)   # the host form stages its images: a larger need
    grown = rm.stats()["device_allocs"]
    assert grown == once + 1
    cifar.resident_evaluate(rm, x[:50], lab[:50], version=-1)
    cifar.resident_evaluate_device(rm, dx[:50], dl[:50], version=-1)
    assert rm.stats()["device_allocs"] == grown
    rm.close()
