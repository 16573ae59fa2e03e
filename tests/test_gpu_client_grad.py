"""The client's gradients on the device: k_client_sample / k_client_sum through
every entry point, bit for bit against tests/golden/client_grad_ref.npz (recorded from the
reference's own network class) and, beyond the fixture's shapes, against the host mirror of the
same source (tests/native/check_client_grad.cpp --mirror over client_backward.h)."""
import os
import subprocess

import numpy as np
import pytest

import client_grad_ref as R
import eval_ref as E
import fleet_amd as F
from fleet_amd import client as K
from fleet_amd.layouts import MNIST
from test_native_math import _clang

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = np.float32


@pytest.fixture(scope="module")
def z():
    return R.load()


@pytest.fixture(scope="module")
def fresh():
    """inputs the fixture does not hold: two models, 40 images, labels, and for every job of
    JOBS its (idx, shifts)"""
    w, b = R.model()
    w2, b2 = E.model_a(seed=9)
    x = E.images_a(40, seed=777)
    lab = np.random.RandomState(5).randint(0, 10, 40).astype(np.int32)
    return (w, b), (w2, b2), x, lab


# (C, B): the ordered sum at B = 1, 2, 7 and 33
JOBS = [(2, 1), (4, 1), (2, 2), (4, 2), (2, 7), (4, 7), (2, 33)]


def _job_inputs(C, B, n_images, seed):
    r = np.random.RandomState(seed)
    idx = r.randint(0, n_images, (C, B)).astype(np.int32)  # with repeats
    shifts = r.randint(-1, 2, (C, B, 2)).astype(np.int32)
    return idx, shifts


@pytest.fixture(scope="module")
def mirror(tmp_path_factory, fresh):
    """the host mirror's vectors for every job of JOBS (model 1) plus one job on model 2 and
    one without indices, computed once: {name: [C, 22961]}"""
    clang = _clang()
    if clang is None:
        pytest.skip("no clang++ for the host build of client_backward.h")
    (w, b), (w2, b2), x, lab = fresh
    d = tmp_path_factory.mktemp("client_grad_mirror")
    exe = str(d / "check_client_grad")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-mfma", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "native", "check_client_grad.cpp"), "-o", exe])
    jobs = []
    for n, (C, B) in enumerate(JOBS):
        idx, sh = _job_inputs(C, B, len(x), 100 + n)
        jobs.append((f"{C}x{B}", w, b, C, B, 2.0, idx, sh))
    idx, sh = _job_inputs(3, 5, len(x), 300)
    jobs.append(("model2", w2, b2, 3, 5, 2.0, idx, sh))
    jobs.append(("noidx", w, b, 4, 7, 1.0, np.arange(28, dtype=np.int32).reshape(4, 7), np.zeros((4, 7, 2), np.int32)))
    with open(d / "jobs.bin", "wb") as fh:
        fh.write(np.int32(len(jobs)).tobytes())
        for name, mw, mb, C, B, T, idx, sh in jobs:
            fh.write(mw.tobytes() + mb.tobytes() + np.array([C, B], np.int32).tobytes() + f(T).tobytes())
            fh.write(np.ascontiguousarray(x[idx.reshape(-1)]).tobytes() + lab[idx.reshape(-1)].tobytes() + sh.tobytes())
    subprocess.check_call([exe, "--mirror", str(d / "jobs.bin"), str(d / "vec.out")], timeout=600)
    vec = np.fromfile(d / "vec.out", f)
    out, o = {}, 0
    for name, mw, mb, C, B, T, idx, sh in jobs:
        out[name] = (vec[o:o + C * R.N_UP].reshape(C, R.N_UP), idx, sh)
        o += C * R.N_UP
    assert o == len(vec)
    return out


def _same(got, want, what):
    bad = R.bits(got) != R.bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def test_every_fixture_case(codec, z):
    """every recorded case through fleet_client_grads, C = 1, B <= 5: equal in bits"""
    w, b = R.model()
    for name, B, teacher, mode, seed, x, lab, sh in R.cases():
        shifts = R.recorded_shifts(z, name, x) if mode else sh
        g = K.client_gradients(codec, w, b, x, lab, shifts=shifts, temperature=R.temperature_of(teacher))
        assert g.shape == (1, R.N_UP)
        if name.startswith("s_"):
            assert R.sha(g[0]) == bytes(z[f"{name}_grad_sha256"]).decode(), name
            _same(g[0][R.G_C1], z[f"{name}_grad_c1"], name)
            _same(g[0][R.G_I1], z[f"{name}_grad_i1"], name)
        else:
            _same(g[0], z[f"{name}_grad"], name)
        assert np.array_equal(g[0][MNIST.header_positions()], np.array(MNIST.header_values(), f))
    # b5 summed in reverse order is another vector: the order is the reference's
    name, B, teacher, mode, seed, x, lab, sh = R.cases()[-1]
    shifts = R.recorded_shifts(z, name, x)
    g = K.client_gradients(codec, w, b, x[::-1], lab[::-1], shifts=shifts[::-1])
    _same(g[0], z["b5_reverse"], "b5 reversed")


def test_fleet_of_three_on_two_models_and_the_chunk_walk(codec, fresh, mirror):
    """C = 3 clients of B = 5 on two model rows equals the three single-client calls, also with
    the chunk forced to 1 and to 2 (the chunk walk and its tail)"""
    import torch
    (w, b), (w2, b2), x, lab = fresh
    want2, idx, sh = mirror["model2"]
    models = torch.from_numpy(np.stack([np.concatenate([w, b]), np.concatenate([w2, b2])])).cuda()
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    di, ds = torch.from_numpy(idx).cuda(), torch.from_numpy(sh).cuda()
    of = np.array([1, 0, 1], np.int32)
    single = np.stack([K.client_gradients(codec, (w, w2)[of[c]], (b, b2)[of[c]], x, lab, idx=idx[c], shifts=sh[c])[0]
                       for c in range(3)])
    _same(single[0], want2[0], "model 2, client 0 against the mirror")
    _same(single[2], want2[2], "model 2, client 2 against the mirror")
    assert (R.bits(single[1]) != R.bits(want2[1])).any()  # client 1 is on the other model
    for chunk in (0, 1, 2):
        with K.client_chunk_override(chunk):
            g = K.client_gradients_device(codec, models, dx, dl, idx=di, shifts=ds, model_of_client=torch.from_numpy(of).cuda())
            codec.check()
        _same(g.cpu().numpy(), single, f"chunk {chunk}")


@pytest.mark.parametrize("C,B", JOBS)
def test_device_against_the_host_mirror(codec, fresh, mirror, C, B):
    (w, b), _, x, lab = fresh
    want, idx, sh = mirror[f"{C}x{B}"]
    _same(K.client_gradients(codec, w, b, x, lab, idx=idx, shifts=sh), want, f"C {C} B {B}")


def test_null_indices_and_null_shifts(codec, fresh, mirror):
    """d_idx NULL takes images c*B + k, d_shift NULL shifts nothing; temperature 1"""
    import torch
    (w, b), _, x, lab = fresh
    want, idx, sh = mirror["noidx"]
    models = torch.from_numpy(np.concatenate([w, b])).cuda()
    g = K.client_gradients_device(codec, models, torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda(), C=4, B=7,
                                      temperature=1.0)
    codec.check()
    _same(g.cpu().numpy(), want, "no indices")
    with pytest.raises(F.FleetError) as e:  # 41 images asked of 40
        K.client_gradients_device(codec, models, torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda(), C=1, B=41)
    assert e.value.code == F.FLEET_ERR_ARG


def test_upload_rows_and_the_existing_consumer(codec, fresh, mirror):
    """upload rows equal Codec.encode_floats of the fp32 rows byte for byte, and update_device
    over 4 such rows equals Codec.update on the host texts"""
    import torch
    (w, b), _, x, lab = fresh
    want, idx, sh = mirror["4x7"]
    models = torch.from_numpy(np.concatenate([w, b])).cuda()
    g, up = K.client_gradients_device(codec, models, torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda(),
                                          idx=torch.from_numpy(idx).cuda(), shifts=torch.from_numpy(sh).cuda(),
                                          uploads=True)
    codec.check()
    _same(g.cpu().numpy(), want, "rows")
    texts = K.upload_texts(up)
    for c in range(4):
        assert texts[c] == codec.encode_floats(want[c]), c
    rows, host_texts = K.client_gradients(codec, w, b, x, lab, idx=idx, shifts=sh, uploads=True)
    assert host_texts == texts
    L = len(texts[0])
    groups = (F.b64_count(L) + 2) // 3
    merged = torch.zeros(16 * groups, dtype=torch.uint8, device="cuda")
    dampen = [1.0, 0.5, 0.25, 1.0]
    codec.update_device(up, L, dampen, MNIST.header_positions(), merged)
    codec.check()
    torch.cuda.synchronize()
    assert merged.cpu().numpy()[:L].tobytes() == codec.update(texts, dampen)


def test_resident_model_versions(codec, fresh):
    """resident_client_gradients_device on (newest, cnn, an older version) equals
    client_gradients on those versions' weights; the step between them is taken with a
    gradient this call produced"""
    import torch
    _, _, x, lab = fresh
    rm = F.ResidentModel(codec, E.seeded_text(), distillation_mode=1, max_versions=3)
    rm.initUpdater([0.5])
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    idx, sh = _job_inputs(3, 4, len(x), 900)
    di, ds = torch.from_numpy(idx).cuda(), torch.from_numpy(sh).cuda()
    g0, up = K.resident_client_gradients_device(rm, None, dx, dl, idx=di, shifts=ds, uploads=True)
    codec.check()
    texts = K.upload_texts(up)
    rm.descentNative(codec.update(texts, [1.0, 1.0, 1.0]), 4, 2)
    assert rm.modelsSize() == 2
    versions = [None, -1, 0]
    g = K.resident_client_gradients_device(rm, versions, dx, dl, idx=di, shifts=ds)
    codec.check()
    g = g.cpu().numpy()
    for c, v in enumerate(versions):
        w, b = rm.export(rm.modelsSize() - 1 if v is None else v)
        _same(g[c], K.client_gradients(codec, w, b, x, lab, idx=idx[c], shifts=sh[c])[0], f"version {v}")
    _same(g[2], g0.cpu().numpy()[2], "the older version is the one the first call ran on")
    assert (R.bits(g[0]) != R.bits(g0.cpu().numpy()[0])).any()  # the step moved the model
    with pytest.raises(F.FleetError) as e:
        K.resident_client_gradients_device(rm, [0, 5, 0], dx, dl, idx=di, shifts=ds)
    assert e.value.code == F.FLEET_ERR_ARG
    rm.close()


def test_host_form_refuses_before_any_launch(codec, fresh):
    (w, b), _, x, lab = fresh
    L, h = codec._L, codec._h
    g = np.zeros((1, R.N_UP), f)
    idx = np.array([0, 1], np.int32)
    sh = np.zeros((2, 2), np.int32)

    def call(w=w, n_w=len(w), b=b, n_b=len(b), x=x, F_=784, lab=lab, idx=idx, sh=sh, C=1, B=2, g=g):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.fleet_client_grads(h, p(w), n_w, p(b), n_b, p(x), len(lab) if lab is not None else 0, F_, p(lab), p(idx),
                                    p(sh), C, B, 2.0, p(g), None, 0)
    assert call() == F.FLEET_OK
    codec.check()
    for kw in (dict(w=None), dict(b=None), dict(x=None), dict(lab=None), dict(g=None), dict(F_=783), dict(C=0),
               dict(B=0), dict(C=-1), dict(n_w=len(w) - 1), dict(n_b=len(b) + 1),
               dict(idx=np.array([0, 40], np.int32)), dict(idx=np.array([-1, 0], np.int32)),
               dict(sh=np.array([[0, 2], [0, 0]], np.int32)), dict(sh=np.array([[0, 0], [-2, 0]], np.int32)),
               dict(idx=None, B=41)):
        assert call(**kw) == F.FLEET_ERR_ARG, kw
    codec.check()  # nothing was launched: no device error is pending


def test_bad_indices_and_a_nan_forward_set_the_error_bit(codec, fresh):
    """a bad image index and a bad model index are FLEET_ERR_ARG at check(); a forward that
    comes out NaN (an inf weight in FC2) sets the error bit too, and nothing faults"""
    import torch
    (w, b), _, x, lab = fresh
    models = torch.from_numpy(np.concatenate([w, b])).reshape(1, -1).cuda()
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    good = torch.tensor([[0, 1]], dtype=torch.int32, device="cuda")
    for idx, of in ((torch.tensor([[0, 40]], dtype=torch.int32, device="cuda"), None),
                    (good, torch.tensor([1], dtype=torch.int32, device="cuda")),
                    (good, torch.tensor([-1], dtype=torch.int32, device="cuda"))):
        K.client_gradients_device(codec, models, dx, dl, idx=idx, model_of_client=of)
        with pytest.raises(F.FleetError) as e:
            codec.check()
        assert e.value.code == F.FLEET_ERR_ARG
    bad_shift = torch.tensor([[[0, 0], [2, 0]]], dtype=torch.int32, device="cuda")
    K.client_gradients_device(codec, models, dx, dl, idx=good, shifts=bad_shift)
    with pytest.raises(F.FleetError):
        codec.check()
    wi = w.copy()
    wi[E.W_SPLITS[3]] = np.inf
    wi[E.W_SPLITS[3] + 1] = np.inf
    with pytest.raises(F.FleetError) as e:
        K.client_gradients(codec, wi, b, x[:2], lab[:2])
    assert e.value.code == F.FLEET_ERR_ARG and "blew up" in str(e.value)
    codec.check()  # the bit was read and cleared
    g = K.client_gradients(codec, w, b, x[:2], lab[:2])  # and the context still works
    assert np.isfinite(g).all()
