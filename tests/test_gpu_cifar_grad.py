"""The client's gradients on the CIFAR network on the GPU (fleet_amd.cifar_client) against the host
mirror of the kernels (tests/native/check_cifar_backward.cpp --mirror, which test_cifar_grad_cpu.py
holds to a float64 restatement): every comparison is on bits."""
import numpy as np
import pytest

import fleet_amd as F
from fleet_amd import cifar_client as K

import cifar_grad_ref as G
import cifar_ref as R
import model_nets as N
from test_gpu_cifar import LAYERS

pytestmark = pytest.mark.gpu
f = np.float32
NINE = [(dx, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]
# (classes, C, B): B = 1 keeps the bare products' -0, 2 is the first ordered add, T and T + 1 the
# staging edge of k_rgb_fc_sum (T = sample_tile())
CASES = [(10, 1, 1), (10, 1, 2), (10, 3, 3), (10, 2, "T"), (10, 2, "T+1"), (100, 1, 2), (100, 2, "T+1")]
N_IMAGES = 40


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(classes, C, B):
    """a case's (models [3, w + b], idx [C, B] or None, shifts, model row per client, temperature):
    the nine shifts in turn, no idx at (1, 2), temperature 1 at (3, 3) and at 100 classes' (1, 2)"""
    rng = np.random.default_rng(1000 * classes + 10 * C + B)
    models = np.stack([np.concatenate(G.model(31 + r + classes, classes)) for r in range(3)])
    idx = None if (C, B) == (1, 2) else rng.integers(0, N_IMAGES, (C, B)).astype(np.int32)
    if idx is not None:
        idx[0, 0] = 1  # the image whose label is outside [0, classes)
    sh = np.array([NINE[(k + B) % 9] for k in range(C * B)], np.int32).reshape(C, B, 2)
    T = 1.0 if (C, B) == (3, 3) or (classes, C, B) == (100, 1, 2) else 2.0
    return models, idx, sh, (np.arange(C) % 3).astype(np.int32), T


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the images and labels, and per case its inputs and the mirror's rows (one mirror run)"""
    d = tmp_path_factory.mktemp("cifar_grad_mirror")
    exe = G.build_checker(d)
    assert exe is not None, "no clang++ for the host mirror"
    x = G.images(11, N_IMAGES)
    lab = {n: np.random.default_rng(n).integers(0, n, N_IMAGES).astype(np.int32) for n in (10, 100)}
    for n in lab:
        lab[n][1] = n + 2
    T = K.sample_tile()
    cases, jobs = {}, []
    for classes, C, B in CASES:
        Bn = {"T": T, "T+1": T + 1}.get(B, B)
        models, idx, sh, of, temp = _inputs(classes, C, Bn)
        ix = np.arange(C * Bn, dtype=np.int32).reshape(C, Bn) if idx is None else idx
        nw = len(models[0]) - (656 + classes)
        for c in range(C):
            jobs.append((classes, models[of[c], :nw], models[of[c], nw:], x[ix[c]], lab[classes][ix[c]], sh[c], temp))
        cases[(classes, C, B)] = [Bn, models, idx, sh, of, temp, len(jobs) - C]
    rows = G.mirror(exe, d, jobs)
    assert all(blown == 0 for _, blown in rows)
    for v in cases.values():
        v[-1] = np.stack([r for r, _ in rows[v[-1]:v[-1] + len(v[4])]])
    return x, lab, cases, (exe, d)


def _same(got, want, what):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, bad.size, bad[:8], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def _device(codec, classes, x, lab, case, **kw):
    B, models, idx, sh, of, temp, _ = case
    return K.client_gradients_device(codec, classes, _t(models), _t(x), _t(lab[classes]), idx=None if idx is None else _t(idx),
                                     shifts=_t(sh), model_of_client=_t(of), C=len(of), B=B, temperature=temp, **kw)


@pytest.mark.parametrize("classes,C,B", CASES)
def test_device_against_the_host_mirror(codec, world, classes, C, B):
    x, lab, cases, _ = world
    case = cases[(classes, C, B)]
    g = _device(codec, classes, x, lab, case)
    codec.check()
    _same(g.cpu().numpy(), case[-1], (classes, C, B))
    if C == 1:  # the host form: one model for every client
        nw = case[1].shape[1] - (656 + classes)
        host = K.client_gradients(codec, classes, case[1][0, :nw], case[1][0, nw:], x, lab[classes], idx=case[2],
                                  shifts=case[3], temperature=case[5])
        _same(host, case[-1], ("host form", classes, C, B))


@pytest.mark.parametrize("chunk", [1, 2])
def test_chunk_walk_and_its_tail(codec, world, chunk):
    x, lab, cases, _ = world
    with K.chunk_override(chunk):
        g = _device(codec, 10, x, lab, cases[(10, 3, 3)])
        codec.check()
    _same(g.cpu().numpy(), cases[(10, 3, 3)][-1], f"chunk {chunk}")


def test_pitched_buffers_on_a_callers_stream_and_upload_rows(codec, world):
    """image, model, row and upload rows wider than their values, the padding NaN or untouched; the
    upload rows are the encode of the float rows' bits (the codec is decimal: the text pins them)"""
    import torch
    x, lab, cases, _ = world
    case = cases[(10, 3, 3)]
    n = K.grad_len(10)
    xp = np.full((N_IMAGES, 3080), np.nan, f)
    xp[:, :3072] = x
    mp = np.full((3, case[1].shape[1] + 5), np.nan, f)
    mp[:, :-5] = case[1]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        grads = torch.full((3, n + 3), -7.0, dtype=torch.float32, device="cuda")
        ups = torch.zeros((3, 16 * ((n + 2) // 3) + 32), dtype=torch.uint8, device="cuda")
        K.client_gradients_device(codec, 10, _t(mp)[:, :-5], _t(xp), _t(lab[10]), idx=_t(case[2]), shifts=_t(case[3]),
                                  model_of_client=_t(case[4]), temperature=case[5], grads=grads, uploads=ups,
                                  stream=s.cuda_stream)
    s.synchronize()
    codec.check(s.cuda_stream)
    g = grads.cpu().numpy()
    _same(np.ascontiguousarray(g[:, :n]), case[-1], "pitched")
    assert (g[:, n:] == -7.0).all()
    from fleet_amd.client import upload_texts
    for c, text in enumerate(upload_texts(ups, n)):
        assert text == codec.encode_floats(case[-1][c]), c


def test_resident_model_versions(codec, world):
    """train, step, train: the rows on (newest, cnn, the loaded version) after one descent_device
    with a row this call produced equal the mirror on those versions' exported weights"""
    x, lab, cases, checker = world
    _, _, idx, sh, _, temp, _ = cases[(10, 3, 3)]
    w, b = R.model(10, 5)
    rm = F.ResidentModel(codec, N.mode0_text(LAYERS(10), R.B_SIZES[10], R.W_SIZES[10], w, b), 0, max_versions=3)
    rm.initUpdater([0.05, 0.02])
    args = (_t(x), _t(lab[10]))
    g0 = K.resident_client_gradients_device(rm, 10, None, *args, idx=_t(idx), shifts=_t(sh), temperature=temp)
    rm.descent_device(g0[0].contiguous(), 2)
    versions = [None, -1, 0]
    g = K.resident_client_gradients_device(rm, 10, versions, *args, idx=_t(idx), shifts=_t(sh), temperature=temp)
    codec.check()
    jobs = [rm.export(rm.modelsSize() - 1 if v is None else v) for v in versions]
    jobs = [(10, wv, bv, x[idx[c]], lab[10][idx[c]], sh[c], temp) for c, (wv, bv) in enumerate(jobs)]
    want = np.stack([r for r, _ in G.mirror(*checker, jobs)])
    _same(g.cpu().numpy(), want, "versions")
    _same(g.cpu().numpy()[2], g0.cpu().numpy()[2], "the loaded version is the one the first call ran on")
    assert (g.cpu().numpy()[0] != g0.cpu().numpy()[0]).any()  # the step moved the model
    rm.close()


def test_a_nan_forward_is_reported_and_the_other_clients_stand(codec, world):
    x, lab, cases, _ = world
    case = list(cases[(10, 3, 3)])
    case[1] = case[1].copy()
    case[1][1, 306480 - 1] = np.nan  # client 1's model: a weight of FC2
    g = _device(codec, 10, x, lab, case)
    with pytest.raises(F.FleetError) as e:
        codec.check()
    assert e.value.code == F.FLEET_ERR_ARG
    codec.check()  # the word is cleared
    _same(g.cpu().numpy()[[0, 2]], case[-1][[0, 2]], "the sound clients")


# -- fleet_rgbnet_grads' refusals, their codes and texts (the body is shared with fleet_client_ex_grads)

def _counts_text(classes, dw=0, db=0):
    from host_form_refusals import counts
    n_w, n_b = counts("rgbnet_grads", classes)
    return f"client gradients: {n_w + dw} weights and {n_b + db} biases, expected {n_w} and {n_b}"


def _pitch_text(classes):
    from host_form_refusals import grad_len
    up_len = F.b64_len(grad_len("rgbnet_grads", classes))
    return f"upload pitch {up_len - 1} < {up_len}"


@pytest.mark.parametrize("kw,code,text", [
    (dict(classes=7), F.FLEET_ERR_ARG, "client gradients: 7 classes, the network has 10 or 100"),
    (dict(classes=0, extra_w=1), F.FLEET_ERR_ARG, "client gradients: 0 classes, the network has 10 or 100"),  # before the counts
    (dict(extra_w=1), F.FLEET_ERR_ARG, lambda: _counts_text(10, dw=1)),
    (dict(classes=100, sized_for=100, extra_b=-1), F.FLEET_ERR_ARG, lambda: _counts_text(100, db=-1)),
    (dict(B=2), F.FLEET_ERR_ARG, "client gradients: 2 images asked of 1"),
    (dict(idx=[-1]), F.FLEET_ERR_ARG, "sample 0: index -1 outside the 1 images"),
    (dict(idx=[0, 1], B=2), F.FLEET_ERR_ARG, "sample 1: index 1 outside the 1 images"),
    (dict(shifts=[0, 2]), F.FLEET_ERR_ARG, "sample 0: shift 2 outside {-1, 0, 1}"),
    (dict(idx=[0, 0], shifts=[1, -1, -2, 0], B=2), F.FLEET_ERR_ARG, "sample 1: shift -2 outside {-1, 0, 1}"),
    (dict(upload_pitch=-1), F.FLEET_ERR_CAPACITY, lambda: _pitch_text(10)),  # one below fleet_b64_len
    # two checks could fire: counts, picks, indices, shifts, pitch, in this order
    (dict(extra_w=1, idx=[1]), F.FLEET_ERR_ARG, lambda: _counts_text(10, dw=1)),
    (dict(idx=[1], shifts=[0, 2]), F.FLEET_ERR_ARG, "sample 0: index 1 outside the 1 images"),
    (dict(shifts=[-2, 0], upload_pitch=16), F.FLEET_ERR_ARG, "sample 0: shift -2 outside {-1, 0, 1}"),
])
def test_host_form_refusals(codec, kw, code, text):
    from host_form_refusals import grad_len, refusal
    if kw.get("upload_pitch") == -1:
        kw = dict(kw, upload_pitch=F.b64_len(grad_len("rgbnet_grads", 10)) - 1)
    assert refusal(codec, "rgbnet_grads", **kw) == (code, text() if callable(text) else text)
