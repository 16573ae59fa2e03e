"""DPgradients on the CIFAR network on the GPU (fleet_amd.cifar_client, clip= / sigma=), in bits
against DESIGN.md §4.9's arithmetic restated in numpy below. The per-sample rows come from the
plain path (test_gpu_cifar_grad.py holds it to the host mirror), every sample run as a client of
its own with B = 1; the squares, the strictly sequential binary32 sum in scale_gradients' walk
order, the scale, the scaled dbias blocks, the ordered sum and the noise are numpy's."""
import functools

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd import cifar_client as K

import cifar_grad_ref as G

pytestmark = pytest.mark.gpu
f = np.float32
WALK = ["dW FC2", "dbias FC2", "dW local5", "dbias local5", "dW local4", "dbias local4", "dbias P2", "dW C2", "dbias P1",
        "dW C1", "dbias I1"]
SIGMAS = [0.0, 1 / 128, 4.0]  # client c takes SIGMAS[c % 3]: every call mixes plain and DP clients
# (classes, C, B): B = 1 is the noise alone; T + 1 crosses k_rgb_fc_sum's staging; 2 x 33 clipped
# samples cross k_rgb_clip's 64 lanes and leave a second wave with two of them
CASES = [(10, 3, 1), (10, 3, 2), (10, 4, 3), (10, 2, "T+1"), (10, 2, 34), (100, 2, 3)]
N_IMAGES = 40


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, bad.size, bad[:8], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def _reference(classes, rows, sigma, z):
    """rows [C, B, n]: every sample's own gradients(). Returns (clip [C], want [C, n]; the rows of
    the clients with sigma = 0 are left to the plain call), after the preconditions on what it computed."""
    C, B, n = rows.shape
    lay = F.layouts.CIFAR10 if classes == 10 else F.layouts.CIFAR100
    at = {name: (lo, hi) for name, lo, hi in G.blocks(classes)}
    sq = rows * rows
    sqsum = np.cumsum(np.concatenate([sq[..., at[k][0]:at[k][1]] for k in WALK], -1), -1, dtype=f)[..., -1]
    layout = np.cumsum(np.concatenate([sq[..., lo:hi] for _, lo, hi in G.blocks(classes)], -1), -1, dtype=f)[..., -1]
    assert (sqsum.view(np.uint32) != layout.view(np.uint32)).any()  # the walk's order shows
    norm = np.sqrt(sqsum)
    assert norm.dtype == f
    clip = np.ones(C, f) if B == 1 else f(0.5) * norm[:, 1] if B == 2 else np.median(norm[:, 1:], axis=1).astype(f)
    scale = f(1) / np.maximum(f(1), norm / clip[:, None])
    want = np.zeros((C, n), f)
    for c in np.flatnonzero(sigma > 0):
        if B > 1:
            assert (scale[c, 1:] < 1).any() and (B < 3 or (scale[c, 1:] == 1).any()), (c, scale[c])
        total = rows[c, 0].copy()
        for k in range(1, B):
            g = rows[c, k].copy()
            for name, (lo, hi) in at.items():
                if name.startswith("dbias"):
                    g[lo:hi] *= scale[c, k]
            total = total + g
        want[c] = (total.astype(np.float64) + (z[:n] * np.float64(clip[c] * sigma[c]) + 0.0)).astype(f)
        want[c, lay.header_positions()] = lay.header_values()
    assert np.isfinite(want).all() and np.isfinite(sqsum).all()
    return clip, want


@functools.lru_cache(maxsize=None)
def _case(codec, classes, C, B):
    """a case's inputs, the plain call's rows and the reference: computed once, shared, not written to"""
    Bn = K.sample_tile() + 1 if B == "T+1" else B
    rng = np.random.default_rng(1000 * classes + 10 * C + Bn)
    model = _t(np.concatenate(G.model(41 + classes, classes)))
    x, lab = _t(G.images(12, N_IMAGES)), _t(rng.integers(0, classes, N_IMAGES).astype(np.int32))
    idx = rng.integers(0, N_IMAGES, (C, Bn)).astype(np.int32)
    sh = rng.integers(-1, 2, (C, Bn, 2)).astype(np.int32)
    rows = K.client_gradients_device(codec, classes, model, x, lab, idx=_t(idx.reshape(-1, 1)),
                                     shifts=_t(sh.reshape(-1, 1, 2))).cpu().numpy().reshape(C, Bn, -1)
    plain = K.client_gradients_device(codec, classes, model, x, lab, idx=_t(idx), shifts=_t(sh)).cpu().numpy()
    codec.check()
    sigma = np.array([SIGMAS[c % 3] for c in range(C)], f)
    clip, want = _reference(classes, rows, sigma, K.dp_noise_table())
    want[sigma == 0] = plain[sigma == 0]
    return dict(args=(model, x, lab), idx=idx, sh=sh, clip=clip, sigma=sigma, want=want)


def _device(codec, classes, case, **kw):
    return K.client_gradients_device(codec, classes, *case["args"], idx=_t(case["idx"]), shifts=_t(case["sh"]),
                                     clip=case["clip"], sigma=case["sigma"], **kw)


@pytest.mark.parametrize("classes,C,B", CASES)
def test_device_against_the_numpy_reference(codec, classes, C, B):
    case = _case(codec, classes, C, B)
    g = _device(codec, classes, case)
    codec.check()
    _same(g.cpu().numpy(), case["want"], (classes, C, B))


@pytest.mark.parametrize("chunk", [1, 2])
def test_chunk_walk_over_mixed_chunks(codec, chunk):
    case = _case(codec, 10, 3, 2)
    with K.chunk_override(chunk):
        g = _device(codec, 10, case)
        codec.check()
    _same(g.cpu().numpy(), case["want"], f"chunk {chunk}")


def test_host_form_and_resident_model_with_upload_rows(codec):
    import model_nets as N
    from fleet_amd.client import upload_texts
    from test_gpu_cifar import LAYERS
    import cifar_ref as R
    case = _case(codec, 10, 3, 2)
    model, x, lab = case["args"]
    m = model.cpu().numpy()
    w, b = m[:-666], m[-666:]
    host = K.client_gradients(codec, 10, w, b, x.cpu().numpy(), lab.cpu().numpy(), idx=case["idx"], shifts=case["sh"],
                              clip=case["clip"], sigma=case["sigma"])
    _same(host, case["want"], "host form")
    # the resident model holds what its text decodes to: the same call on those weights is the reference
    rm = F.ResidentModel(codec, N.mode0_text(LAYERS(10), R.B_SIZES[10], R.W_SIZES[10], w, b), 0, max_versions=2)
    want = _device(codec, 10, dict(case, args=(_t(np.concatenate(rm.export(-1))), x, lab))).cpu().numpy()
    g, ups = K.resident_client_gradients_device(rm, 10, -1, x, lab, idx=_t(case["idx"]), shifts=_t(case["sh"]),
                                                uploads=True, clip=case["clip"], sigma=case["sigma"])
    codec.check()
    _same(g.cpu().numpy(), want, "resident")
    assert (want[0] != want[1]).any() and np.isfinite(want).all()
    for c, text in enumerate(upload_texts(ups, K.grad_len(10))):
        assert text == codec.encode_floats(want[c]), c
    rm.close()


@pytest.mark.parametrize("clip,sigma", [([1.0], None), (None, [0.5]), ([1.0], [-0.5]), ([1.0], [np.inf]), ([1.0], [np.nan]),
                                        ([0.0], [0.5]), ([np.inf], [0.5])])
def test_refusals_before_any_launch(codec, clip, sigma):
    w, b = G.model(1, 10)
    x, lab, g = np.zeros((1, 3072), f), np.zeros(1, np.int32), np.full((1, K.grad_len(10)), -7.0, f)
    cp, sg = (None if v is None else np.array(v, f) for v in (clip, sigma))
    rc = codec._L.fleet_rgb_dp_grads(codec._live(), 10, w.ctypes.data, len(w), b.ctypes.data, len(b), x.ctypes.data, 1,
                                     3072, lab.ctypes.data, None, None, 1, 1, 2.0, None if cp is None else cp.ctypes.data,
                                     None if sg is None else sg.ctypes.data, g.ctypes.data, None, 0)
    assert rc == F.FLEET_ERR_ARG and (g == -7.0).all()
