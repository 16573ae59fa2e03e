"""DPgradients and the distillation cost on the device: k_client_clip,
k_client_sum_dp and k_client_sample_distill through every entry point, bit for bit against
tests/golden/client_dp_ref.npz (recorded from the reference's own network class). Only the
fixture's shapes run here: B <= 4, C <= 3, the clients of a call on the same samples and model row.
tests/test_gpu_client_dp_shapes.py runs the shapes beyond them (clients with samples, model rows,
clips and sigmas of their own, B up to 33, the chunk walk over mixed chunks, clip_scale's edges)
against the host mirror of the same source."""
import numpy as np
import pytest

import client_dp_ref as R
import eval_ref as E
import fleet_amd as F
from fleet_amd import client as K
from fleet_amd.layouts import MNIST

pytestmark = pytest.mark.gpu
f = np.float32
COST = {0: "cross_entropy", 1: "distillation"}


@pytest.fixture(scope="module")
def z():
    return R.load()


@pytest.fixture(scope="module")
def inputs():
    """the fixture's model and its eight images, labels and shifts, on the host and the device"""
    import torch
    w, b = R.model()
    x, lab, sh = R.G.images(), R.G.labels(), R.shifts8()
    dev = dict(models=torch.from_numpy(np.concatenate([w, b])).cuda(), x=torch.from_numpy(x).cuda(),
               lab=torch.from_numpy(lab).cuda())
    return w, b, x, lab, sh, dev


def _same(got, want, what):
    bad = R.bits(got) != R.bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def _dp_kw(cost, clip, sigma):
    return dict(cost=COST[cost], **(dict(clip=clip, sigma=sigma) if sigma > 0 else {}))


def _against_fixture(z, name, row):
    _same(row[R.G_I1], z[f"{name}_grad_i1"], f"{name}: I1 bias block")
    _same(row[R.G_FC2], z[f"{name}_grad_fc2"], f"{name}: FC2 bias block")
    if name in R.FULL:
        _same(row, z[f"{name}_grad"], name)
    assert R.sha(row) == R.sha_of(z, f"{name}_grad_sha256"), name
    assert np.array_equal(row[MNIST.header_positions()], np.array(MNIST.header_values(), f)), name


@pytest.fixture(scope="module")
def singles(codec, inputs):
    """the three clients of the fleet tests, each through a call of its own on the bare
    weights: sigma = 0, c's parameters, d's parameters, all on c's samples"""
    w, b, x, lab, sh, dev = inputs
    pick = R.PICK_C
    params = [(0.0, 0.0), (R.CLIP_C, R.SIGMA_C), (R.CLIP_D, R.SIGMA_D)]
    rows = [K.client_gradients(codec, w, b, x[pick], lab[pick], shifts=sh[pick], clip=c, sigma=s)[0] for c, s in params]
    return np.stack(rows), np.array([p[0] for p in params], f), np.array([p[1] for p in params], f)


def _fleet(inputs):
    import torch
    w, b, x, lab, sh, dev = inputs
    idx = np.array([R.PICK_C] * 3, np.int32)
    shifts = np.ascontiguousarray(np.stack([sh[R.PICK_C]] * 3))
    return torch.from_numpy(idx).cuda(), torch.from_numpy(shifts).cuda()


def test_every_fixture_case_through_the_bare_weights_form(codec, z, inputs):
    """(a)-(f) through fleet_client_ex_grads, C = 1: equal in bits"""
    w, b = inputs[:2]
    for name, B, cost, clip, sigma, x, lab, sh in R.cases():
        g = K.client_gradients(codec, w, b, x, lab, shifts=sh, temperature=R.TEMPERATURE, **_dp_kw(cost, clip, sigma))
        assert g.shape == (1, R.N_UP)
        _against_fixture(z, name, g[0])


def test_three_clients_in_one_call_and_the_chunk_walk(codec, z, inputs, singles):
    """one call with the clients (sigma = 0, c, d) equals the three single-client calls, also
    with the chunk forced to 1 and to 2; the sigma = 0 row is the existing entry point's"""
    w, b, x, lab, sh, dev = inputs
    want, clip, sigma = singles
    _against_fixture(z, "c", want[1])
    _against_fixture(z, "d", want[2])
    plain = K.client_gradients(codec, w, b, x[R.PICK_C], lab[R.PICK_C], shifts=sh[R.PICK_C])[0]
    _same(want[0], plain, "sigma = 0 against the existing entry point")
    di, ds = _fleet(inputs)
    for chunk in (0, 1, 2):
        with K.client_chunk_override(chunk):
            g = K.client_gradients_device(codec, dev["models"], dev["x"], dev["lab"], idx=di, shifts=ds, clip=clip,
                                          sigma=sigma)
            codec.check()
        _same(g.cpu().numpy(), want, f"chunk {chunk}")


def test_upload_rows_decode_to_the_rows(codec, inputs, singles):
    """the upload rows are Base64::encode of the fp32 rows, byte for byte, and decode to what
    the encoded rows decode to (the text keeps a float's leading digits only, so a decoded row
    is not the row in bits)"""
    w, b, x, lab, sh, dev = inputs
    want, clip, sigma = singles
    di, ds = _fleet(inputs)
    g, up = K.client_gradients_device(codec, dev["models"], dev["x"], dev["lab"], idx=di, shifts=ds, clip=clip,
                                      sigma=sigma, uploads=True)
    codec.check()
    _same(g.cpu().numpy(), want, "rows")
    for c, text in enumerate(K.upload_texts(up)):
        assert text == codec.encode_floats(want[c]), c
        _same(codec.decode_floats(text), codec.decode_floats(codec.encode_floats(want[c])), f"upload row {c} decoded")


def test_resident_model_versions(codec, inputs):
    """resident_client_gradients_device over versions [None, -1, 0] with (sigma = 0, c, d) and
    under the distillation cost equals the bare-weights form on those versions' rows"""
    import torch
    w, b, x, lab, sh, dev = inputs
    rm = F.ResidentModel(codec, E.seeded_text(), distillation_mode=1, max_versions=3)
    rm.initUpdater([0.5])
    di, ds = _fleet(inputs)
    clip, sigma = np.array([1.0, R.CLIP_C, R.CLIP_D], f), np.array([0.0, R.SIGMA_C, R.SIGMA_D], f)
    g0, up = K.resident_client_gradients_device(rm, None, dev["x"], dev["lab"], idx=di, shifts=ds, uploads=True)
    codec.check()
    rm.descentNative(codec.update(K.upload_texts(up), [1.0, 1.0, 1.0]), 4, 2)
    assert rm.modelsSize() == 2
    versions = [None, -1, 0]
    pick = R.PICK_C
    for cost in ("cross_entropy", "distillation"):
        g = K.resident_client_gradients_device(rm, versions, dev["x"], dev["lab"], idx=di, shifts=ds, cost=cost, clip=clip,
                                               sigma=sigma)
        codec.check()
        g = g.cpu().numpy()
        for c, v in enumerate(versions):
            mw, mb = rm.export(rm.modelsSize() - 1 if v is None else v)
            one = K.client_gradients(codec, mw, mb, x[pick], lab[pick], shifts=sh[pick], cost=cost, clip=clip[c],
                                     sigma=sigma[c])[0]
            _same(g[c], one, f"{cost}, version {v}")
    rm.close()


def test_default_keywords_are_the_existing_entry_point(codec, inputs):
    w, b, x, lab, sh, dev = inputs
    di, ds = _fleet(inputs)
    L, h = codec._L, codec._live()
    import torch
    old = torch.empty((3, R.N_UP), dtype=torch.float32, device="cuda")
    codec._check(L.fleet_client_grads_device(h, dev["models"].data_ptr(), dev["models"].numel(), 1, None,
                                             dev["x"].data_ptr(), 8, 784, dev["lab"].data_ptr(), di.data_ptr(),
                                             ds.data_ptr(), 3, 4, 2.0, old.data_ptr(), R.N_UP, None, 0, None))
    new = K.client_gradients_device(codec, dev["models"], dev["x"], dev["lab"], idx=di, shifts=ds, cost="cross_entropy",
                                    clip=None, sigma=None)
    zero = K.client_gradients_device(codec, dev["models"], dev["x"], dev["lab"], idx=di, shifts=ds, clip=1.0, sigma=0.0)
    codec.check()
    torch.cuda.synchronize()
    _same(new.cpu().numpy(), old.cpu().numpy(), "default keywords")
    _same(zero.cpu().numpy(), old.cpu().numpy(), "sigma = 0 for every client")


def test_refusals_come_before_any_launch_and_leave_the_outputs(codec, inputs):
    """an unknown cost; one of clip / sigma without the other; a negative or non-finite sigma;
    with sigma > 0 a clip that is <= 0 or non-finite: FLEET_ERR_ARG from the three forms, the
    output rows untouched, no device error pending"""
    import torch
    w, b, x, lab, sh, dev = inputs
    L, h = codec._L, codec._live()
    di, ds = _fleet(inputs)
    rm = F.ResidentModel(codec, E.seeded_text(), distillation_mode=1, max_versions=2)
    versions = np.array([-1, -1, -1], np.int32)
    ok = np.array([1.0, 1.0, 1.0], f)
    nan, inf = float("nan"), float("inf")

    def arr(v):
        return None if v is None else np.array(v, f)
    bad = [dict(cost=2), dict(cost=-1), dict(clip=None, sigma=ok), dict(clip=ok, sigma=None),
           dict(sigma=[0.5, -0.5, 0.5]), dict(sigma=[0.5, nan, 0.5]), dict(sigma=[inf, 0.5, 0.5]),
           dict(sigma=[0.0, 0.0, -0.0 - 1e-30]),
           dict(clip=[1.0, 0.0, 1.0]), dict(clip=[1.0, 1.0, -2.0]), dict(clip=[inf, 1.0, 1.0]), dict(clip=[1.0, nan, 1.0])]
    good = [dict(), dict(clip=[0.0, -1.0, nan], sigma=[0.0, 0.0, 0.0])]  # a clip is not looked at where sigma is 0
    sentinel = 12345.0
    hg = np.full((3, R.N_UP), sentinel, f)
    dg = torch.full((3, R.N_UP), sentinel, dtype=torch.float32, device="cuda")
    idx, shifts = di.cpu().numpy(), ds.cpu().numpy()

    def calls(cost=0, clip=ok, sigma=ok):
        clip, sigma = arr(clip), arr(sigma)
        pc, ps = (None if clip is None else clip.ctypes.data), (None if sigma is None else sigma.ctypes.data)
        return (L.fleet_client_ex_grads(h, w.ctypes.data, len(w), b.ctypes.data, len(b), x.ctypes.data, 8, 784,
                                        lab.ctypes.data, idx.ctypes.data, shifts.ctypes.data, 3, 4, 2.0, cost, pc, ps,
                                        hg.ctypes.data, None, 0),
                L.fleet_client_ex_grads_device(h, dev["models"].data_ptr(), dev["models"].numel(), 1, None,
                                               dev["x"].data_ptr(), 8, 784, dev["lab"].data_ptr(), di.data_ptr(),
                                               ds.data_ptr(), 3, 4, 2.0, cost, pc, ps, dg.data_ptr(), R.N_UP, None, 0,
                                               None),
                rm._L.fleet_rmodel_client_ex_grads_device(rm._live(), versions.ctypes.data, dev["x"].data_ptr(), 8, 784,
                                                          dev["lab"].data_ptr(), di.data_ptr(), ds.data_ptr(), 3, 4, 2.0,
                                                          cost, pc, ps, dg.data_ptr(), R.N_UP, None, 0, None))
    for kw in bad:
        assert calls(**kw) == (F.FLEET_ERR_ARG,) * 3, kw
    codec.check()  # nothing was launched: no device error is pending
    torch.cuda.synchronize()
    assert (hg == sentinel).all() and bool((dg == sentinel).all())
    for kw in good:
        assert calls(**kw) == (F.FLEET_OK,) * 3, kw
    codec.check()
    torch.cuda.synchronize()
    assert not (hg == sentinel).any() and not bool((dg == sentinel).any())
    # and through the Python keywords
    with pytest.raises(F.FleetError) as e:
        K.client_gradients(codec, w, b, x[:2], lab[:2], clip=1.0, sigma=-1.0)
    assert e.value.code == F.FLEET_ERR_ARG
    with pytest.raises(ValueError):
        K.client_gradients(codec, w, b, x[:2], lab[:2], cost="hinge")
    rm.close()
