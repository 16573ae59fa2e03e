"""DPgradients and the distillation cost on the device beyond the fixture's shapes (DESIGN.md
§4.7): k_client_clip, k_client_sum_dp and k_client_sample_distill, and launch_client_grads_ex's
choice of kernels per chunk, bit for bit against the host mirror of the same source
(tests/native/check_client_dp.cpp --mirror over client_backward.h; tests/client_dp_jobs.py holds
the job list and says how its clips are chosen, tests/test_client_dp_mirror_cpu.py ties the
mirror to the reference's recorded bits). Every comparison is equality of bit patterns.

Clients carry samples, model rows, clips and sigmas of their own, at B - 1 = 0, 1, 2, 6 and 32;
the mirror's output must show, before anything runs on the device, that every job clips some
slots and not others and that slot 0's norm lies above a clip (check_conditions)."""
import subprocess

import numpy as np
import pytest

import client_dp_jobs as J
import eval_ref as E
import fleet_amd as F
from fleet_amd import client as K
from test_native_math import _clang

pytestmark = pytest.mark.gpu
f = np.float32
COST = {0: "cross_entropy", 1: "distillation"}


@pytest.fixture(scope="module")
def ex(tmp_path_factory):
    """{name: Expectation}: the mirror's rows and stats for the whole job list, computed once,
    its conditions checked"""
    clang = _clang()
    if clang is None:
        pytest.skip("no clang++ for the host build of client_backward.h")
    d = tmp_path_factory.mktemp("client_dp_shapes")
    exe = d / "check_client_dp"
    subprocess.check_call(J.compile_command(clang, exe))
    ex = J.expectations(lambda tag, jobs: J.run_mirror(exe, d, tag, jobs))
    J.check_conditions(ex)
    return ex


def _same(got, want, what):
    bad = J.bits(got) != J.bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def _dev(job):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
            dict(models=job.model_rows(), x=job.x, lab=job.lab, idx=job.idx, shifts=job.shifts, of=job.model_of).items()}


def _dp_kw(job):
    """the keywords of a call: clip and sigma only where the job has a DP client"""
    kw = dict(cost=COST[job.cost], temperature=job.temperature)
    if job.dp.any():
        kw.update(clip=job.clip, sigma=job.sigma)
    return kw


def _device(codec, job, t=None, **kw):
    t = t or _dev(job)
    return K.client_gradients_device(codec, t["models"], t["x"], t["lab"], idx=t["idx"], shifts=t["shifts"],
                                     model_of_client=t["of"], **{**_dp_kw(job), **kw})


def _run(codec, job, **kw):
    g = _device(codec, job, **kw)
    codec.check()
    return g.cpu().numpy()


# ------------------------------------------------------------------ (a) the shape sweep

@pytest.mark.parametrize("C,B", J.SWEEP)
def test_shape_sweep(codec, ex, C, B):
    """a mix of sigma = 0, 2^-60, 1/128 and 4 over two model rows, cross-entropy"""
    e = ex[f"{C}x{B}"]
    assert e.job.dp.any() and not e.job.dp.all() and len(set(e.job.model_of)) == 2
    _same(_run(codec, e.job), e.want.vec, f"C {C} B {B}")


@pytest.mark.parametrize("C,B", [(3, 2), (4, 3)])
def test_shape_sweep_host_form(codec, ex, C, B):
    """the host form takes one model: a call per model row, each compared on that row's clients"""
    e = ex[f"{C}x{B}"]
    j = e.job
    for m, (w, b) in enumerate(j.models):
        g = K.client_gradients(codec, w, b, j.x, j.lab, idx=j.idx, shifts=j.shifts, **_dp_kw(j))
        on = j.model_of == m
        assert on.any()
        _same(g[on], e.want.vec[on], f"C {C} B {B}, the clients of model {m}")


# ------------------------------------------------------------------ (b) distillation

@pytest.mark.parametrize("name", ["distill_3x2", "distill_3x2_plain", "distill_4x3", "distill_4x3_plain",
                                  "distill_3x2_t1"])
def test_distillation(codec, ex, name):
    e = ex[name]
    assert e.job.cost == 1 and e.job.temperature == (1.0 if name.endswith("t1") else 2.0)
    assert e.job.dp.any() != name.endswith("plain")
    _same(_run(codec, e.job), e.want.vec, name)


# ------------------------------------------------------------------ (c) the chunk walk

def test_chunk_walk(codec, ex):
    """sigma > 0, > 0, 0, 0, > 0: at chunk 2 a DP chunk, a chunk that takes k_client_sum and a
    DP tail of one client; chunk 1 and 3 mix the kinds another way, 0 and 5 take one chunk"""
    e = ex["walk"]
    assert list(e.job.dp) == [True, True, False, False, True]
    t = _dev(e.job)
    for chunk in (0, 1, 2, 3, 5):
        with K.client_chunk_override(chunk):
            g = _device(codec, e.job, t)
            codec.check()
        _same(g.cpu().numpy(), e.want.vec, f"chunk {chunk}")
    assert F.lib().fleet_client_grad_set_chunk(0) == 0  # the override was restored


# ------------------------------------------------------------------ (d) reuse on one context

def test_workspace_and_parameters_are_reused_across_calls(codec, ex):
    """DP 5x7, DP 3x2 with other clips and sigmas, plain 4x3 (no clip, no sigma), DP 5x7 again:
    the scales' offset behind the rows moves with chunk * B, clip and sigma are uploaded anew"""
    first, second, third = ex["5x7"], ex["reuse_3x2"], ex["4x3"]
    g1 = _run(codec, first.job)
    g2 = _run(codec, second.job)
    t = _dev(third.job)
    g3 = K.client_gradients_device(codec, t["models"], t["x"], t["lab"], idx=t["idx"], shifts=t["shifts"],
                                   model_of_client=t["of"])
    codec.check()
    g4 = _run(codec, first.job)
    _same(g1, first.want.vec, "DP 5x7")
    _same(g2, second.want.vec, "DP 3x2 after 5x7")
    _same(g3.cpu().numpy(), third.plain, "plain 4x3 after two DP calls")
    _same(g4, first.want.vec, "DP 5x7 again")
    _same(g4, g1, "the two runs of the first call")


# ------------------------------------------------------------------ (e) clip_scale's edges

def test_clip_scale_edges(codec, ex):
    """one client each: clip = slot 1's norm, one ulp below, one ulp above; the smallest
    subnormal clip (norm / clip overflows, scale 0); the smallest subnormal sigma (DP on the
    host, so DP on the device: no flushed denormal); a model whose rows are finite and whose
    sqsum is +inf (scale 0). Slot 2 of every client is clipped or zeroed, so every row differs
    from its plain twin."""
    e = ex["edges"]
    j, st, norms = e.job, e.want.stats, e.norms
    one, below = f(1.0), np.nextafter(f(1.0), f(0))
    assert (j.sigma[[0, 1, 2, 3, 5]] == J.SIGMA_TINY).all() and j.sigma[4] == J.SUBNORMAL > 0
    assert j.clip[0] == norms[0, 1] and st[0, 2, 1] == one
    assert j.clip[1] < norms[1, 1] and np.nextafter(j.clip[1], f(np.inf)) == norms[1, 1] and f(1 - 2.0 ** -22) <= st[1, 2, 1] < one
    assert j.clip[2] > norms[2, 1] and np.nextafter(j.clip[2], f(0)) == norms[2, 1] and st[2, 2, 1] == one
    for c in (0, 1, 2):
        assert 0 < st[c, 2, 2] < below, c
    assert j.clip[3] == J.SUBNORMAL and (st[3, 2, 1:] == 0).all() and np.isfinite(st[3, 1, 1:]).all()
    assert (j.clip[4] < norms[4, 1:]).all() and (st[4, 2, 1:] < 1).all() and (st[4, 2, 1:] > 0).all()
    assert j.model_of[5] == 2 and np.isposinf(st[5, 0, 1:]).all() and (st[5, 2, 1:] == 0).all()
    assert not e.want.blown.any() and not np.isnan(e.want.vec).any()  # E is finite for every sample
    assert np.isfinite(e.plain[5, J.BIAS_START:]).all()  # the rows that are scaled hold no inf to make a NaN of
    for c in range(6):
        assert (J.bits(e.want.vec[c, J.BIAS_START:]) != J.bits(e.plain[c, J.BIAS_START:])).any(), c
    got = _run(codec, j)  # check() raises nothing
    for c in range(6):
        _same(got[c], e.want.vec[c], f"edge client {c}")


# ------------------------------------------------------------------ (f) pitches and a stream

def test_pitches_and_an_explicit_stream(codec, ex):
    """grad_pitch 22961 + 7, F = 800, model_pitch 21530 + 6, the padding of the inputs NaN, on a
    stream that is not the current one"""
    import torch
    e = ex["3x2"]
    j = e.job
    sentinel = f(-12345.5)
    x = np.full((len(j.x), 800), np.nan, f)
    x[:, :784] = j.x
    rows = np.full((len(j.models), J.N_ROW + 6), np.nan, f)
    rows[:, :J.N_ROW] = j.model_rows()
    t = _dev(j)
    t["x"], t["models"] = torch.from_numpy(x).cuda(), torch.from_numpy(rows).cuda()
    grads = torch.full((j.C, J.N_UP + 7), float(sentinel), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    s.wait_stream(torch.cuda.current_stream())  # the uploads above
    out = _device(codec, j, t, grads=grads, stream=s.cuda_stream)
    assert out.data_ptr() == grads.data_ptr()
    s.synchronize()
    codec.check(stream=s.cuda_stream)
    g = grads.cpu().numpy()
    _same(g[:, :J.N_UP], e.want.vec, "rows at a pitch")
    assert (g[:, J.N_UP:] == sentinel).all()


# ------------------------------------------------------------------ (g) the resident form

def test_resident_form(codec):
    """resident_client_gradients_device on versions [None, -1, 0] after one step, C = 3, B = 3,
    distinct samples per client, sigma = 0, 2^-60 and 1/128: each row is client_gradients' on
    the exported weights, under both costs. The 2^-60 client's clip of 1 lies below every norm,
    so its row differs from the plain one in a bias block only by clipping."""
    import torch
    inp = J.inputs()
    x, lab = inp["x"], inp["lab"]
    idx, sh = J._draw(3, 3, len(x), 570, distinct=True)
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    di, ds = torch.from_numpy(idx).cuda(), torch.from_numpy(sh).cuda()
    rm = F.ResidentModel(codec, E.seeded_text(), distillation_mode=1, max_versions=3)
    rm.initUpdater([0.5])
    g0, up = K.resident_client_gradients_device(rm, None, dx, dl, idx=di, shifts=ds, uploads=True)
    codec.check()
    rm.descentNative(codec.update(K.upload_texts(up), [1.0, 1.0, 1.0]), 4, 2)
    assert rm.modelsSize() == 2
    versions = [None, -1, 0]
    clip, sigma = np.array([1.0, 1.0, 35.0], f), np.array([0.0, J.SIGMA_TINY, 1.0 / 128], f)
    for cost in ("cross_entropy", "distillation"):
        g = K.resident_client_gradients_device(rm, versions, dx, dl, idx=di, shifts=ds, cost=cost, clip=clip, sigma=sigma)
        codec.check()
        plain = K.resident_client_gradients_device(rm, versions, dx, dl, idx=di, shifts=ds, cost=cost)
        codec.check()
        g, plain = g.cpu().numpy(), plain.cpu().numpy()
        for c, v in enumerate(versions):
            mw, mb = rm.export(rm.modelsSize() - 1 if v is None else v)
            one = K.client_gradients(codec, mw, mb, x, lab, idx=idx[c], shifts=sh[c], cost=cost, clip=clip[c],
                                     sigma=sigma[c])[0]
            _same(g[c], one, f"{cost}, version {v}")
        _same(g[0], plain[0], f"{cost}: the sigma = 0 client")
        for c in (1, 2):
            assert (J.bits(g[c, J.BIAS_START:]) != J.bits(plain[c, J.BIAS_START:])).any(), (cost, c)
        felt = np.abs(plain[1, :J.BIAS_START]) > 2.0 ** -20  # a noise of 2^-60 z changes only sums near zero
        assert felt.any() and not (J.bits(g[1, :J.BIAS_START]) != J.bits(plain[1, :J.BIAS_START]))[felt].any()  # no dW block is scaled
    rm.close()


# ------------------------------------------------------------------ (h) upload rows

def test_upload_rows(codec, ex):
    e = ex["4x3"]
    g, up = _device(codec, e.job, uploads=True)
    codec.check()
    _same(g.cpu().numpy(), e.want.vec, "rows")
    texts = K.upload_texts(up)
    assert len(texts) == 4
    for c, text in enumerate(texts):
        assert text == codec.encode_floats(e.want.vec[c]), c


# ------------------------------------------------------------------ (i) a blown model beside sound ones

def test_a_blown_model_leaves_its_neighbours_alone(codec, ex):
    """client 1's forward is NaN (an inf pair in FC2): check() says so, and rows 0 and 2, both
    DP and both clipped, are the mirror's; row 1 is unspecified and not looked at"""
    e = ex["blown"]
    j = e.job
    assert j.dp.all() and list(e.want.blown > 0) == [False, True, False]
    assert not np.isnan(e.want.vec[[0, 2]]).any() and (e.want.stats[[0, 2], 2, 1] < 1).all()
    g = _device(codec, j)
    with pytest.raises(F.FleetError) as err:
        codec.check()
    assert err.value.code == F.FLEET_ERR_ARG and "blew up" in str(err.value)
    codec.check()  # the bit was read and cleared
    g = g.cpu().numpy()
    for c in (0, 2):
        _same(g[c], e.want.vec[c], f"client {c} beside the blown one")
