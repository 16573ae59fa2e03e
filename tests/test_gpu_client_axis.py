"""Every launch form of the aggregation along the client-count axis: client counts on
each form's chunk and ring edges (client_axis.py: the M lists and the kernel constants
they follow), on two layouts of a few hundred values that still have two tiles at
widths 16 and 64, a ragged last group and header slots in several tiles.

Expected values are the oracle's: update_faithful (the per-op chain) for merged bytes,
decode_floats of it for merged_f32 (bitwise), encode_floats for encoded rows; Kardam's
side outputs through test_gpu_kardam_fused.check_side_outputs (the two-pass
kardam_grads, pinned to the oracle in test_updater.py; norms to its rtol 1e-12).
Everything else is byte-exact or bit-exact.

  1 update sweep        -- codec.update per plan x M list x layout x payload mix
  2 fused-step sweep    -- update_encode_device: merged, merged_f32 and EVERY next row
  3 Kardam sweep        -- update_kardam_device per plan x M list x layout
  4 k_kardam_reduce     -- 512 / 516, 2048 / 2052 and > 8192 partial slots per client
  5 rejection per form  -- a bad Base64 char / a layout mismatch in a late chunk or a
                           reused ring slot is reported, and leaves no residue
  6 off-domain, late    -- sums that leave the fast domain after 66 of 130 clients
"""
import numpy as np
import pytest
import torch

import client_axis as A
import fleet_amd as F
from fleet_amd.layouts import synthetic
from test_gpu_kardam_fused import PLANS as KD_PLANS
from test_gpu_kardam_fused import check_side_outputs

pytestmark = pytest.mark.gpu

NAMES = sorted(A.LAYOUTS)
# Kardam's flat tiles at W = 64 too (the list of test_gpu_kardam_fused forces 16 and 32)
KD_SWEEP_PLANS = KD_PLANS + ["update=tiled,flat_w2=64"]


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def rows_tensor(ups, pitch):
    host = np.zeros((len(ups), pitch), np.uint8)
    for c, u in enumerate(ups):
        host[c, : len(u)] = np.frombuffer(u, np.uint8)
    return torch.from_numpy(host).cuda()


def assert_update_form(spec, L):
    kernel, width, _ = A.UPDATE_FORMS[spec]
    assert F.update_kernel(L) == kernel, spec
    if width is not None:  # the flat tiles: every tile of the planned narrow width
        g = F.update_plan_grid(L)
        assert (g["kind"], g["n_a"], g["n_w"]) == ("flat", width, 0), (spec, g)


# 1 ------------------------------------------------------------------ update sweep

@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("spec", list(A.UPDATE_FORMS))
def test_update_sweep(codec, oracle, plan, spec, name):
    plan(spec)
    L = A.b64_len(A.LAYOUTS[name].n_up)
    assert_update_form(spec, L)
    for M in A.UPDATE_FORMS[spec][2]:
        for mix in A.MIXES:
            exp, exp_f32 = A.expected(oracle, name, mix, M)
            merged, f32 = codec.update(A.uploads(oracle, name, mix, M), A.dampen(M), want_f32=True)
            assert merged == exp, (spec, name, M, mix)
            assert same_bits(f32, exp_f32), (spec, name, M, mix)


# 2 -------------------------------------------------------------- fused-step sweep

_next = {}


def next_batch(oracle, name, M):
    """(values [M, 3 * groups], the oracle's Base64::encode of every row): the next
    batch's rows, one payload mix per client in turn (uploads of another seed)."""
    if (name, M) not in _next:
        lay = A.LAYOUTS[name]
        rows = np.zeros((M, 3 * A.groups_of(lay.n_up)), np.float32)
        for c in range(M):
            rows[c, : lay.n_up] = A.upload_values(oracle, name, c % 3, c, seed=A.SEED + 100)
        _next[(name, M)] = (rows, [oracle.encode_floats(rows[c, : lay.n_up]) for c in range(M)])
    return _next[(name, M)]


def fused_step(codec, oracle, name, M, ups, d):
    """One update_encode_device call on fresh output buffers: (merged bytes, merged_f32,
    next rows [M, pitch] as numpy); errors surface at check()."""
    lay = A.LAYOUTS[name]
    L, groups = A.b64_len(lay.n_up), A.groups_of(lay.n_up)
    text = rows_tensor(ups, 16 * groups)
    values_next = torch.from_numpy(next_batch(oracle, name, M)[0]).cuda()
    merged = torch.zeros(16 * groups, dtype=torch.uint8, device="cuda")
    f32 = torch.zeros(3 * groups, dtype=torch.float32, device="cuda")
    nxt = torch.zeros_like(text)
    codec.update_encode_device(text, L, d, lay.header_positions(), merged, f32, values_next, nxt)
    torch.cuda.synchronize()
    codec.check()
    return merged.cpu().numpy()[:L].tobytes(), f32.cpu().numpy()[: lay.n_up], nxt.cpu().numpy()


def assert_fused_exact(codec, oracle, name, M, mix, ctx):
    L = A.b64_len(A.LAYOUTS[name].n_up)
    exp, exp_f32 = A.expected(oracle, name, mix, M)
    merged, f32, nxt = fused_step(codec, oracle, name, M, A.uploads(oracle, name, mix, M), A.dampen(M))
    assert merged == exp, ctx
    assert same_bits(f32, exp_f32), ctx
    want = next_batch(oracle, name, M)[1]
    for c in range(M):  # every row: the second and the ragged row-blocks are under test
        assert nxt[c, :L].tobytes() == want[c], (ctx, c)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("spec", list(A.FUSED_FORMS))
def test_fused_step_sweep(codec, oracle, plan, spec, name):
    """fleet_codec.h makes no promise about the bytes of an output row past `len`, so they
    are not asserted on."""
    plan(spec)
    assert F.update_encode_kernel(A.b64_len(A.LAYOUTS[name].n_up)) == A.FUSED_FORMS[spec]
    for k, M in enumerate(A.M_FUSED):
        assert_fused_exact(codec, oracle, name, M, k % 3, (spec, name, M))


# 3 ------------------------------------------------------------------ Kardam sweep

@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("spec", KD_SWEEP_PLANS)
def test_kardam_sweep(codec, oracle, plan, spec, name):
    plan(spec)
    for M in A.kardam_m_list(spec):
        check_side_outputs(codec, oracle, A.LAYOUTS[name], M, dampen=A.dampen(M))


# 4 ------------------------------------------------- k_kardam_reduce instantiations

@pytest.mark.parametrize("spec,slots,n0", A.REDUCE_CASES)
def test_kardam_reduce_instantiations(codec, oracle, plan, spec, slots, n0):
    """k_kardam_reduce<64, 8> up to 512 partial slots per client, <64, 32> up to 2048,
    <256, 32> beyond, with its strided tail past 8192: the sizes either side of each
    edge. The slot count is held against the planner's grid, so a planner change cannot
    move a case to another instantiation unnoticed."""
    plan(spec)
    n = A.roundtrip_size(oracle, n0)
    g = F.update_plan_grid(A.b64_len(n))
    assert g["kind"] == "stream" and 4 * g["blocks"] == slots == A.stream_slots(spec, n), (spec, n, g)
    check_side_outputs(codec, oracle, synthetic(n), 2, rounds=("none", "all"))


# 5 ------------------------------------------------------------ rejection per form

def reject_cases(oracle, name):
    """(what, error class, uploads) of every corrupt batch of M_REJECT clients."""
    clean = A.uploads(oracle, name, 0, A.M_REJECT)
    out = []
    for c, pos, what in A.bad_char_cases(name):
        out.append((f"{what}, client {c}", F.Base64Error, clean[:c] + [A.corrupt_char(clean[c], pos)] + clean[c + 1:]))
    for c in A.LAYOUT_BAD_CLIENTS:
        out.append((f"layout, client {c}", F.LayoutError, clean[:c] + [A.mismatch_upload(oracle, name, c)] + clean[c + 1:]))
    return out


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("spec", list(A.UPDATE_FORMS))
def test_update_rejects(codec, oracle, plan, spec, name):
    plan(spec)
    assert_update_form(spec, A.b64_len(A.LAYOUTS[name].n_up))
    M, d = A.M_REJECT, A.dampen(A.M_REJECT)
    exp, exp_f32 = A.expected(oracle, name, 0, M)
    for what, err, ups in reject_cases(oracle, name):
        with pytest.raises(err):
            codec.update(ups, d, want_f32=True)
            pytest.fail(f"{spec}, {name}: {what} was merged")
        # no residue: the same context is exact on the clean uploads
        merged, f32 = codec.update(A.uploads(oracle, name, 0, M), d, want_f32=True)
        assert merged == exp and same_bits(f32, exp_f32), (spec, name, what)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("spec", list(A.FUSED_FORMS))
def test_fused_step_rejects(codec, oracle, plan, spec, name):
    """The fused step reports a corrupt upload at check() (never a half-written result as
    success), the error word is clean afterwards and the next step is exact."""
    plan(spec)
    assert F.update_encode_kernel(A.b64_len(A.LAYOUTS[name].n_up)) == A.FUSED_FORMS[spec]
    M, d = A.M_REJECT, A.dampen(A.M_REJECT)
    for what, err, ups in reject_cases(oracle, name):
        with pytest.raises(err):
            fused_step(codec, oracle, name, M, ups, d)
            pytest.fail(f"{spec}, {name}: {what} was merged")
        codec.check()  # reported once: no error word left set
        assert_fused_exact(codec, oracle, name, M, 0, (spec, name, what))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("spec", KD_SWEEP_PLANS)
def test_kardam_rejects(codec, oracle, plan, spec, name):
    plan(spec)
    lay = A.LAYOUTS[name]
    L, groups = A.b64_len(lay.n_up), A.groups_of(lay.n_up)
    M, d = A.M_REJECT, A.dampen(A.M_REJECT)
    exp, exp_f32 = A.expected(oracle, name, 0, M)
    clean = A.uploads(oracle, name, 0, M)
    _, want_ng, _ = codec.kardam_grads(clean, d, 0.05, None)

    def step(ups):
        merged = torch.zeros(16 * groups, dtype=torch.uint8, device="cuda")
        f32 = torch.zeros(3 * groups, dtype=torch.float32, device="cuda")
        ng, _ = codec.update_kardam_device(rows_tensor(ups, 16 * groups), L, d, lay.header_positions(), 0.05, merged,
                                           f32)
        codec.check()
        return merged.cpu().numpy()[:L].tobytes(), f32.cpu().numpy()[: lay.n_up], ng

    for what, err, ups in reject_cases(oracle, name):
        with pytest.raises(err):
            step(ups)
            pytest.fail(f"{spec}, {name}: {what} was merged")
        codec.check()
        merged, f32, ng = step(clean)
        assert merged == exp and same_bits(f32, exp_f32), (spec, name, what)
        np.testing.assert_allclose(ng, want_ng, rtol=1e-12, atol=0)


# 6 ---------------------------------------------------- off-domain after many chunks

_off = {}


def off_case(oracle, early):
    if early not in _off:
        ups = A.off_domain_uploads(oracle, early)
        exp = oracle.update_faithful(ups, A.dampen(A.M_OFF))
        _off[early] = (ups, exp, oracle.decode_floats(exp))
    return _off[early]


@pytest.mark.parametrize("early", [False, True], ids=["late", "early+late"])
@pytest.mark.parametrize("spec", list(A.UPDATE_FORMS))
def test_off_domain_after_many_chunks(codec, oracle, plan, spec, early):
    """The general-chain recompute (chain_general) of columns whose running sum reaches
    1e8 only after the rings have wrapped and many chunks have been consumed."""
    plan(spec)
    assert_update_form(spec, A.b64_len(A.LAYOUTS["hdrs"].n_up))
    ups, exp, exp_f32 = off_case(oracle, early)
    merged, f32 = codec.update(ups, A.dampen(A.M_OFF), want_f32=True)
    assert merged == exp, (spec, early)
    assert same_bits(f32, exp_f32), (spec, early)


@pytest.mark.parametrize("early", [False, True], ids=["late", "early+late"])
def test_off_domain_through_the_accumulator(codec, oracle, early):
    """The same 130 uploads pushed one by one (Codec.accumulator): the same bytes."""
    ups, exp, exp_f32 = off_case(oracle, early)
    with codec.accumulator(len(ups[0]), A.LAYOUTS["hdrs"].header_positions()) as acc:
        for u, f in zip(ups, A.dampen(A.M_OFF)):
            acc.push(u, f)
        assert acc.count == A.M_OFF
        merged, f32 = acc.finish(want_f32=True)
    assert merged == exp
    assert same_bits(f32, exp_f32)
