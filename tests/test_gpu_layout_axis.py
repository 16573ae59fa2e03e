"""The layout axis: header-dense layouts (layout_axis.dense, about 2.2 values per header)
through every form that takes a header list, at the header counts where a kernel takes
another path -- tile_init's strided iterations over the list (from 64 * NW headers), the
accumulator's search in global memory (past kAccLdsHdr), a second k_descent chunk (past
kMaxDescentSegs segments), the cap of FLEET_MAX_HEADERS -- with groups of two and three
header slots on wave, tile and block edges. Every expected value is the oracle's
(update_faithful, update_fused with the header mask, its per-op natives, descent,
synth_upload), never another plan or form of the library; the inputs are validated in
test_layout_axis_inputs.py. The last section holds the device-resident entry points to
their header-list contract (include/fleet_codec.h): a refused list launches nothing."""
import numpy as np
import pytest

import fleet_amd as F
import layout_axis as A
from test_gpu_acc_burst import policy, same_bits
from test_gpu_fuzz import FUSED_PLANS, KD_PLANS, PLANS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = 0xA5  # what an output buffer holds where nothing may be written


def rows_of(ups, pitch=None, lead=0):
    """The uploads as a uint8 CUDA tensor [M, pitch], zero past each upload's length; with
    `lead` rows of another allocation's bytes before them (the tensor is then a slice)."""
    L = len(ups[0])
    pitch = pitch or 16 * ((L + 15) // 16)
    host = np.zeros((lead + len(ups), pitch), np.uint8)
    for c, u in enumerate(ups):
        host[lead + c, :L] = np.frombuffer(u, np.uint8)
    return torch.from_numpy(host).cuda()[lead:]


def outputs(lay, lead=0):
    G = A.groups_of(lay.n_up)
    merged = torch.full((16 * (G + lead),), FILL, dtype=torch.uint8, device="cuda")[16 * lead:]
    f32 = torch.full((3 * (G + lead),), -7.0, dtype=torch.float32, device="cuda")[3 * lead:]
    return merged, f32


def assert_merged(lay, merged, f32, exp, exp32, gb=0, ge=None):
    """Groups [gb, ge) of the device outputs hold the oracle's bytes and values."""
    L = len(exp)
    ge = A.groups_of(lay.n_up) if ge is None else ge
    b0, b1 = min(L, 16 * gb), min(L, 16 * ge)
    assert merged.cpu().numpy()[b0:b1].tobytes() == exp[b0:b1]
    v0, v1 = 3 * gb, min(lay.n_up, 3 * ge)
    if f32 is not None:
        assert same_bits(f32.cpu().numpy()[v0:v1], exp32[v0:v1])


def plan_nw(spec):
    """Waves per block of the tile form a plan runs at these sizes (tile_init's stride is 64 * NW)."""
    if "weave6" in spec or "weave8" in spec:
        return int(spec[-1])
    if "tiled" in spec:
        return A.NW_TILED
    return A.NW_PIPE  # the default plan and update=pipe; the stream kernel searches the list instead


# 2 ------------------------------------------------------------------- batch update

@pytest.mark.parametrize("H", A.EDGES)
@pytest.mark.parametrize("spec", PLANS)
def test_update_at_every_edge(codec, oracle, plan, spec, H):
    lay = A.dense(H)
    ups, d = A.uploads(oracle, lay, 3), A.dampen(3)
    exp, exp32 = A.expected(oracle, lay, 3)
    plan(spec)
    merged, f32 = codec.update(ups, d, want_f32=True)
    assert merged == exp, (spec, H)
    assert same_bits(f32, exp32), (spec, H)


@pytest.mark.parametrize("spec", PLANS)
def test_update_with_wrapping_client_chunks(codec, oracle, plan, spec):
    """70 clients: the tiles' client chunks and the pipelined ring wrap, the header list is
    longer than the accumulator's and every tile form's first iteration."""
    lay = A.dense(1025)
    ups, d = A.uploads(oracle, lay, 70), A.dampen(70)
    exp, exp32 = A.expected(oracle, lay, 70)
    plan(spec)
    merged, f32 = codec.update(ups, d, want_f32=True)
    assert merged == exp and same_bits(f32, exp32)


def windows_of(lay):
    """[0, 64), [64, 65), [65, b), [b, G): the first ends and the third begins inside the
    header run of groups 63 .. 64, the second holds three header slots and nothing else."""
    a, b = A.window_cuts(lay)
    assert A.header_bits(lay)[a] == 7
    return [(0, a), (a, a + 1), (a + 1, b), (b, A.groups_of(lay.n_up))]


@pytest.mark.parametrize("H", [1025, 4096])
@pytest.mark.parametrize("spec", ["update=stream", "update=tiled", "update=pipe"])
def test_update_device_windows(codec, oracle, plan, spec, H):
    lay = A.dense(H)
    ups, d = A.uploads(oracle, lay, 3), A.dampen(3)
    exp, exp32 = A.expected(oracle, lay, 3)
    L, hp = len(exp), lay.header_positions()
    t = rows_of(ups)
    plan(spec)
    whole_m = np.full(16 * A.groups_of(lay.n_up), FILL, np.uint8)
    whole_v = np.full(3 * A.groups_of(lay.n_up), -7.0, np.float32)
    for gb, ge in windows_of(lay):
        merged, f32 = outputs(lay)
        codec.update_device(t, L, d, hp, merged, f32, gb, ge)
        codec.check()
        m, v = merged.cpu().numpy(), f32.cpu().numpy()
        assert (m[: 16 * gb] == FILL).all() and (m[16 * ge:] == FILL).all(), (gb, ge)  # nothing outside the window
        assert (v[: 3 * gb] == -7.0).all() and (v[3 * ge:] == -7.0).all(), (gb, ge)
        whole_m[16 * gb: 16 * ge] = m[16 * gb: 16 * ge]
        whole_v[3 * gb: 3 * ge] = v[3 * gb: 3 * ge]
    assert whole_m[:L].tobytes() == exp
    assert same_bits(whole_v[: lay.n_up], exp32)


@pytest.fixture(scope="module")
def contexts():
    cs = [F.Codec(0) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


@pytest.mark.parametrize("H", [1025, 4096])
def test_update_multi_cuts_a_header_run(contexts, oracle, H):
    """Three contexts on device 0 (test_gpu_multi.py): the second one's window begins
    between two three-header groups."""
    lay, cut = A.dense_cut_for(H)
    from fleet_amd.shard import group_range
    assert group_range(A.groups_of(lay.n_up), 3, 1)[0] == cut
    ups, d = A.uploads(oracle, lay, 3), A.dampen(3)
    exp, exp32 = A.expected(oracle, lay, 3)
    merged, f32 = F.update_multi(contexts, ups, d, want_f32=True)
    assert merged == exp and same_bits(f32, exp32)


@pytest.mark.parametrize("H", [257, 577, 4096])
@pytest.mark.parametrize("spec", FUSED_PLANS)
def test_fused_step(codec, oracle, plan, spec, H):
    lay = A.dense(H)
    M = 3
    ups, d = A.uploads(oracle, lay, M), A.dampen(M)
    exp, exp32 = A.expected(oracle, lay, M)
    L, G = len(exp), A.groups_of(lay.n_up)
    nxt = np.zeros((M, 3 * G), np.float32)
    for c in range(M):
        nxt[c, : lay.n_up] = A.upload_values(oracle, lay, c, seed=A.SEED + 1)
    t, values = rows_of(ups), torch.from_numpy(nxt).cuda()
    merged, f32 = outputs(lay)
    nxt_text = torch.zeros_like(t)
    plan(spec)
    codec.update_encode_device(t, L, d, lay.header_positions(), merged, f32, values, nxt_text)
    codec.check()
    assert_merged(lay, merged, f32, exp, exp32)
    want = A.uploads(oracle, lay, M, seed=A.SEED + 1)
    got = nxt_text.cpu().numpy()
    for c in range(M):
        assert got[c, :L].tobytes() == want[c], (spec, H, c)


@pytest.mark.parametrize("where", ["second of three", "last"])
@pytest.mark.parametrize("spec", PLANS)
def test_layout_mismatch(codec, oracle, plan, spec, where):
    """One upload whose header code at index j differs (layout_axis.mismatch): j = 0, the
    first index of tile_init's second iteration under this plan's form, the last. As the
    last upload it is the one the host walk reads, so the other two then differ from it."""
    H = 1025
    lay = A.dense(H)
    ups, d = A.uploads(oracle, lay, 3), A.dampen(3)
    plan(spec)
    for j in (0, 64 * plan_nw(spec), H - 1):
        bad = list(ups)
        c = 1 if where == "second of three" else 2
        bad[c] = A.mismatch_upload(oracle, lay, j, c)
        with pytest.raises(F.LayoutError) as ei:
            codec.update(bad, d)
        assert ei.value.code == F.FLEET_ERR_LAYOUT, (spec, j)
    assert codec.update(ups, d) == A.expected(oracle, lay, 3)[0]


# 3 ------------------------------------------------------------------------ Kardam

@pytest.mark.parametrize("H", [257, 577, 4096])
@pytest.mark.parametrize("spec", KD_PLANS)
def test_kardam_side_outputs(codec, oracle, plan, spec, H):
    """A wave mixes header, flat and ragged lanes, and flat positions sit behind thousands
    of headers; check_side_outputs holds G bit for bit and the norms to 1e-12 relative."""
    from test_gpu_kardam_fused import check_side_outputs
    plan(spec)
    check_side_outputs(codec, oracle, A.dense(H), 3)


@pytest.mark.parametrize("H", [257, 4096])
def test_kardam_grads_vs_the_per_op_chain(codec, oracle, H):
    lay = A.dense(H)
    M, lr = 3, 0.05
    ups, d = A.uploads(oracle, lay, M), A.dampen(M)

    def chain(us):
        return [oracle.scalar_mul(oracle.scalar_mul(oracle.flat_gradient(u), f), lr) for u, f in zip(us, d)]
    want = chain(ups)
    prev = chain(A.uploads(oracle, lay, M, seed=A.SEED + 2))
    prev[1] = None
    texts, ng, nd = codec.kardam_grads(ups, d, lr, prev)
    for c in range(M):
        assert texts[c] == want[c], (H, c)
        assert ng[c] == pytest.approx(oracle.norm(want[c]), rel=1e-12)
        if prev[c] is None:
            assert np.isnan(nd[c])
        else:
            assert nd[c] == pytest.approx(oracle.norm(oracle.subtract(want[c], prev[c])), rel=1e-12)


# 4 ---------------------------------------------------------- per-op natives, the cap

@pytest.mark.parametrize("H", [257, 1025, 4096])
def test_per_op_natives(codec, oracle, H):
    lay = A.dense(H)
    ups = A.uploads(oracle, lay, 2)
    pos, n_up = codec.layout_parse(ups[0])
    assert pos.tolist() == lay.header_positions() and n_up == lay.n_up
    flat = codec.getFlatGradient(ups[0])
    assert flat == oracle.flat_gradient(ups[0])
    assert codec.mergeFlatGradient(ups[1], flat) == oracle.merge_flat_gradient(ups[1], flat)


def test_one_header_past_the_cap(codec, oracle):
    over, lay = A.dense(F.FLEET_MAX_HEADERS + 1), A.dense(F.FLEET_MAX_HEADERS)
    bad, ups, d = A.uploads(oracle, over, 3), A.uploads(oracle, lay, 3), A.dampen(3)
    flat = oracle.flat_gradient(bad[0])  # the oracle has no cap
    for call in (lambda: codec.layout_parse(bad[0]), lambda: codec.getFlatGradient(bad[0]),
                 lambda: codec.mergeFlatGradient(bad[1], flat), lambda: codec.update(bad, d)):
        with pytest.raises(F.LayoutError) as ei:
            call()
        assert ei.value.code == F.FLEET_ERR_LAYOUT
        # a following good call on the same context is unaffected
        assert codec.layout_parse(ups[0])[0].tolist() == lay.header_positions()
    assert codec.getFlatGradient(ups[0]) == oracle.flat_gradient(ups[0])
    assert codec.update(ups, d) == A.expected(oracle, lay, 3)[0]


def test_header_lists_past_the_cap_are_refused(codec, oracle):
    """n_headers = 4097 at the device-resident entry points: FLEET_ERR_ARG, nothing launched."""
    over = A.dense(F.FLEET_MAX_HEADERS + 1)
    ups, d = A.uploads(oracle, over, 3), A.dampen(3)
    L, hp = len(ups[0]), over.header_positions()
    with pytest.raises(F.FleetError) as ei:
        codec.accumulator(L, hp)
    assert ei.value.code == F.FLEET_ERR_ARG
    t = rows_of(ups)
    merged, f32 = outputs(over)
    with pytest.raises(F.FleetError) as ei:
        codec.update_device(t, L, d, hp, merged, f32)
    assert ei.value.code == F.FLEET_ERR_ARG
    values = torch.full((2, over.n_up + 3), -7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(F.FleetError) as ei:
        codec.synth_device(5, values, over.n_up, hp, over.header_values())
    assert ei.value.code == F.FLEET_ERR_ARG
    codec.check()
    torch.cuda.synchronize()
    assert (merged == FILL).all() and (f32 == -7.0).all() and (values == -7.0).all()


# 5 ------------------------------------------------------------ streaming accumulator

ACC_H = [1023, 1024, 1025, 4096]
ACC_M = 5


def acc_case(oracle, H):
    lay = A.dense(H)
    d = policy("inverse", ACC_M)
    exp, exp32 = A.expected(oracle, lay, ACC_M, d)
    return lay, A.uploads(oracle, lay, ACC_M), d, exp, exp32


@pytest.mark.parametrize("close", ["push_finish", "finish"])
@pytest.mark.parametrize("parts", [[5], [1, 4], [2, 3], [1] * 5], ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("H", ACC_H)
def test_acc_partitions(codec, oracle, H, parts, close):
    """test_gpu_acc_burst.test_partitions on header lists either side of kAccLdsHdr."""
    lay, ups, d, exp, exp32 = acc_case(oracle, H)
    with codec.accumulator(len(ups[0]), lay.header_positions()) as acc:
        i = 0
        for j, k in enumerate(parts):
            u, f = ups[i: i + k], d[i: i + k]
            assert acc.count == i
            if close == "push_finish" and j == len(parts) - 1:
                merged, f32 = acc.push_finish(u, f, want_f32=True)
            elif close == "push_finish" and k == 1:
                acc.push(u[0], f[0])
            else:
                acc.push_many(u, f)
            i += k
        if close == "finish":
            assert acc.count == ACC_M
            merged, f32 = acc.finish(want_f32=True)
        assert acc.count == 0
    assert merged == exp
    assert same_bits(f32, exp32)


@pytest.mark.parametrize("H", ACC_H)
def test_acc_windows(codec, oracle, H):
    """Accumulators over [0, a), [a, b), [b, G): a inside the header run of groups 63 .. 64,
    b behind more headers than the LDS list holds where the layout has them (4096: the
    window's first header index h0 is 1027), else at the layout's last header."""
    lay, ups, d, exp, exp32 = acc_case(oracle, H)
    L, G, hp = len(exp), A.groups_of(lay.n_up), lay.header_positions()
    a, b = A.window_cuts(lay)
    whole_m, whole_v = np.zeros(L + 16, np.uint8), np.zeros(lay.n_up, np.float32)
    for k, (gb, ge) in enumerate(((0, a), (a, b), (b, G))):
        with codec.accumulator(L, hp, gb, ge) as acc:
            if k == 1:
                acc.push(ups[0], d[0])
                acc.push_many(ups[1:3], d[1:3])
                m, v = acc.push_finish(ups[3:], d[3:], want_f32=True)
            else:
                acc.push_many(ups[:2], d[:2])
                for u, f in zip(ups[2:], d[2:]):
                    acc.push(u, f)
                m, v = acc.finish(want_f32=True)
        m = np.frombuffer(m, np.uint8)
        b0, b1 = 16 * gb, min(L, 16 * ge)
        assert not m[:b0].any() and not m[b1:].any()  # only the window is written
        v0, v1 = 3 * gb, min(lay.n_up, 3 * ge)
        assert not v[:v0].any() and not v[v1:].any()
        whole_m[b0:b1] = m[b0:b1]
        whole_v[v0:v1] = v[v0:v1]
    assert whole_m[:L].tobytes() == exp
    assert same_bits(whole_v, exp32)


@pytest.mark.parametrize("H,j", [(1025, 0), (1025, 1024), (4096, 0), (4096, 1024), (4096, 4095)])
def test_acc_refuses_a_later_upload_that_differs(codec, oracle, H, j):
    """A later upload whose header code at index j differs, alone and at every position of
    a burst of three: LayoutError from push, push_many and push_finish, the count as it was,
    and a good retry gives the oracle's bytes over exactly the accepted uploads."""
    lay, ups, d, _, _ = acc_case(oracle, H)
    bad = [A.mismatch_upload(oracle, lay, j, c) for c in range(ACC_M)]
    with codec.accumulator(len(ups[0]), lay.header_positions()) as acc:
        acc.push(ups[0], d[0])

        def refused(call):
            with pytest.raises(F.LayoutError) as ei:
                call()
            assert ei.value.code == F.FLEET_ERR_LAYOUT and acc.count == 1
        refused(lambda: acc.push(bad[1], d[1]))
        for p in range(3):
            burst = [bad[1 + q] if q == p else ups[1 + q] for q in range(3)]
            refused(lambda: acc.push_many(burst, d[1:4]))
            refused(lambda: acc.push_finish(burst, d[1:4]))
        merged, f32 = acc.push_finish(ups[1:4], d[1:4], want_f32=True)
        assert acc.count == 0
    exp = oracle.update_faithful(ups[:4], d[:4])
    assert merged == exp and same_bits(f32, oracle.decode_floats(exp))


def test_acc_rejected_first_burst_does_not_fix_the_header_codes(codec, oracle):
    """Uploads X: the clean ones with another code in header slot 2000 alone (the
    accumulator compares codes at its positions and walks nothing, so the expected bytes
    are the oracle's fused restatement with the header mask). A first burst that mixes
    clean and X is refused whichever comes first; the next first burst, all clean or all
    X, defines the codes and is accepted."""
    lay, ups, d, exp, _ = acc_case(oracle, 4096)
    hp, j = lay.header_positions(), 2000
    assert j >= A.ACC_LDS_HDR
    xs = []
    for c in range(ACC_M):
        v = A.upload_values(oracle, lay, c).copy()
        v[hp[j]] += 1.0
        xs.append(oracle.encode_floats(v))
    exp_x = oracle.update_fused(xs, d, A.header_mask(lay))
    assert exp_x != exp
    with codec.accumulator(len(ups[0]), hp) as acc:
        for first, then, want in (([xs[0], ups[1], ups[2]], ups, exp), ([ups[0], xs[1], ups[2]], xs, exp_x),
                                  ([xs[0], xs[1], ups[2]], ups, exp)):
            with pytest.raises(F.LayoutError):
                acc.push_many(first, d[:3])
            assert acc.count == 0
            with pytest.raises(F.LayoutError):
                acc.push_finish(first, d[:3])
            assert acc.count == 0
            acc.push_many(then[:3], d[:3])
            assert acc.count == 3
            assert acc.push_finish(then[3:], d[3:]) == want


def test_acc_device_forms(codec, oracle):
    """push_many_device, push_finish_device and finish_device on a stream of their own,
    rows pitched wider than the padded upload."""
    lay, ups, d, exp, exp32 = acc_case(oracle, 1025)
    L, G = len(exp), A.groups_of(lay.n_up)
    t = rows_of(ups, pitch=16 * G + 64)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with codec.accumulator(L, lay.header_positions()) as acc:
        merged, f32 = outputs(lay)
        torch.cuda.synchronize()
        acc.push_many_device(t[:3], d[:3], stream=s.cuda_stream)
        assert acc.count == 3
        acc.push_finish_device(t[3:], d[3:], merged, f32, stream=s.cuda_stream)
        assert acc.count == 0
        assert_merged(lay, merged, f32, exp, exp32)
        merged, f32 = outputs(lay)
        torch.cuda.synchronize()
        acc.push_many_device(t, d, stream=s.cuda_stream)
        acc.finish_device(merged, f32, stream=s.cuda_stream)
        assert_merged(lay, merged, f32, exp, exp32)


# 6 ----------------------------------------------------------------------- descent

def special_floats():
    bits = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF8ABCDE, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000],
                    np.uint32)
    return bits.view(np.float32)


def descent_case(oracle, n_seg):
    """Layout, parameters, gradient and the oracle's step. The gradient carries NaNs with
    distinct payloads (quiet and signalling, both signs), both infinities and both zeros
    in the segments of every chunk of kMaxDescentSegs segments, the x86 NaN rule's inputs."""
    lay = A.segments(n_seg)
    segs = A.segment_ranges(lay)
    g = A.upload_values(oracle, lay, 0).copy()
    sp = special_floats()
    special = []  # per chunk, the gradient positions that hold the special values
    for chunk in range(0, n_seg, A.MAX_DESCENT_SEGS):
        slots = [s + e for s, n in segs[chunk: chunk + A.MAX_DESCENT_SEGS] for e in range(n)][: len(sp)]
        g[slots] = sp[: len(slots)]
        special.append(slots)
    n_sw = sum(s > 0 for s in lay.w_sizes)
    pos_w = np.concatenate([np.arange(s, s + n) for s, n in segs[:n_sw]])  # gradient position of each weight
    pos_b = np.concatenate([np.arange(s, s + n) for s, n in segs[n_sw:]])
    assert len(pos_w) == lay.n_weights and len(pos_b) == lay.n_fc_bias
    rng = np.random.default_rng(n_seg)
    w0 = rng.normal(0, 0.05, lay.n_weights).astype(np.float32)
    b0 = rng.normal(0, 0.1, lay.n_fc_bias).astype(np.float32)
    lr = np.float32(0.0173)
    ew, eb = oracle.descent(w0, b0, g, lay.w_present(), lay.fc_flags(), lr)
    nan_at = set(pos_w[np.isnan(ew)].tolist()) | set(pos_b[np.isnan(eb)].tolist())
    assert len(special) == (n_seg + A.MAX_DESCENT_SEGS - 1) // A.MAX_DESCENT_SEGS
    assert all(nan_at & set(slots) for slots in special)  # a NaN step in every chunk
    return lay, segs, g, w0, b0, lr, ew, eb, pos_w, pos_b


@pytest.mark.parametrize("n_seg", A.SEGMENT_COUNTS)
def test_descent_past_one_chunk_of_segments(codec, oracle, n_seg):
    lay, segs, g, w0, b0, lr, ew, eb, _, _ = descent_case(oracle, n_seg)
    assert not same_bits(ew, w0) and not same_bits(eb, b0)
    w, b = codec.descent(w0, b0, g, lay, lr)
    assert same_bits(w, ew) and same_bits(b, eb)
    tw, tb, tg = (torch.from_numpy(x).cuda() for x in (w0, b0, g))
    codec.descent_device(tw, tb, tg, lay, lr)
    torch.cuda.synchronize()
    assert same_bits(tw.cpu().numpy(), ew) and same_bits(tb.cpu().numpy(), eb)


@pytest.mark.parametrize("n_seg", A.SEGMENT_COUNTS)
def test_descent_windows(codec, oracle, n_seg):
    """Cuts on a segment's edge, inside a segment, between segments 64 and 65 (where the
    second k_descent chunk begins), inside a segment of a later chunk, and a last window of
    header slots and a non-fc bias block alone. After each window exactly the parameters
    its positions cover have moved, and after all of them the step is the oracle's."""
    lay, segs, g, w0, b0, lr, ew, eb, pos_w, pos_b = descent_case(oracle, n_seg)
    end = segs[-1][0] + segs[-1][1]
    cuts = [segs[10][0], segs[20][0] + 1]
    assert segs[20][1] >= 2 and end < lay.n_up
    if n_seg > A.MAX_DESCENT_SEGS:
        cuts.append(segs[A.MAX_DESCENT_SEGS][0])  # the 65th segment's first value: the chunk edge
    if n_seg > A.MAX_DESCENT_SEGS + 1:
        k = next(i for i in range(100, n_seg) if segs[i][1] >= 3)
        cuts.append(segs[k][0] + 2)
    runs = [[0] + cuts + [end, lay.n_up]]
    if n_seg > A.MAX_DESCENT_SEGS + 1:
        # one window of more than kMaxDescentSegs segments: it begins inside segment 1 and
        # ends inside a segment of its second chunk, so that chunk's offsets are window-relative
        runs.append([0, segs[1][0] + 1, segs[k][0] + 2, lay.n_up])
        assert segs[1][1] >= 2 and k - 1 > A.MAX_DESCENT_SEGS
    for cuts in runs:
        tw, tb = torch.from_numpy(w0).cuda(), torch.from_numpy(b0).cuda()
        for vb, ve in zip(cuts[:-1], cuts[1:]):
            assert vb < ve
            win = torch.from_numpy(g[vb:ve].copy()).cuda()
            codec.descent_window_device(tw, tb, win, vb, ve, lay, lr)
            torch.cuda.synchronize()
            done_w, done_b = pos_w < ve, pos_b < ve
            assert same_bits(tw.cpu().numpy(), np.where(done_w, ew, w0)), (vb, ve)
            assert same_bits(tb.cpu().numpy(), np.where(done_b, eb, b0)), (vb, ve)
            if vb == end:  # header slots and a non-fc bias block: nothing moves
                assert done_w.all() and done_b.all()
        codec.check()
        assert same_bits(tw.cpu().numpy(), ew) and same_bits(tb.cpu().numpy(), eb)


# 7 ------------------------------------------------------------------ synth_device

def test_synth_device_at_the_cap(codec, oracle):
    """4096 headers: k_synth_headers takes more than one block."""
    lay = A.dense(F.FLEET_MAX_HEADERS)
    M, seed = 3, 991
    hp, hv = np.asarray(lay.header_positions(), np.int32), np.asarray(lay.header_values(), np.float32)
    vals = torch.full((M, lay.n_up + 5), -7.0, dtype=torch.float32, device="cuda")
    codec.synth_device(seed, vals, lay.n_up, hp, hv)
    full = vals.cpu().numpy()
    assert (full[:, lay.n_up:] == -7.0).all()
    for c in range(M):
        want = oracle.synth_upload(seed, c, list(lay.w_sizes), list(lay.b_sizes))
        assert same_bits(full[c, : lay.n_up], want), c
    # a column window, its header positions re-based as the bench's strong-scaling ranks do
    a, b = A.window_cuts(lay)
    for gb, ge in ((a, b), (b, A.groups_of(lay.n_up))):
        v0, v1 = 3 * gb, min(lay.n_up, 3 * ge)
        keep = (hp >= v0) & (hp < v1)
        assert keep.sum() > 256
        win = torch.full((M, v1 - v0 + 2), -7.0, dtype=torch.float32, device="cuda")
        codec.synth_device(seed, win, v1 - v0, hp[keep] - v0, hv[keep], elem0=v0)
        got = win.cpu().numpy()
        assert same_bits(got[:, : v1 - v0], full[:, v0:v1]) and (got[:, v1 - v0:] == -7.0).all()


# 8 ------------------------------------------------------------- the argument contract

def bad_lists(lay):
    """Header lists the entry points refuse: two swapped, one twice, a negative one, one at n."""
    hp = lay.header_positions()
    unsorted = list(hp)
    unsorted[5], unsorted[6] = unsorted[6], unsorted[5]
    dup = list(hp)
    dup[9] = dup[8]
    neg = [-1] + hp[1:]
    at_n = hp[:-1] + [lay.n_up]
    return {"unsorted": unsorted, "duplicate": dup, "negative": neg, "== n": at_n}


@pytest.mark.parametrize("entry", ["update_device", "update_encode_device", "update_kardam_device"])
def test_update_entry_points_refuse_a_bad_header_list(codec, oracle, entry):
    """FLEET_ERR_ARG, nothing written, and the context keeps the good list: the next call
    with it (no re-upload: the list equals the resident one) gives the oracle's bytes.
    Every tensor is a slice one row into its allocation, so nothing a kernel could do
    with the refused lists (positions -1 and n) would leave the test's memory."""
    lay = A.dense(321)
    assert lay.n_up % 3 != 0  # position n is still inside the last group's row bytes
    M = 3
    ups, d = A.uploads(oracle, lay, M), A.dampen(M)
    exp, exp32 = A.expected(oracle, lay, M)
    L, G, hp = len(exp), A.groups_of(lay.n_up), lay.header_positions()
    t = rows_of(ups, lead=1)
    values = torch.zeros((M + 1, 3 * G), dtype=torch.float32, device="cuda")[1:]
    nxt = torch.zeros((M + 1, t.shape[1]), dtype=torch.uint8, device="cuda")[1:]

    def call(positions, merged, f32):
        if entry == "update_device":
            codec.update_device(t, L, d, positions, merged, f32)
        elif entry == "update_encode_device":
            codec.update_encode_device(t, L, d, positions, merged, f32, values, nxt)
        else:
            codec.update_kardam_device(t, L, d, positions, 0.05, merged, f32)
        codec.check()

    merged, f32 = outputs(lay, lead=1)
    call(hp, merged, f32)
    assert_merged(lay, merged, f32, exp, exp32)
    for what, positions in bad_lists(lay).items():
        merged, f32 = outputs(lay, lead=1)
        with pytest.raises(F.FleetError) as ei:
            call(positions, merged, f32)
        assert ei.value.code == F.FLEET_ERR_ARG, what
        assert "ascending" in str(ei.value), what
        torch.cuda.synchronize()
        assert (merged == FILL).all() and (f32 == -7.0).all(), what  # nothing launched
        call(hp, merged, f32)
        assert_merged(lay, merged, f32, exp, exp32)


def test_synth_device_refuses_positions_outside_its_columns(codec, oracle):
    """Position n_up with vpitch > n_up and position -1 against a tensor that begins one
    row into its allocation: FLEET_ERR_ARG and no store. NULL lists with n_headers > 0
    likewise."""
    lay = A.dense(257)
    M = 2
    hp, hv = lay.header_positions(), lay.header_values()
    alloc = torch.full((M + 1, lay.n_up + 4), -7.0, dtype=torch.float32, device="cuda")
    vals = alloc[1:]
    for positions in (hp[:-1] + [lay.n_up], [-1] + hp[1:]):
        with pytest.raises(F.FleetError) as ei:
            codec.synth_device(3, vals, lay.n_up, positions, hv)
        assert ei.value.code == F.FLEET_ERR_ARG and "outside" in str(ei.value)
    fn = F.lib().fleet_synth_window_device
    p = np.asarray(hp, np.int32)
    v = np.asarray(hv, np.float32)
    for pos_arg, val_arg in ((None, v.ctypes.data), (p.ctypes.data, None), (None, None)):
        rc = fn(codec._h, 3, M, 0, 0, pos_arg, val_arg, len(hp), lay.n_up, vals.data_ptr(), vals.shape[1], None)
        assert rc == F.FLEET_ERR_ARG
    torch.cuda.synchronize()
    assert (alloc == -7.0).all()
    codec.synth_device(3, vals, lay.n_up, hp, hv)  # the good list still works
    got = vals.cpu().numpy()
    assert same_bits(got[0, : lay.n_up], oracle.synth_upload(3, 0, list(lay.w_sizes), list(lay.b_sizes)))
    assert (alloc[0] == -7.0).all() and (got[:, lay.n_up:] == -7.0).all()


def test_accumulator_refuses_a_bad_header_list(codec, oracle):
    lay = A.dense(321)
    for what, positions in bad_lists(lay).items():
        with pytest.raises(F.FleetError) as ei:
            codec.accumulator(A.b64_len(lay.n_up), positions)
        assert ei.value.code == F.FLEET_ERR_ARG and "ascending" in str(ei.value), what
