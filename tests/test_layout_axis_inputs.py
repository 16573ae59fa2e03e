"""The inputs of test_gpu_layout_axis.py, validated without a GPU: the header-count edges
follow the constants in the sources, every dense layout has the header count it claims and
keeps the group patterns and header runs the GPU tests lean on, the segment family has its
stated segment counts, the mismatch twins differ where intended, the header values survive
the codec, and the oracle (no header cap of its own) is self-consistent on all of it:
its faithful per-op chain equals its fused restatement. fleet_layout_from_sizes is host
code and is held to the cap here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fleet_amd as F
import layout_axis as A

CSRC = os.path.join(F.ROOT, "fleet_amd", "csrc")
BIG = [h for h in A.EDGES if h >= 257]


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _one(pattern, text):
    found = set(re.findall(pattern, text))
    assert len(found) == 1, (pattern, found)
    return found.pop()


def test_edges_follow_the_constants_in_the_sources():
    k = _src("kernels.hip")
    # tile_init strides by the block's threads, 64 * NW with NW the tile's second parameter
    assert "for (int i = tid; i < n_hdr; i += 64 * NW)" in k and "if (i != tid) hp = hdr[i];" in k
    assert int(_one(r"__shared__ TileShared<TG, (\d+), true> sh;", k)) == A.NW_TILED
    assert int(_one(r"__shared__ TileShared<kFlatTG, (\d+), true> sh;", k)) == A.NW_TILED
    assert "__shared__ TileShared<TG, NW, (bool)FLEET_PIPE_D16> sh;" in k
    # the launchers take the block from the plan (launch_plan.cpp), both from launch_plan.h's constants
    lp, lc = _src("launch_plan.h"), _src("launch_plan.cpp")
    assert int(_one(r"constexpr int kPipeNW = (\d+);", lp)) == A.NW_PIPE
    assert "FLEET_LAUNCH((k_update_pipe<16, 1, kPipeNW, 0>), INT32_MAX" in k and "p->threads = 64 * kPipeNW;" in lc
    assert "dim3(p.threads), 0, s, FLEET_UPDATE_ARGS" in k
    a, b, c = _one(r"if \(p\.nw == (\d+)\) FLEET_LAUNCH\(k_update_weave<(\d+)>\);\s*"
                   r"else FLEET_LAUNCH\(k_update_weave<(\d+)>\);", k)
    assert (int(a), int(c)) == (int(b), int(c)) == A.NW_WEAVE and "p->threads = 64 * p->nw;" in lc
    assert int(_one(r"#define FLEET_KD_NW (\d+)", lp)) == A.NW_PIPE_KD and "kKdPipeNW = FLEET_KD_NW" in lp
    assert "FLEET_LAUNCH((k_update_pipe<16, 1, kKdPipeNW, 0, true>)" in k and "p.threads = 64 * kKdPipeNW;" in lc
    assert int(_one(r"constexpr int kAccLdsHdr = (\d+);", _src("acc_kernels.hip"))) == A.ACC_LDS_HDR
    h = _src("kernels.h")
    assert int(_one(r"constexpr int kMaxDescentSegs = (\d+);", h)) == A.MAX_DESCENT_SEGS
    assert int(_one(r"constexpr int kMaxHeaderSlots = (\d+);", h)) == F.FLEET_MAX_HEADERS == A.FLEET_MAX_HEADERS
    assert int(_one(r"#define FLEET_MAX_HEADERS (\d+)", open(F.HEADER_PATH).read())) == F.FLEET_MAX_HEADERS
    assert "segs->back().n == fleet::kMaxDescentSegs" in _src("fleet_codec.cpp")
    want = {17, 1023, 1024, 1025, 4095, 4096, 2 * 576 + 1}
    for nw in (4, 5, 6, 8, 9):
        want |= {64 * nw - 1, 64 * nw, 64 * nw + 1}
    assert set(A.EDGES) == want  # the values as read today
    assert A.SEGMENT_COUNTS == (64, 65, 129)


@pytest.mark.parametrize("H", A.EDGES + [4097, 6000])
def test_dense_layouts_have_the_header_count_they_claim(oracle, H):
    lay = A.dense(H)
    assert 2 + len(lay.w_sizes) + len(lay.b_sizes) == H
    hp = lay.header_positions()
    assert len(hp) == H == len(set(hp)) and hp == sorted(hp) and hp[-1] < lay.n_up
    hm = oracle.header_mask(list(lay.w_sizes), list(lay.b_sizes))  # the oracle has no header cap
    assert len(hm) == lay.n_up and list(np.flatnonzero(hm)) == hp
    assert np.array_equal(hm, A.header_mask(lay))
    sizes = lay.w_sizes + lay.b_sizes
    small = sum(s in (0, 1, 2, 3, 5) for s in sizes)
    assert small >= len(sizes) - 8  # the runs' lead-in blocks and one longer block in the short layouts
    if H >= 400:
        assert 2.0 < lay.n_up / H < 2.3 and max(sizes) <= 5
    assert lay.n_up <= 13_500
    assert lay.fc_layers and all(lay.b_sizes[k] > 0 for k in lay.fc_layers)
    assert A.dense(H, seed=5) != lay and len(A.dense(H, seed=5).header_positions()) == H


@pytest.mark.parametrize("H", BIG)
def test_dense_layouts_keep_the_group_patterns_and_runs(H):
    lay = A.dense(H)
    bits = A.header_bits(lay)
    assert set(bits.tolist()) == set(range(8))  # each header-bit pattern of a 3-value group
    three = A.three_header_groups(lay)
    assert any(g % 64 == 0 for g in three) and any(g % 64 == 63 for g in three)
    assert 0 in three and 63 in three and 64 in three  # group 0; a tile's last group and the next one's first
    hs = set(lay.header_positions())
    G = A.groups_of(lay.n_up)
    assert G > 256
    for m in (16, 64, 256):  # the pipe tile, the tile / wave, the acc kernels' block
        spans = [B for B in range(m, G, m) if 3 * B - 1 in hs and 3 * B in hs]
        assert spans, (H, m)
    assert any(B % 64 for B in range(16, G, 16) if 3 * B - 1 in hs and 3 * B in hs)  # a 16-group edge that is no 64-group edge
    assert any(bits[g] and bits[g + 1] and bits[g + 2] for g in range(0, G - 2))


def test_ragged_ends():
    """A last group of one value that is a header slot, and a last group of two values."""
    one = [h for h in A.EDGES if A.dense(h).n_up % 3 == 1 and A.dense(h).b_sizes[-1] == 0]
    two = [h for h in A.EDGES if A.dense(h).n_up % 3 == 2]
    assert one and two
    assert any(h >= 257 for h in one) and any(h > A.ACC_LDS_HDR for h in one + two)
    for h in one:
        lay = A.dense(h)
        assert lay.header_positions()[-1] == lay.n_up - 1 and A.header_bits(lay)[-1] == 1


@pytest.mark.parametrize("H", BIG)
def test_window_cuts(H):
    lay = A.dense(H)
    a, b = A.window_cuts(lay)
    bits = A.header_bits(lay)
    assert bits[a - 1] == 7 and bits[a] == 7  # [0, a) ends and [a, b) begins inside a run of three-header groups
    before = A.headers_before(lay, b)
    if H > A.ACC_LDS_HDR + 1:
        assert before > A.ACC_LDS_HDR and before < H  # the last window's first header index is past the LDS list's size
    else:
        assert H - 4 <= before < H  # the last window holds the last few headers only
    assert a == 64 and A.headers_before(lay, a) > 64  # a wave's worth of headers before the second window


@pytest.mark.parametrize("H", [65, 257, 1023, 1024, 1025, 4096, 4097, 6000])
def test_header_values_round_trip_and_the_oracle_is_self_consistent(oracle, H):
    lay = A.dense(H)
    hv = np.asarray(lay.header_values(), np.float32)
    assert np.array_equal(oracle.decode_floats(oracle.encode_floats(hv)), hv)
    M = 3
    ups, d = A.uploads(oracle, lay, M), A.dampen(M)
    assert len({len(u) for u in ups}) == 1 and len(ups[0]) == A.b64_len(lay.n_up) and len(set(ups)) == M
    v = np.stack([A.upload_values(oracle, lay, c) for c in range(M)])
    assert np.array_equal(v[:, lay.header_positions()], np.tile(hv, (M, 1)))
    exp, f32 = A.expected(oracle, lay, M)
    assert exp == oracle.update_fused(ups, d, A.header_mask(lay))
    assert len(f32) == lay.n_up
    flat = oracle.flat_gradient(ups[0])
    assert len(oracle.decode_floats(flat)) == lay.n_flat  # the walk skipped exactly the header slots
    back = oracle.decode_floats(oracle.merge_flat_gradient(ups[1], flat))
    assert len(back) == lay.n_up and np.array_equal(back[lay.header_positions()], hv)
    assert len(set(A.dampen(3))) == 3 and float(np.float32(A.dampen(3)[1])) != A.dampen(3)[1]


@pytest.mark.parametrize("H", [h for h in A.EDGES if h not in (65, 257, 1023, 1024, 1025, 4096)])
def test_every_edge_is_self_consistent(oracle, H):
    lay = A.dense(H)
    hv = np.asarray(lay.header_values(), np.float32)
    assert np.array_equal(oracle.decode_floats(oracle.encode_floats(hv)), hv)
    exp, _ = A.expected(oracle, lay, 3)
    assert exp == oracle.update_fused(A.uploads(oracle, lay, 3), A.dampen(3), A.header_mask(lay))


def test_wrapping_client_count_is_self_consistent(oracle):
    lay = A.dense(1025)
    exp, _ = A.expected(oracle, lay, 70)
    assert exp == oracle.update_fused(A.uploads(oracle, lay, 70), A.dampen(70), A.header_mask(lay))


@pytest.mark.parametrize("n_seg", A.SEGMENT_COUNTS)
def test_segment_family(oracle, n_seg):
    lay = A.segments(n_seg)
    segs = A.segment_ranges(lay)
    assert len(segs) == n_seg
    assert sum(s > 0 for s in lay.w_sizes) + sum(lay.b_sizes[k] > 0 for k in lay.fc_layers) == n_seg
    assert sum(n for _, n in segs) == lay.n_weights + lay.n_fc_bias
    assert 0 in lay.w_sizes and 0 in lay.b_sizes  # blocks that are no segment, in between
    non_fc = [k for k in range(len(lay.b_sizes)) if k not in lay.fc_layers]
    assert any(lay.b_sizes[k] > 0 and 0 < k < len(lay.b_sizes) - 1 for k in non_fc)
    assert len(lay.w_sizes) + len(lay.b_sizes) > n_seg + 10  # a segment's index is not its block's
    assert any(n >= 3 for _, n in segs[A.MAX_DESCENT_SEGS:]) or n_seg == A.MAX_DESCENT_SEGS
    hv = np.asarray(lay.header_values(), np.float32)
    assert np.array_equal(oracle.decode_floats(oracle.encode_floats(hv)), hv)
    # the oracle's step moves exactly the segments' parameters
    g = A.upload_values(oracle, lay, 0)
    w0, b0 = np.ones(lay.n_weights, np.float32), np.ones(lay.n_fc_bias, np.float32)
    w1, b1 = oracle.descent(w0, b0, g, lay.w_present(), lay.fc_flags(), 0.5)
    assert len(w1) == lay.n_weights and len(b1) == lay.n_fc_bias


@pytest.mark.parametrize("H", [257, 321, 577, 1025, 4096])
def test_mismatch_twins_differ_at_the_stated_header(oracle, H):
    lay = A.dense(H)
    hp = lay.header_positions()
    good = oracle.decode_ints(A.uploads(oracle, lay, 1)[0])
    js = {0, 1, H - 1, len(lay.w_sizes) + 1} | {64 * nw for nw in A.TILE_NW if 64 * nw < H} | (
        {A.ACC_LDS_HDR} if H > A.ACC_LDS_HDR else set())
    for j in sorted(js):
        twin = A.mismatch(lay, j)
        assert twin.n_up == lay.n_up and twin != lay
        bad = A.mismatch_upload(oracle, lay, j, 0)
        assert len(bad) == A.b64_len(lay.n_up)
        codes = oracle.decode_ints(bad)
        assert codes[hp[j]] != good[hp[j]], (H, j)
        # the twin is a layout of its own: the reference's walk accepts it
        assert len(oracle.decode_floats(oracle.flat_gradient(bad))) == twin.n_flat
        if j not in (0, len(lay.w_sizes) + 1):
            differ = [i for i in range(H) if codes[hp[i]] != good[hp[i]]]
            assert j in differ and max(abs(i - j) for i in differ) <= 8  # the nearest non-empty block is close


def _from_sizes(lay, cap, with_pos=True):
    w = np.ascontiguousarray(lay.w_sizes, np.int32)
    b = np.ascontiguousarray(lay.b_sizes, np.int32)
    pos = np.full(max(cap, 1) + 2, -7, np.int32)
    nh, n_up = C.c_int(-1), C.c_size_t(0)
    rc = F.lib().fleet_layout_from_sizes(w.ctypes.data, len(w), b.ctypes.data, len(b),
                                         pos.ctypes.data if with_pos else None, cap, C.byref(nh), C.byref(n_up))
    return rc, nh.value, n_up.value, pos


def test_layout_from_sizes_at_the_cap():
    cap = F.FLEET_MAX_HEADERS
    lay = A.dense(cap)
    rc, nh, n_up, pos = _from_sizes(lay, cap)
    assert (rc, nh, n_up) == (F.FLEET_OK, cap, lay.n_up)
    assert pos[:cap].tolist() == lay.header_positions() and pos[cap:].tolist() == [-7, -7]
    over = A.dense(cap + 1)
    rc, nh, n_up, pos = _from_sizes(over, cap)
    assert (rc, nh, n_up) == (F.FLEET_ERR_CAPACITY, cap + 1, over.n_up)  # refused, count and length still reported
    assert pos[:cap].tolist() == over.header_positions()[:cap] and pos[cap:].tolist() == [-7, -7]
    rc, nh, n_up, pos = _from_sizes(lay, cap - 1)
    assert (rc, nh, n_up) == (F.FLEET_ERR_CAPACITY, cap, lay.n_up)
    assert pos[:cap - 1].tolist() == lay.header_positions()[:cap - 1] and pos[cap - 1:].tolist() == [-7, -7, -7][:len(pos) - cap + 1]
    # header_pos == NULL: it only counts
    assert _from_sizes(lay, cap, with_pos=False)[:3] == (F.FLEET_OK, cap, lay.n_up)
    assert _from_sizes(over, cap, with_pos=False)[:3] == (F.FLEET_ERR_CAPACITY, cap + 1, over.n_up)
    assert _from_sizes(over, 0, with_pos=False)[:3] == (F.FLEET_ERR_CAPACITY, cap + 1, over.n_up)
