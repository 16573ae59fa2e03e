"""Shared inputs of the layout-axis tests (test_gpu_layout_axis.py on the GPU,
test_layout_axis_inputs.py on the CPU): header-dense layouts at the header counts where the
kernels take another path, layouts with a stated number of descent segments, their uploads
and, per layout and header index, a twin layout of the same length whose header code
there differs. A plain module: it holds no test.

The other axes (clients, values, plans, the tail past the walk) have modules of their own;
here only the layout moves. An upload of dense(H) holds about 2.2 values per header: 9,000
values at the cap of 4096 headers, so every case stays small."""
import functools

import numpy as np

from fleet_amd.layouts import Layout

# Block sizes in turn: runs of zero-size blocks (2, 3 and 4 header slots in a row), single
# values between two headers, payload runs of 2, 3 and 5. 12 blocks hold 14 values, 26
# slots, and 26 is prime to 3, so the pattern meets a group at every phase.
PATTERN = (0, 0, 0, 1, 2, 0, 3, 1, 0, 0, 5, 2)

# The constants the edges below stand on, as read today (test_layout_axis_inputs.py parses
# them from the sources and fails when one moves without its edge).
FLEET_MAX_HEADERS = 4096  # include/fleet_codec.h: the cap of every header list
# tile_init (kernels.hip) strides the header list by the block's 64 * NW threads: its
# second iteration runs from 64 * NW headers on
NW_TILED = 4    # TileShared<TG, 4, D16> / TileShared<kFlatTG, 4, true>: the classic and flat tiles
NW_PIPE = 5     # k_update_pipe<16, 1, 5, 0>: the pipelined tiles
NW_WEAVE = (6, 8)  # k_update_weave<6 | 8>
NW_PIPE_KD = 9  # FLEET_KD_NW: the pipelined tiles with Kardam's side outputs
TILE_NW = (NW_TILED, NW_PIPE) + NW_WEAVE + (NW_PIPE_KD,)
ACC_LDS_HDR = 1024      # kAccLdsHdr (acc_kernels.hip): longer lists are searched in global memory
MAX_DESCENT_SEGS = 64   # kMaxDescentSegs (kernels.h): segments per k_descent launch

CONTROL = 17  # CIFAR's count, the most the suite had
# 64 * NW - 1, 64 * NW, 64 * NW + 1 per tile form; 2 * 64 * NW_PIPE_KD + 1 = a third
# iteration of the widest block; kAccLdsHdr - 1, kAccLdsHdr, kAccLdsHdr + 1; the cap - 1, the cap
EDGES = sorted({CONTROL} | {64 * nw + k for nw in TILE_NW for k in (-1, 0, 1)} | {2 * 64 * NW_PIPE_KD + 1} |
               {ACC_LDS_HDR - 1, ACC_LDS_HDR, ACC_LDS_HDR + 1} | {FLEET_MAX_HEADERS - 1, FLEET_MAX_HEADERS})
SEGMENT_COUNTS = (MAX_DESCENT_SEGS, MAX_DESCENT_SEGS + 1, 2 * MAX_DESCENT_SEGS + 1)

# Header runs placed on purpose (first slot, length): slots 47 | 48 lie either side of
# group 16 (a pipelined tile's edge), 189..194 are groups 63 and 64 (three headers each, in a
# wave's and tile's last group and in the next one's first) and 195 follows, 767 | 768 lie
# either side of group 256 (an acc block's edge). A layout that would end before slot 768
# gets one longer payload block.
RUNS = ((47, 2), (189, 7), (767, 2))
REACH = 790  # slots a dense layout of at least 257 headers has at the least


def groups_of(n_up):
    return (n_up + 2) // 3


def b64_len(n_values):
    return 4 * ((4 * n_values + 2) // 3)


def _dense_sizes(n_headers, seed, pad, runs):
    """Sizes of the n_headers - 2 blocks in upload order, and the number of weight blocks."""
    n_blocks = n_headers - 2
    n_w = (n_blocks + 1) // 2
    sizes, pos, zeros, k = [], 1, 0, seed
    for b in range(n_blocks):
        if b == n_w:
            pos += 1  # the bias count's slot
        # a run of r header slots from t: the block before it ends at t - 1, r - 1 empty blocks follow
        here = [r for t, r in runs if pos == t]
        ahead = [(t, r) for t, r in runs if 0 <= t - pos - 1 <= 5]
        if zeros:
            s, zeros = 0, zeros - 1
        elif here:
            s, zeros = 0, here[0] - 2
        elif ahead:
            s, zeros = ahead[0][0] - pos - 1, ahead[0][1] - 1
        elif b < 3:
            s = 0  # group 0: the weight count and two empty blocks, three header slots
        elif pad and pos > 200:
            s, pad = pad, 0
        else:
            s = PATTERN[k % len(PATTERN)]
            k += 1
        sizes.append(s)
        pos += 1 + s
    return sizes, n_w


@functools.lru_cache(maxsize=None)
def dense(n_headers, seed=0, extra_run=None):
    """A layout of exactly n_headers header slots, 2 + len(w_sizes) + len(b_sizes); the
    seed turns the size pattern, extra_run is the first slot of one more run of ten
    header slots. Every second bias layer with values counts as fully connected."""
    assert n_headers >= 5
    runs = RUNS if extra_run is None else tuple(sorted(RUNS + ((extra_run, 10),)))
    sizes, n_w = _dense_sizes(n_headers, seed, 0, runs)
    short = REACH - (n_headers + sum(sizes))
    if n_headers >= 257 and short > 0:
        sizes, n_w = _dense_sizes(n_headers, seed, short, runs)
    w, b = tuple(sizes[:n_w]), tuple(sizes[n_w:])
    return Layout(f"dense{n_headers}s{seed}", w, b, tuple(k for k, s in enumerate(b) if s > 0 and k % 2 == 0))


@functools.lru_cache(maxsize=None)
def segments(n_seg):
    """A layout with exactly n_seg descent segments (present, non-empty weight blocks and
    non-empty fully-connected bias blocks), zero-size blocks and non-fc bias blocks in
    between, so a segment's index is not its block's."""
    n_sw = (2 * n_seg) // 3
    w_pat, b_pat = (3, 0, 5, 2, 0, 0, 1, 7), (4, 2, 0, 6, 3, 0, 1)
    w, b, fc = [], [], []
    while sum(s > 0 for s in w) < n_sw:
        w.append(w_pat[len(w) % len(w_pat)])
    w.append(0)
    while len([k for k in fc if b[k] > 0]) < n_seg - n_sw:
        k = len(b)
        b.append(b_pat[k % len(b_pat)])
        if k % 3 != 1:  # every third bias layer is not fully connected
            fc.append(k)
    b.append(5)  # a last non-fc bias block: slots no window's step touches
    return Layout(f"segments{n_seg}", tuple(w), tuple(b), tuple(fc))


@functools.lru_cache(maxsize=None)
def dense_cut_for(n_headers, world=3):
    """dense(n_headers) with one more header run, placed so that the balanced split of its
    groups over `world` contexts (fleet_amd.shard.group_range, fleet_update_multi) begins
    context 1's window between two three-header groups."""
    g1 = groups_of(dense(n_headers).n_up) // world
    for t in range(3 * (g1 - 16), 3 * (g1 + 4), 3):
        lay = dense(n_headers, 0, t)
        G = groups_of(lay.n_up)
        cut = G // world + min(1, G % world)
        bits = header_bits(lay)
        if bits[cut - 1] == 7 and bits[cut] == 7:
            return lay, cut
    raise AssertionError(f"no run on the cut of dense({n_headers}) over {world}")


def segment_ranges(lay):
    """[(first value position, length)] of the layout's descent segments, in order."""
    out, idx = [], 1
    for s in lay.w_sizes:
        idx += 1
        if s > 0:
            out.append((idx, s))
        idx += s
    idx += 1
    for k, s in enumerate(lay.b_sizes):
        idx += 1
        if s > 0 and k in lay.fc_layers:
            out.append((idx, s))
        idx += s
    assert idx == lay.n_up
    return out


def header_bits(lay):
    """Per 3-value group the mask of its header slots (bit e = slot 3 g + e)."""
    bits = np.zeros(groups_of(lay.n_up), np.uint8)
    for p in lay.header_positions():
        bits[p // 3] |= 1 << (p % 3)
    return bits


def header_mask(lay):
    m = np.zeros(lay.n_up, np.uint8)
    m[lay.header_positions()] = 1
    return m


def mismatch(lay, j):
    """A twin layout of the same length whose header code at the clean layout's j-th header
    slot differs: one unit moved to block j's size from the nearest non-empty block of its
    section (the walk stays consistent, so the twin parses as a layout); for the two count
    slots the first bias block becomes the last weight block."""
    w, b = list(lay.w_sizes), list(lay.b_sizes)
    n_w = len(w)
    if j in (0, n_w + 1):
        assert b
        w.append(b.pop(0))
    else:
        sec, k = (w, j - 1) if j <= n_w else (b, j - n_w - 2)
        donors = sorted((m for m in range(len(sec)) if m != k and sec[m] > 0), key=lambda m: (abs(m - k), m < k))
        sec[k] += 1
        sec[donors[0]] -= 1
    twin = Layout(f"{lay.name}x{j}", tuple(w), tuple(b))
    assert twin.n_up == lay.n_up
    return twin


SEED = 7311
_values, _uploads, _expected = {}, {}, {}


def upload_values(oracle, lay, c, seed=SEED):
    key = (lay, c, seed)
    if key not in _values:
        _values[key] = oracle.synth_upload(seed, c, list(lay.w_sizes), list(lay.b_sizes))
    return _values[key]


def uploads(oracle, lay, M, seed=SEED):
    """Clients 0 .. M - 1 of the layout: oracle.encode_floats of oracle.synth_upload."""
    out = []
    for c in range(M):
        key = (lay, c, seed)
        if key not in _uploads:
            _uploads[key] = oracle.encode_floats(upload_values(oracle, lay, c, seed))
        out.append(_uploads[key])
    return out


def mismatch_upload(oracle, lay, j, c, seed=SEED):
    """Client c's upload under mismatch(lay, j)."""
    return uploads(oracle, mismatch(lay, j), c + 1, seed)[c]


# three distinct factors, 1 / 3 no binary32 value (scalarMultiply's f64 branch)
DAMPEN3 = (1.0, 1.0 / 3.0, 0.25)


def dampen(M):
    return [DAMPEN3[c % 3] / (1 + c // 3) for c in range(M)]


def expected(oracle, lay, M, d=None, seed=SEED):
    """(merged bytes, merged_f32) of the oracle's faithful per-op chain, computed once."""
    d = tuple(dampen(M) if d is None else d)
    key = (lay, M, d, seed)
    if key not in _expected:
        exp = oracle.update_faithful(uploads(oracle, lay, M, seed), list(d))
        _expected[key] = (exp, oracle.decode_floats(exp))
    return _expected[key]


def three_header_groups(lay):
    return [int(g) for g in np.flatnonzero(header_bits(lay) == 7)]


def headers_before(lay, group):
    """Headers at positions below 3 * group (the index a window's search starts from)."""
    return int(np.searchsorted(np.asarray(lay.header_positions()), 3 * group))


def window_cuts(lay):
    """(a, b) of the windows [0, a), [a, b), [b, G): a between two three-header groups in a
    row (RUNS: groups 63 | 64, so the first window ends and the second begins inside the
    run); b the first group with more than kAccLdsHdr headers before it, else the group
    of the last header."""
    G = groups_of(lay.n_up)
    three = three_header_groups(lay)
    a = [g for g in three if g + 1 in three and g > 1][0] + 1
    hp = lay.header_positions()
    b = hp[ACC_LDS_HDR] // 3 + 1 if len(hp) > ACC_LDS_HDR + 1 else hp[-1] // 3
    assert 0 < a < b < G
    return a, b
