"""Shared inputs of the client-axis tests (test_gpu_client_axis.py on the GPU,
test_client_axis_inputs.py on the CPU): the two small layouts, the uploads per (layout,
mix, client), the launch plans with the kernel each must name and the client counts that
sit on its chunk and ring edges, the corrupt uploads of the rejection tests and the
sizes that pin k_kardam_reduce's instantiations. A plain module: it holds no test.

Every form but the stream kernel walks the clients in chunks; the M lists below follow
the chunk size c and ring depth r of each form (kernels.hip), as
{1, c-1, c, c+1, 2c, 2c+1, r*c, r*c+1, (r+1)*c+1, one value >= 2*r*c+1}. A change of one
of the named constants moves the edges: the lists then have to follow."""
import numpy as np

from fleet_amd.layouts import Layout, synthetic
from test_gpu_fuzz import DAMPEN, FUSED_PLANS, PLANS, _payload

# synthetic(50): 17 groups -- two 16-group pipelined tiles (the second one group), one
# ragged 64-group tile, a last group of 2 values (the second one the trailing header 0).
# hdrs: 193 values, 65 groups -- two 64-group tiles (the second one group), five 16-group
# tiles, a last group of 1 value, zero-size blocks, header slots 0, 1, 62, 63, 134, 135,
# 166, 167 (groups 0, 20, 21, 44, 45, 55: four 16-group tiles, one 64-group tile).
LAYOUTS = {"syn50": synthetic(50), "hdrs": Layout("hdrs", (60, 0, 70), (30, 0, 25))}
# an upload of the same length whose header slots hold other codes (the layout check)
MISMATCH = {"syn50": Layout("syn50x", (20, 26), ()), "hdrs": Layout("hdrsx", (61, 0, 69), (30, 0, 25))}
MIXES = (0, 1, 2)  # test_gpu_fuzz._payload: gradient-like, wide magnitudes, edge values sprinkled in
SEED = 4242

# k_update_pipe<16, 1, 5, 0>: CPP = 4 producer waves * 64 / TG 16 = 16 clients per pass,
# RING = FLEET_PIPE_RING 3072 floats / (E 48 * CPP 16) = 4 passes: the ring wraps for M > 64
M_PIPE = [1, 15, 16, 17, 32, 33, 64, 65, 81, 129]
# k_update_pipe<16, 1, 9, 0, true> (FLEET_KD_NW 9): CPP = 8 * 64 / 16 = 32, RING =
# FLEET_KD_RING 3072 / (48 * 32) = 2 passes: wraps for M > 64
M_PIPE_KD = [1, 31, 32, 33, 64, 65, 97, 130]
# k_update_tiled_encode<64>: tiled_chunk_clients<64, true> = FLEET_TILED_PT_D16 / (3 * 64) = 8
M_CLASSIC = [7, 8, 9, 17, 65, 129]
# update_flat_block: kFlatPass 512 / W clients per pass (W = 16 / 32: 4 / 2 clients in one wave)
M_FLAT = {16: [31, 32, 33, 65, 129], 32: [15, 16, 17, 33, 129], 64: [7, 8, 9, 17, 129]}
# update_weave_block: chunks of NW clients; one chunk, the first consumed chunk (FIRST),
# later chunks, the short last chunk
M_WEAVE = {6: [1, 5, 6, 7, 12, 13, 19, 129], 8: [1, 7, 8, 9, 16, 17, 25, 129]}
# update_lane: two clients per trip and an odd tail (Kardam: one per trip, the even
# client's norm sums held); ladder rungs at M / 4 .. (all 0 for M < 4)
M_STREAM = [1, 2, 3, 4, 5, 8, 9, 65]

_PIPE, _MIXED = "k_update_pipe<16, 1, 5, 0, false>", "k_update_mixed<256, false>"
# plan -> (kernel fleet_update_kernel must name, flat tile width or None, M list). Both
# layouts are far below one round of tiles, so tile=flat alone plans its narrowest width.
UPDATE_FORMS = {
    "": (_PIPE, None, M_PIPE),
    "update=pipe": (_PIPE, None, M_PIPE),
    "update=stream": (_MIXED, None, M_STREAM),
    "update=stream,grid=plain": (_MIXED, None, M_STREAM),
    "update=stream,grid=lanes": (_MIXED, None, M_STREAM),
    "update=tiled,tile=classic": ("k_update_tiled_encode<64>", None, M_CLASSIC),
    "update=tiled,tile=flat": ("k_update_flat", 16, M_FLAT[16]),
    "update=tiled,tile=flat,flat_w2=16": ("k_update_flat", 16, M_FLAT[16]),
    "update=tiled,tile=flat,flat_w2=32": ("k_update_flat", 32, M_FLAT[32]),
    "update=tiled,tile=flat,flat_w2=64": ("k_update_flat", 64, M_FLAT[64]),
    "update=tiled,tile=weave6": ("k_update_weave<6>", None, M_WEAVE[6]),
    "update=tiled,tile=weave8": ("k_update_weave<8>", None, M_WEAVE[8]),
}
assert set(PLANS) <= set(UPDATE_FORMS)  # every plan of the fuzz has its M list here

# launch_update_encode: rpb = min(M, tile_enc_rows or 24) rows per encode block, so a
# second, ragged row-block from M = 25 (tile_enc_rows=5: from 6; the pipelined form: one
# row per block at these sizes); 65 and 81 wrap the pipelined ring
M_FUSED = [11, 23, 24, 25, 49, 65, 81]
_PIPE_ENC = _PIPE + " (with the encode's blocks)"
# plan -> kernel fleet_update_encode_kernel must name
FUSED_FORMS = {
    "": _PIPE_ENC,
    "update=pipe": _PIPE_ENC,
    "update=stream": "k_update_encode<256>",
    "update=stream,grid=lanes": "k_update_encode<256>",
    "update=tiled": "k_update_flat",  # below 65,536 groups the fused step's tiles are the flat ones
    "update=tiled,tile=flat": "k_update_flat",
    "update=tiled,tile=flat,flat_w2=16": "k_update_flat",
    "update=tiled,tile=classic": "k_update_tiled_encode<64>",
    "update=tiled,tile=weave6": "k_update_weave_encode<6>",
    "update=tiled,tile=weave8": "k_update_weave_encode<8>",
    "update=tiled,tile=flat,tile_enc_rows=5": "k_update_flat",
    "update=stream,tile_enc_rows=5": "k_update_encode<256>",
}
assert set(FUSED_PLANS) <= set(FUSED_FORMS)


def kardam_m_list(spec):
    """The M list of a plan's Kardam form (launch_update_kardam: the pipelined tiles, the
    flat tiles at a forced width 16 / 32 / 64 -- any other tile choice keeps the planned
    width, 16 at these sizes -- or the stream kernel)."""
    if "update=pipe" in spec:
        return M_PIPE_KD
    if "update=stream" in spec:
        return M_STREAM
    for w in (32, 64):
        if f"flat_w2={w}" in spec:
            return M_FLAT[w]
    return M_FLAT[16]


def groups_of(n_up):
    return (n_up + 2) // 3


def b64_len(n_values):
    return 4 * ((4 * n_values + 2) // 3)


def payload_mask(lay):
    m = np.ones(lay.n_up, bool)
    m[lay.header_positions()] = False
    return m


_values, _uploads = {}, {}


def upload_values(oracle, name, mix, c, seed=SEED):
    """Client c's upload of layout `name` as floats: the oracle's synthetic upload with the
    payload mix written over the non-header slots (the same for every M: the uploads of a
    smaller client count are a prefix of a larger one's)."""
    key = (name, mix, c, seed)
    if key not in _values:
        lay = LAYOUTS[name]
        v = oracle.synth_upload(seed + mix, c, list(lay.w_sizes), list(lay.b_sizes))
        p = _payload(np.random.default_rng([seed, sorted(LAYOUTS).index(name), mix, c]), mix, lay.n_flat)
        if p is not None:
            v[payload_mask(lay)] = p
        _values[key] = v
    return _values[key]


def uploads(oracle, name, mix, M, seed=SEED):
    out = []
    for c in range(M):
        key = (name, mix, c, seed)
        if key not in _uploads:
            _uploads[key] = oracle.encode_floats(upload_values(oracle, name, mix, c, seed))
        out.append(_uploads[key])
    return out


def dampen(M):
    """test_gpu_fuzz.DAMPEN in turn: binary32 and non-binary32 factors side by side, so a
    narrow flat tile's wave (several clients) meets both (dampen_lane3's ballot)."""
    return [DAMPEN[c % len(DAMPEN)] for c in range(M)]


_expected = {}


def expected(oracle, name, mix, M):
    """(merged bytes, merged_f32) of the oracle's faithful per-op chain, computed once."""
    key = (name, mix, M)
    if key not in _expected:
        exp = oracle.update_faithful(uploads(oracle, name, mix, M), dampen(M))
        _expected[key] = (exp, oracle.decode_floats(exp))
    return _expected[key]


def sweep_cases():
    """Every (layout, M, mix) of the update sweep and the fused-step sweep."""
    ms = sorted({m for _, _, lst in UPDATE_FORMS.values() for m in lst} | set(M_FUSED) | {M_REJECT, M_OFF})
    return [(name, M, mix) for name in LAYOUTS for M in ms for mix in MIXES]


# -- item 5: rejection -------------------------------------------------------------
# 70 clients: at least two chunks of every form (the widest, Kardam's pipelined pass, 32)
# and both pipelined rings wrapped (slots reused from client 64)
M_REJECT = 70
# clients: the first, one of a later chunk of every form, one whose pass reuses a ring
# slot, the last
BAD_CLIENTS = (0, 33, 66, M_REJECT - 1)
LAYOUT_BAD_CLIENTS = (0, 37, M_REJECT - 2)


def needed_chars(name):
    """Base64 chars of the ragged last group that carry its values."""
    lay = LAYOUTS[name]
    r = lay.n_up - 3 * (groups_of(lay.n_up) - 1)
    return (32 * r + 5) // 6


def bad_char_cases(name):
    """(client, byte position, what) of the bad-char placements: a payload group that is
    neither group 0 nor a header group, in each of BAD_CLIENTS; a needed position of the
    ragged last group; a group of the second 16-group tile (hdrs: group 17; the ragged
    last group is the second tile of both widths in syn50 and of the 64-group tiles in hdrs)."""
    lay = LAYOUTS[name]
    g_last = groups_of(lay.n_up) - 1
    g_main = {"syn50": 5, "hdrs": 7}[name]
    cases = [(c, 16 * g_main + 5, "payload group") for c in BAD_CLIENTS]
    cases.append((35, 16 * g_last + needed_chars(name) - 1, "ragged last group"))
    if name == "hdrs":
        cases.append((50, 16 * 17 + 9, "second 16-group tile"))
    return cases


def corrupt_char(upload, pos):
    b = bytearray(upload)
    b[pos] = ord("*")
    return bytes(b)


def mismatch_upload(oracle, name, c, seed=SEED):
    lay = MISMATCH[name]
    return oracle.encode_floats(oracle.synth_upload(seed, c, list(lay.w_sizes), list(lay.b_sizes)))


# -- item 6: sums that leave the fast domain after many chunks ----------------------
M_OFF = 130
OFF_FROM = 66  # the first client with large values: past both pipelined rings' first wrap
# hdrs columns: beside header slots (61 | 62, 63 | 64, 133 | 134), the first payload
# slot, the ragged last group's only value
OFF_COLUMNS = (2, 61, 64, 100, 133, 192)


def off_domain_uploads(oracle, early):
    """130 gradient-like hdrs uploads with values of 9e7 .. 9.9e8 in OFF_COLUMNS from
    client 66 on (early: in clients 3 and 40 too), so the running sum passes 1e8 only
    after many chunks (or early and again late)."""
    rng = np.random.default_rng(SEED + 6 + int(early))
    ups = []
    for c in range(M_OFF):
        v = upload_values(oracle, "hdrs", 0, c).copy()
        if c >= OFF_FROM or (early and c in (3, 40)):
            # positive: the codec reads a negative value of this size back as a small one
            v[list(OFF_COLUMNS)] = rng.uniform(9e7, 9.9e8, len(OFF_COLUMNS)).astype(np.float32)
        ups.append(oracle.encode_floats(v))
    return ups


# -- item 4: k_kardam_reduce's instantiations ---------------------------------------
# launch_update_kardam: 4 partial slots (waves) per block of the stream grid; grid=plain
# has ceil(groups / 256) blocks, grid=lanes ceil(groups / 84). k_kardam_reduce<64, 8> up
# to 512 slots, <64, 32> up to 2048, <256, 32> beyond, whose strided tail runs past
# U * NT = 8192 slots.
STREAM_GROUPS_PER_BLOCK = {"update=stream,grid=plain": 256, "update=stream,grid=lanes": 84}
# (plan, slots, first n_up tried): the last sizes of 512 / 2048 slots, the first of 516 /
# 2052, and 8,212 slots (172,033 groups and more; four full blocks and a part of one past
# slot 8192, so the tail's slots hold payload sums, not just the trailing header's 0)
REDUCE_CASES = [("update=stream,grid=plain", 512, 3 * 128 * 256 - 30),
                ("update=stream,grid=plain", 516, 3 * 128 * 256 + 1),
                ("update=stream,grid=lanes", 512, 3 * 128 * 84 - 30),
                ("update=stream,grid=lanes", 516, 3 * 128 * 84 + 1),
                ("update=stream,grid=plain", 2048, 3 * 512 * 256 - 30),
                ("update=stream,grid=plain", 2052, 3 * 512 * 256 + 1),
                ("update=stream,grid=lanes", 8212, 3 * (2052 * 84 + 40))]


def roundtrip_size(oracle, n_up):
    """The next size whose N = n_up - 3 the codec round-trips (test_gpu_fuzz's loop: else
    the reference's own header walk misreads the bucket)."""
    while oracle.decode_floats(oracle.encode_floats(np.array([n_up - 3], np.float32)))[0] != n_up - 3:
        n_up += 1
    return n_up


def stream_slots(spec, n_up):
    per = STREAM_GROUPS_PER_BLOCK[spec]
    return 4 * ((groups_of(n_up) + per - 1) // per)
