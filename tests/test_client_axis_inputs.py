"""The inputs of test_gpu_client_axis.py, validated without a GPU: the expected values do
not hang on one restatement of the chain (the oracle's faithful per-op chain equals its
fused restatement on every case), every size's N survives the codec, the corrupt
uploads of the rejection tests differ from the clean ones in exactly the intended byte
or header codes, and the sizes of the k_kardam_reduce cases give the stated slot counts
by the grid formulas (pure arithmetic here; the GPU module holds them against
fleet_update_plan_grid)."""
import numpy as np
import pytest

import client_axis as A


@pytest.mark.parametrize("name", sorted(A.LAYOUTS))
def test_layouts_keep_the_edges(name):
    """At least 2 tiles at widths 16 and 64, a ragged last group, header slots in more
    than one tile."""
    lay = A.LAYOUTS[name]
    groups = A.groups_of(lay.n_up)
    assert groups > 64 or (name == "syn50" and groups > 16)  # syn50: two 16-group tiles, one ragged 64-group tile
    assert lay.n_up % 3 != 0
    assert A.b64_len(lay.n_up) % 16 != 0
    hdr_groups = {p // 3 for p in lay.header_positions()}
    assert len({g // 16 for g in hdr_groups}) > 1
    if name == "hdrs":
        assert lay.n_up == 193 and groups == 65
        assert lay.header_positions() == [0, 1, 62, 63, 134, 135, 166, 167]
        assert len({g // 64 for g in hdr_groups}) == 1 and (groups - 1) // 64 == 1  # the second 64-group tile: one group
    assert A.MISMATCH[name].n_up == lay.n_up


def test_sizes_round_trip(oracle):
    for lay in A.LAYOUTS.values():
        assert A.roundtrip_size(oracle, lay.n_up) == lay.n_up
        for s in lay.w_sizes + lay.b_sizes:
            assert oracle.decode_floats(oracle.encode_floats(np.array([s], np.float32)))[0] == s


def test_m_lists_sit_on_the_chunk_edges():
    """c - 1, c, c + 1, a second chunk, r * c + 1 and one M >= 129 per chunked form."""
    def edges(lst, c, r=1):
        return {c - 1, c, c + 1, r * c + 1} <= set(lst) | {0} and max(lst) >= 129
    assert edges(A.M_PIPE, 16, 4) and {1, 33, 64, 81} <= set(A.M_PIPE)
    assert edges(A.M_PIPE_KD, 32, 2) and {1, 64, 97} <= set(A.M_PIPE_KD)
    assert edges(A.M_CLASSIC, 8) and 17 in A.M_CLASSIC
    for w, lst in A.M_FLAT.items():
        assert edges(lst, 512 // w) and 2 * (512 // w) + 1 in lst
    for nw, lst in A.M_WEAVE.items():
        assert edges(lst, nw) and {1, 2 * nw, 2 * nw + 1, 3 * nw + 1} <= set(lst)
    assert {1, 2, 3, 4, 5, 8, 9} <= set(A.M_STREAM)
    assert {23, 24, 25, 49} <= set(A.M_FUSED) and max(A.M_FUSED) > 64
    for spec in ("update=pipe", "update=stream,grid=lanes", "update=tiled", "update=tiled,flat_w2=32",
                 "update=tiled,flat_w2=21", "update=tiled,tile=classic"):
        assert A.kardam_m_list(spec) in (A.M_PIPE_KD, A.M_STREAM, A.M_FLAT[16], A.M_FLAT[32])
    assert A.kardam_m_list("update=tiled,flat_w2=21") is A.M_FLAT[16]


@pytest.mark.parametrize("name", sorted(A.LAYOUTS))
def test_expected_values_do_not_depend_on_one_restatement(oracle, name):
    lay = A.LAYOUTS[name]
    hm = oracle.header_mask(list(lay.w_sizes), list(lay.b_sizes))
    assert list(np.flatnonzero(hm)) == lay.header_positions()
    n = 0
    for nm, M, mix in A.sweep_cases():
        if nm != name:
            continue
        ups, d = A.uploads(oracle, name, mix, M), A.dampen(M)
        assert len(ups) == M and all(len(u) == A.b64_len(lay.n_up) for u in ups)
        exp, f32 = A.expected(oracle, name, mix, M)
        assert exp == oracle.update_fused(ups, d, hm), (name, M, mix)
        assert len(f32) == lay.n_up
        n += 1
    ms = {m for _, _, lst in A.UPDATE_FORMS.values() for m in lst} | set(A.M_FUSED)
    assert n >= len(A.MIXES) * len(ms)


def test_uploads_keep_their_headers_and_carry_the_mix(oracle):
    for name, lay in A.LAYOUTS.items():
        hp = lay.header_positions()
        for mix in A.MIXES:
            v = np.stack([A.upload_values(oracle, name, mix, c) for c in range(A.M_OFF)])
            assert np.array_equal(v[:, hp], np.tile(np.asarray(lay.header_values(), np.float32), (A.M_OFF, 1)))
            assert len({A.uploads(oracle, name, mix, A.M_OFF)[c] for c in range(A.M_OFF)}) == A.M_OFF
        wide = np.stack([A.upload_values(oracle, name, 1, c) for c in range(A.M_OFF)])
        assert np.abs(wide).max() >= 1e8  # mix 1 holds values past the fast domain
        edge = np.stack([A.upload_values(oracle, name, 2, c) for c in range(A.M_OFF)])
        assert not np.isfinite(edge).all()  # mix 2 sprinkles inf / NaN


def test_off_domain_payloads_trip_late(oracle):
    lay = A.LAYOUTS["hdrs"]
    hp = set(lay.header_positions())
    assert not hp & set(A.OFF_COLUMNS) and 3 * (A.groups_of(lay.n_up) - 1) in A.OFF_COLUMNS
    assert any(c + 1 in hp for c in A.OFF_COLUMNS) and any(c - 1 in hp for c in A.OFF_COLUMNS)
    hm = oracle.header_mask(list(lay.w_sizes), list(lay.b_sizes))
    for early in (False, True):
        ups = A.off_domain_uploads(oracle, early)
        assert len(ups) == A.M_OFF and A.OFF_FROM > 64
        v = np.stack([oracle.decode_floats(u) for u in ups])
        cols = list(A.OFF_COLUMNS)
        big = np.abs(v[:, cols]) >= 8.9e7
        assert big[A.OFF_FROM:].all() and bool(big[: A.OFF_FROM].any()) == early
        if not early:  # no partial sum of the first 66 clients can reach 1e8 (every dampening factor <= 2)
            assert max(A.DAMPEN) <= 2.0
            assert 2.0 * np.abs(np.delete(v[: A.OFF_FROM], sorted(hp), axis=1)).sum(axis=0).max() < 1e8
        assert oracle.update_faithful(ups, A.dampen(A.M_OFF)) == oracle.update_fused(ups, A.dampen(A.M_OFF), hm)


@pytest.mark.parametrize("name", sorted(A.LAYOUTS))
def test_corrupt_uploads_differ_as_intended(oracle, name):
    lay = A.LAYOUTS[name]
    L = A.b64_len(lay.n_up)
    ups = A.uploads(oracle, name, 0, A.M_REJECT)
    hdr_groups = {p // 3 for p in lay.header_positions()}
    g_last = A.groups_of(lay.n_up) - 1
    assert {c // 32 for c in A.BAD_CLIENTS} >= {0, 1, 2} and max(A.BAD_CLIENTS) == A.M_REJECT - 1
    assert any(64 <= c < A.M_REJECT - 1 for c in A.BAD_CLIENTS)  # a reused ring slot
    whats = set()
    for c, pos, what in A.bad_char_cases(name):
        bad = A.corrupt_char(ups[c], pos)
        assert len(bad) == L and pos < L
        assert [i for i in range(L) if bad[i] != ups[c][i]] == [pos] and ups[c][pos:pos + 1] not in (b"*", b"=")
        g = pos // 16
        if what == "ragged last group":
            assert g == g_last and pos % 16 < A.needed_chars(name)
        else:
            assert g != 0 and g not in hdr_groups and g != g_last
        if what == "second 16-group tile":
            assert g // 16 == 1
        whats.add(what)
    assert {"payload group", "ragged last group"} <= whats
    # the layout mismatch: same length, other codes in the clean layout's header slots
    hp = lay.header_positions()
    want = {"hdrs": ({1, 63}, {1, 62, 63}), "syn50": ({0, 1}, {0, 1})}[name]
    for c in A.LAYOUT_BAD_CLIENTS:
        assert 0 <= c < A.M_REJECT - 1  # never the last upload, whose header the others are held against
        bad = A.mismatch_upload(oracle, name, c)
        assert len(bad) == L
        good_codes, bad_codes = oracle.decode_ints(ups[c]), oracle.decode_ints(bad)
        differ = {p for p in hp if good_codes[p] != bad_codes[p]}
        assert want[0] <= differ <= want[1], differ
    assert A.LAYOUT_BAD_CLIENTS[0] == 0 and A.LAYOUT_BAD_CLIENTS[-1] == A.M_REJECT - 2
    assert 8 < A.LAYOUT_BAD_CLIENTS[1] < 64 and A.LAYOUT_BAD_CLIENTS[1] >= 32


def test_reduce_sizes_give_the_stated_slots(oracle):
    """4 slots per block of the stream grid: 512 / 516 and 2048 / 2052 sit on the edges of
    k_kardam_reduce's three instantiations, more than 8192 reach its strided tail."""
    slots = set()
    for spec, want, n0 in A.REDUCE_CASES:
        n = A.roundtrip_size(oracle, n0)
        assert n - n0 < 8
        assert A.stream_slots(spec, n) == want, (spec, n)
        slots.add(want)
    assert {512, 516, 2048, 2052} <= slots and max(slots) > 8192
    spec, want, n0 = A.REDUCE_CASES[-1]
    assert A.groups_of(n0) >= 172_033 and "lanes" in spec
