"""The upload pool (fleet_pool: Codec.pool, k_pool_fold): uploads kept in slots in HBM, any
subset of them aggregated in any order, gives the bytes the reference's chain over those
uploads in that order gives (CppNNUpdater.java:383-411, 420-421, 463-464, 490-508; the
staleSize > 0 branch, where StalenessSimulator.java:38-176 picks among the buffered
uploads). Every expected value is the oracle's (the faithful per-op chain or the fused
restatement) or a recorded fixture; the host and device forms appear beside them."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import fleet_amd as F
import layout_axis as A
from fleet_amd.layouts import MNIST, Layout, synthetic
from test_gpu_acc import CHAINS, EDGE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BURST = 64  # picks per launch (fleet_acc_burst)
# binary32 values (dampen_stage's f32 multiply) in turn with values that are none (its f64 multiply)
MIXED = (0.5, 1 / 3, 1.0, math.exp(-0.7), 0.25, 0.1)


def uploads_for(oracle, layout, M, seed):
    return [oracle.encode_floats(oracle.synth_upload(seed, c, list(layout.w_sizes), list(layout.b_sizes)))
            for c in range(M)]


def mixed(K):
    return [MIXED[k % len(MIXED)] for k in range(K)]


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def scrambled(slots, n, seed):
    """n distinct slots of the pool in a scrambled order."""
    return [int(s) for s in np.random.default_rng(seed).permutation(slots)[:n]]


def filled(codec, hp, ups, slots, where=None):
    """A pool holding ups[i] in slot where[i] (default: slot i)."""
    pool = codec.pool(len(ups[0]), hp, slots)
    for i, u in enumerate(ups):
        pool.put(i if where is None else where[i], u)
    return pool


def check(oracle, pool, slot_of, ups, order, d, fused_mask=None):
    """pool.update over the uploads `order` (indices into ups) equals the oracle's chain."""
    merged, f32 = pool.update([slot_of[i] for i in order], d, want_f32=True)
    picked = [ups[i] for i in order]
    exp = oracle.update_faithful(picked, d) if fused_mask is None else oracle.update_fused(picked, d, fused_mask)
    assert merged == exp
    assert same_bits(f32, oracle.decode_floats(exp))


# 1 ---------------------------------------------------------------- recorded chains

@pytest.mark.parametrize("name", CHAINS)
def test_recorded_chains(codec, name):
    z = np.load(os.path.join(GOLDEN, f"chain_{name}.npz"))
    lens = z["upload_lens"]
    M = int(z["M"])
    ups = [z["uploads"][c, : lens[c]].tobytes() for c in range(M)]
    lay = Layout(name, tuple(int(s) for s in z["w_sizes"]), tuple(int(s) for s in z["b_sizes"]))
    where = scrambled(M + 3, M, seed=M)
    with filled(codec, lay.header_positions(), ups, M + 3, where) as pool:
        assert pool.slots == M + 3 and sorted(s for s in range(pool.slots) if pool.occupied(s)) == sorted(where)
        assert pool.update(where, [float(x) for x in z["dampen"]]) == z["merged"].tobytes()
        assert all(pool.slot_status(s) == 0 for s in range(pool.slots))


# 2 --------------------------------------------------------------- subset and order

@pytest.fixture(scope="module")
def mnist8(oracle):
    return uploads_for(oracle, MNIST, 8, seed=108)


def test_subset_and_order(codec, oracle, mnist8):
    where = [9, 0, 4, 11, 2, 7, 5, 1]
    assert len(set(mnist8)) == 8  # unpicked slots hold different uploads
    with filled(codec, MNIST.header_positions(), mnist8, 12, where) as pool:
        assert pool.free_slot() == 3
        for order in ([5, 2, 7], [7, 2, 5], list(range(7, -1, -1))):
            check(oracle, pool, where, mnist8, order, mixed(len(order)))
        assert sorted(s for s in range(12) if pool.occupied(s)) == sorted(where)  # an update frees nothing


# 3 ------------------------------------------------------------------ tiny layouts

@pytest.mark.parametrize("n_up", [3, 4, 5, 6, 7])
def test_tiny_layouts(codec, oracle, n_up):
    """One partial group, and K = 1, where the first pick is the whole chain and the last pick at once."""
    lay = synthetic(n_up)
    ups = uploads_for(oracle, lay, 3, seed=n_up * 10)
    with filled(codec, lay.header_positions(), ups, 4, [3, 0, 2]) as pool:
        for order in ([1], [2, 0], [1, 2, 0]):
            check(oracle, pool, [3, 0, 2], ups, order, [math.exp(-0.5 * k) for k in range(len(order))])


# 4 ------------------------------------------------------------------ launch edges

@pytest.fixture(scope="module")
def pool130(codec, oracle):
    lay = synthetic(50)
    ups = uploads_for(oracle, lay, 130, seed=504)
    where = scrambled(130, 130, seed=4)
    pool = filled(codec, lay.header_positions(), ups, 130, where)
    yield pool, ups, where
    pool.close()


@pytest.mark.parametrize("K", [BURST - 1, BURST, BURST + 1, 2 * BURST, 2 * BURST + 1])
def test_launch_edges(oracle, pool130, K):
    """A state round trip at each 64-pick boundary, the finish form as a launch of 1 pick, and
    both branches of dampen_stage inside one launch."""
    assert F.ACC_BURST == BURST
    pool, ups, where = pool130
    order = scrambled(130, K, seed=K)
    check(oracle, pool, where, ups, order, mixed(K))


# 5 ------------------------------------------------- multi-block and ragged tail

@pytest.mark.parametrize("n_up,K", [(100000, 9), (99998, 5)])
def test_multi_block_vs_fused_oracle(codec, oracle, n_up, K):
    lay = synthetic(n_up)
    ups = uploads_for(oracle, lay, K, seed=7)
    where = scrambled(K + 1, K, seed=n_up)
    hm = oracle.header_mask(list(lay.w_sizes), list(lay.b_sizes))
    with filled(codec, lay.header_positions(), ups, K + 1, where) as pool:
        check(oracle, pool, where, ups, list(range(K - 1, -1, -1)), [1 / ((c % 3) + 1) for c in range(K)], hm)


# 6 ------------------------------------------------------- out-of-domain payloads

def edge_uploads(oracle, lay, K, seed, at):
    """Gradient-like payloads; upload `at` alone carries the EDGE values (|x| >= 1e8, >= 1e9,
    +-inf, NaN, denormals), which leave the table stages' domain."""
    rng = np.random.default_rng(seed)
    n = lay.n_up - 3
    ups = []
    for c in range(K):
        v = oracle.synth_upload(seed, c, list(lay.w_sizes), list(lay.b_sizes))
        p = rng.normal(0, 1e-2, n).astype(np.float32)
        if c == at:
            k = max(len(EDGE), n // 8)
            p[rng.choice(n, k, replace=False)] = np.resize(EDGE, k)
        v[2:lay.n_up - 1] = p
        ups.append(oracle.encode_floats(v))
    return ups


@pytest.mark.parametrize("at", [0, 2, 4], ids=["first", "middle", "last"])
@pytest.mark.parametrize("n_up", [159, 1001])
def test_out_of_domain_payloads(codec, oracle, n_up, at):
    lay = synthetic(n_up)
    ups = edge_uploads(oracle, lay, 5, 4100 + n_up + at, at)
    with filled(codec, lay.header_positions(), ups, 5) as pool:
        check(oracle, pool, list(range(5)), ups, list(range(5)), [1 / 3, math.exp(-0.7), 7.25e3, 1.0, 1 / 3])


@pytest.mark.parametrize("K,first", [(3, 0), (66, 63)], ids=["k3", "across_launches"])
def test_running_sum_leaves_the_table_domain(codec, oracle, K, first):
    """Three picks of 6e7 at the same positions: each is inside the table stages' domain, the
    running sum leaves it at the second of them (1.2e8) -- inside one launch, and with the
    three at positions 63, 64 and 65 of a 66-pick list, across the launch boundary."""
    lay = synthetic(159)
    rng = np.random.default_rng(66)
    ups = []
    for c in range(K):
        v = oracle.synth_upload(660, c, list(lay.w_sizes), list(lay.b_sizes))
        v[2:lay.n_up - 1] = rng.normal(0, 1e-2, lay.n_up - 3).astype(np.float32)
        if first <= c < first + 3:
            v[[5, 17, 60, 61, 62, 150]] = [6e7, -6e7, 6e7, 6e7, -6e7, 6e7]
        ups.append(oracle.encode_floats(v))
    d = [1.0 if first <= c < first + 3 else MIXED[c % len(MIXED)] for c in range(K)]
    where = scrambled(K, K, seed=K)
    with filled(codec, lay.header_positions(), ups, K, where) as pool:
        check(oracle, pool, where, ups, list(range(K)), d)


# 7 ------------------------------------------------------------------ header lists

@pytest.mark.parametrize("n_hdr", [0, 1])
def test_short_header_lists(codec, oracle, n_hdr):
    """No header slot at all, and one: the list is the caller's, the oracle's fused chain takes
    the same mask (header slots keep the last pick's code)."""
    lay = synthetic(1000)
    ups = uploads_for(oracle, lay, 4, seed=70 + n_hdr)
    hp = lay.header_positions()[:n_hdr]
    hm = np.zeros(lay.n_up, np.uint8)
    hm[hp] = 1
    with filled(codec, hp, ups, 4) as pool:
        check(oracle, pool, list(range(4)), ups, [2, 0, 3], mixed(3), hm)


@pytest.mark.parametrize("n_hdr", [A.ACC_LDS_HDR, A.ACC_LDS_HDR + 1])
def test_dense_header_lists(codec, oracle, n_hdr):
    """The block's LDS copy of the list and the search in global memory, either side of
    kAccLdsHdr, on a header-dense layout in which groups hold 2 and 3 header slots."""
    lay = A.dense(n_hdr)
    hp = lay.header_positions()
    bits = A.header_bits(lay)
    assert len(hp) == n_hdr and {3, 5, 6} & set(bits.tolist()) and 7 in bits
    ups = A.uploads(oracle, lay, 3)
    with filled(codec, hp, ups, 5, [4, 1, 2]) as pool:
        merged, f32 = pool.update([4, 1, 2], A.dampen(3), want_f32=True)
        exp, exp32 = A.expected(oracle, lay, 3)
        assert merged == exp and same_bits(f32, exp32)
        check(oracle, pool, [4, 1, 2], ups, [2, 0], A.dampen(2))


# 8 ------------------------------------------------------------------------ window

def test_window(codec, oracle):
    """A window strictly inside the upload: the host and the device forms write exactly the
    window's bytes and values, the sentinels outside it survive."""
    torch = pytest.importorskip("torch")
    lay = synthetic(1000)
    ups = uploads_for(oracle, lay, 4, seed=88)
    order, d = [3, 0, 2], mixed(3)
    L = len(ups[0])
    G = (lay.n_up + 2) // 3
    gb, ge = 5, 200
    assert 0 < gb < ge < G
    exp = np.frombuffer(oracle.update_faithful([ups[i] for i in order], d), np.uint8)
    exp32 = oracle.decode_floats(exp.tobytes())
    b0, b1, v0, v1 = 16 * gb, 16 * ge, 3 * gb, 3 * ge
    picks = np.array(order, np.int32)
    dd = np.array(d, np.float64)
    with codec.pool(L, lay.header_positions(), 4, gb, ge) as pool:
        for s, u in enumerate(ups):
            pool.put(s, u)
        out = np.full(L + 16, 0xA5, np.uint8)
        f32 = np.full(lay.n_up + 1, -7.5, np.float32)
        n = C.c_size_t(0)
        rc = F.lib().fleet_pool_update(pool._h, picks.ctypes.data, 3, dd.ctypes.data, out.ctypes.data, len(out),
                                       C.byref(n), f32.ctypes.data)
        assert rc == F.FLEET_OK and n.value == L
        assert (out[:b0] == 0xA5).all() and (out[b1:] == 0xA5).all() and np.array_equal(out[b0:b1], exp[b0:b1])
        assert (f32[:v0] == -7.5).all() and (f32[v1:] == -7.5).all() and same_bits(f32[v0:v1], exp32[v0:v1])
        dev_rows = torch.zeros((4, 16 * G), dtype=torch.uint8, device="cuda")
        for s, u in enumerate(ups):
            dev_rows[s, :L] = torch.from_numpy(np.frombuffer(u, np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        for s in range(4):
            pool.drop(s)
            pool.put_device(s, dev_rows[s])
        m_dev = torch.full((16 * G,), 0xA5, dtype=torch.uint8, device="cuda")
        f_dev = torch.full((3 * G,), -7.5, dtype=torch.float32, device="cuda")
        pool.update_device(order, d, m_dev, f_dev)
        m, f = m_dev.cpu().numpy(), f_dev.cpu().numpy()
        assert (m[:b0] == 0xA5).all() and (m[b1:] == 0xA5).all() and np.array_equal(m[b0:b1], exp[b0:b1])
        assert (f[:v0] == -7.5).all() and (f[v1:] == -7.5).all() and same_bits(f[v0:v1], exp32[v0:v1])


# 9 ----------------------------------------------------- persistence across updates

def test_persistence_across_updates(codec, oracle):
    """The staleSize > 0 pattern: picked slots are dropped and refilled, later updates mix old
    and new uploads; the kernel's state and hfirst[] of earlier updates do not leak."""
    lay = synthetic(1001)
    ups = uploads_for(oracle, lay, 8, seed=99)
    held = dict(enumerate(ups[:6]))  # slot -> upload
    with filled(codec, lay.header_positions(), ups[:6], 6) as pool:
        def update(picks, d):
            merged, f32 = pool.update(picks, d, want_f32=True)
            exp = oracle.update_faithful([held[s] for s in picks], d)
            assert merged == exp and same_bits(f32, oracle.decode_floats(exp))
        update([3, 0], [1 / 3, 0.5])
        for s in (3, 0):
            pool.drop(s)
            assert not pool.occupied(s)
        assert pool.free_slot() == 0
        for s, u in ((0, ups[6]), (3, ups[7])):
            pool.put(s, u)
            held[s] = u
        update([4, 0, 1, 3], mixed(4))
        update([5, 2], [math.exp(-0.7), 1.0])  # slots never picked before


# 10 ----------------------------------------------------------------- device forms

def test_device_forms(codec, oracle):
    torch = pytest.importorskip("torch")
    lay = synthetic(99998)
    K = 5
    ups = uploads_for(oracle, lay, K, seed=81)
    d = mixed(K)
    L = len(ups[0])
    pitch = 16 * ((L + 15) // 16)
    G = pitch // 16
    host = np.zeros((K, pitch), np.uint8)
    for c, u in enumerate(ups):
        host[c, :L] = np.frombuffer(u, np.uint8)
    dev = torch.from_numpy(host).cuda()
    where = [6, 2, 0, 5, 3]
    order = [4, 1, 3, 0, 2]
    picks = [where[i] for i in order]
    exp = oracle.update_faithful([ups[i] for i in order], d)
    merged = torch.zeros(pitch, dtype=torch.uint8, device="cuda")
    f32 = torch.zeros(3 * G, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with codec.pool(L, lay.header_positions(), 7) as pool:
        for c in range(K):
            pool.put_device(where[c], dev[c], stream=side.cuda_stream)
        assert sorted(s for s in range(7) if pool.occupied(s)) == sorted(where)
        pool.update_device(picks, d, merged, f32, stream=side.cuda_stream)
        torch.cuda.synchronize()
        assert merged.cpu().numpy()[:L].tobytes() == exp
        assert same_bits(f32.cpu().numpy()[: lay.n_up], oracle.decode_floats(exp))
        # a host update over device puts, and host puts beside them, give the same bytes
        hm, hf = pool.update(picks, d, want_f32=True)
        assert hm == exp and same_bits(hf, oracle.decode_floats(exp))
        pool.put(1, ups[0])
        pool.put_device(4, dev[1], stream=side.cuda_stream)
        assert pool.update([1, 4], d[:2]) == oracle.update_faithful(ups[:2], d[:2])
        bad = host[1].copy()
        bad[333] = ord("*")
        bad_dev = torch.from_numpy(bad).cuda()
        pool.put_device(2, bad_dev, stream=side.cuda_stream)
        with pytest.raises(F.Base64Error) as ei:
            pool.update_device(picks, d, merged, f32, stream=side.cuda_stream)
        assert ei.value.slots == [2] and [s for s in range(7) if pool.slot_status(s)] == [2]


# 11 ----------------------------------------------------------------------- errors

@pytest.fixture(scope="module")
def pool70(codec, oracle):
    lay = synthetic(1001)
    ups = uploads_for(oracle, lay, 70, seed=111)
    g = ups[1]
    star = g[:40] + b"*" + g[41:]  # a payload group: no header slot in it
    assert 40 // 16 not in [p // 3 for p in lay.header_positions()]
    v = oracle.synth_upload(111, 1, list(lay.w_sizes), list(lay.b_sizes))
    v[0] = 2.0  # a differing header slot
    hdr = oracle.encode_floats(v)
    assert len(hdr) == len(g)
    pool = filled(codec, lay.header_positions(), ups, 73)
    pool.put(70, star)
    pool.put(71, hdr)
    yield pool, ups, lay
    pool.close()


def flagged(pool):
    return {s: pool.slot_status(s) for s in range(pool.slots) if pool.slot_status(s)}


@pytest.mark.parametrize("K,at", [(3, 0), (3, 1), (3, 2), (70, 66)], ids=["first", "middle", "last", "past64"])
def test_malformed_base64_names_its_slot(oracle, pool70, K, at):
    pool, ups, _ = pool70
    rest = scrambled(70, K - 1, seed=10 * K + at)
    picks = rest[:at] + [70] + rest[at:]
    d = mixed(K)
    with pytest.raises(F.Base64Error) as ei:
        pool.update(picks, d, want_f32=True)
    assert ei.value.code == F.FLEET_ERR_BASE64 and ei.value.slots == [70]
    assert flagged(pool) == {70: 1}
    # the pool was not disturbed, and a malformed upload in an unpicked slot fails nothing
    assert all(pool.occupied(s) for s in range(72))
    dr = d[:at] + d[at + 1:]
    merged, f32 = pool.update(rest, dr, want_f32=True)
    exp = oracle.update_faithful([ups[s] for s in rest], dr)
    assert merged == exp and same_bits(f32, oracle.decode_floats(exp))
    assert flagged(pool) == {}


def test_layout_mismatch_names_the_slots_that_differ_from_the_first_pick(oracle, pool70):
    pool, ups, _ = pool70
    with pytest.raises(F.LayoutError) as ei:
        pool.update([4, 71, 9], mixed(3))
    assert ei.value.code == F.FLEET_ERR_LAYOUT and ei.value.slots == [71] and flagged(pool) == {71: 2}
    # the same upload as the first pick defines the update's header: the others differ from it
    with pytest.raises(F.LayoutError) as ei:
        pool.update([71, 4, 9], mixed(3))
    assert ei.value.slots == [4, 9] and flagged(pool) == {4: 2, 9: 2}
    # Base64 comes before layout
    with pytest.raises(F.Base64Error) as ei:
        pool.update([4, 71, 70], mixed(3))
    assert flagged(pool) == {71: 2, 70: 1} and ei.value.slots == [71, 70]
    assert pool.update([9, 4], [0.5, 1 / 3]) == oracle.update_faithful([ups[9], ups[4]], [0.5, 1 / 3])


def test_argument_errors_touch_nothing(oracle, pool70):
    pool, ups, lay = pool70
    L = F.lib()
    n_len = len(ups[0])
    with pytest.raises(F.Base64Error):
        pool.update([3, 70], [1.0, 1.0])
    assert flagged(pool) == {70: 1}
    assert not pool.occupied(72)
    pool.put(69, ups[69])
    pool.drop(69)  # a dropped slot
    out = np.full(n_len + 16, 0xA5, np.uint8)
    f32 = np.full(lay.n_up + 1, -7.5, np.float32)
    d = np.array(mixed(3), np.float64)

    def refused(picks, K=None):
        pk = np.array(picks, np.int32)
        n = C.c_size_t(0)
        K = len(pk) if K is None else K
        rc = L.fleet_pool_update(pool._h, pk.ctypes.data, K, d.ctypes.data, out.ctypes.data, len(out), C.byref(n),
                                 f32.ctypes.data)
        assert rc == F.FLEET_ERR_ARG
        assert (out == 0xA5).all() and (f32 == -7.5).all() and flagged(pool) == {70: 1}
        with pytest.raises(F.FleetError) as ei:
            pool.update(picks[:K], list(d[:K]))
        assert ei.value.code == F.FLEET_ERR_ARG and flagged(pool) == {70: 1}

    refused([1, 73, 2])      # out of range
    refused([1, -1, 2])
    refused([1, 72, 2])      # never occupied
    refused([1, 69, 2])      # dropped
    refused([1, 2, 1])       # twice
    refused([1, 2, 3], K=0)
    for bad_slot in (73, -1):
        for call in (lambda s: pool.put(s, ups[0]), pool.drop, pool.occupied, pool.slot_status):
            with pytest.raises(F.FleetError) as ei:
                call(bad_slot)
            assert ei.value.code == F.FLEET_ERR_ARG
    with pytest.raises(F.FleetError) as ei:
        pool.put(5, ups[5][:-4])  # another length
    assert ei.value.code == F.FLEET_ERR_ARG
    assert pool.update([5, 6], [1.0, 0.5]) == oracle.update_faithful([ups[5], ups[6]], [1.0, 0.5])  # slot 5 is as it was
    # capacity
    n = C.c_size_t(0)
    pk = np.array([1, 2, 3], np.int32)
    rc = L.fleet_pool_update(pool._h, pk.ctypes.data, 3, d.ctypes.data, out.ctypes.data, n_len - 1, C.byref(n), None)
    assert rc == F.FLEET_ERR_CAPACITY and n.value == n_len and (out == 0xA5).all()
    with pytest.raises(F.FleetError) as ei:
        pool.codec.pool(n_len, lay.header_positions(), 0)
    assert ei.value.code == F.FLEET_ERR_ARG
    pool.put(69, ups[69])


# 12 ------------------------------------------------------- FleetUpdater end to end

def test_updater_with_a_picker(codec, oracle):
    """M = 3, staleSize = 2, inverse dampening, the small layout of the recorded chains. The
    scripted picker returns None, then None with one entry discarded (with M = 3 a call that
    picks leaves fewer than M behind, so a discard next to leftovers needs a call that picks
    nothing), then a non-FIFO subset, then the leftover together with new arrivals."""
    from fleet_amd.updater import FleetUpdater, get_dampen
    lay = Layout("small", (200, 0, 128), (30, 10), (1,))
    rng = np.random.default_rng(12)
    w = rng.normal(0, 0.05, lay.n_weights).astype(np.float32)
    b = rng.normal(0, 0.05, lay.n_fc_bias).astype(np.float32)
    lrates = [0.05, 0.02, 0.01]
    script = [(None, []), (None, [1]), ([3, 0, 2], []), ([1, 0, 2], [])]
    seen = []

    def picker(pending, curr_epoch):
        seen.append([p.client_id for p in pending])
        return script.pop(0)

    u = FleetUpdater(codec, lay, 3, lrates, w, b, policy=1, stale_size=2, picker=picker)
    ups = uploads_for(oracle, lay, 7, seed=120)
    epochs = [0, 0, 0, 0, 0, 1, 0]
    # arrival -> the clients its update picks, in pick order
    picked_at = {4: [4, 0, 3], 6: [5, 2, 6]}
    epoch = 0
    for i, up in enumerate(ups):
        got = u.update(up, [i % 10] * 10, epochs[i], client_id=i)
        if i in picked_at:
            ids = picked_at[i]
            d = [get_dampen(1, epoch - epochs[c]) for c in ids]
            exp = oracle.update_faithful([ups[c] for c in ids], d)
            assert got == exp
            w, b = oracle.descent(w, b, oracle.decode_floats(exp), lay.w_present(), lay.fc_flags(),
                                  np.float32(lrates[epoch]))
            epoch += 1
        else:
            assert got is None
        assert same_bits(u.weights, w) and same_bits(u.fc_bias, b) and u.curr_epoch == epoch
    assert seen == [[0, 1, 2], [0, 1, 2, 3], [0, 2, 3, 4], [2, 5, 6]] and script == []
    assert u.acc == [] and not any(u._pool.occupied(s) for s in range(u._pool.slots))
    assert len({get_dampen(1, 1 - e) for e in (0, 1)}) == 2  # the second update dampened its stale picks
