"""The arrival gate (fleet_gate: Pool.gate, k_pool_vet) against the oracle: per resident
slot the Base64 verdict an update's fold reaches, the header codes against the model's, and
the squared norm and largest magnitude of the flat gradient -- new
ByteVec(getFlatGradient(g)).getNorm(), cppNN_backend.cpp:701-720, 779-795.

sumsq is checked to 1e-12 relative against oracle.norm(oracle.flat_gradient(u)) squared (the
tolerance every norm of this suite carries: another summation order of the same fp32
products in double), max_abs bit for bit against max |oracle.decode_floats(
oracle.flat_gradient(u))|. The Base64 and layout verdicts are compared with what
Pool.update reports for the same slot."""
import numpy as np
import pytest

import fleet_amd as F
import layout_axis as A
from fleet_amd.layouts import MNIST, synthetic
from test_gpu_acc import EDGE

pytestmark = pytest.mark.gpu

BURST = 64
RTOL = 1e-12
SHAPES = {"synthetic7": synthetic(7), "synthetic8": synthetic(8), "synthetic9": synthetic(9),
          "synthetic50003": synthetic(50_003), "mnist": MNIST, "dense1025": A.dense(1025)}


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def payload(lay):
    m = np.ones(lay.n_up, bool)
    m[lay.header_positions()] = False
    return m


# codes whose decoded value int2float leaves undivided (last digit 9, or the sign's extremes):
# |dec(code)| >= 1e9, past the table stages' domain, so Q runs the general codec
EXTREME = np.array([1999999999, -1999999999, 2147483647, -2147483648, 999999999, -1000000009], np.int32)


def upload_of(oracle, lay, kind, seed=11):
    """One upload: the synthetic mix, the mix with magnitudes at the codec's
    limit among it (values the encoder saturates on and codes that leave the table stages'
    domain), or a payload of zeros."""
    v = oracle.synth_upload(seed, 0, list(lay.w_sizes), list(lay.b_sizes)).copy()
    pay = np.flatnonzero(payload(lay))
    if kind == "zeros":
        v[pay] = 0.0
    if kind != "edge":
        return oracle.encode_floats(v)
    rng = np.random.default_rng(seed)
    at = rng.choice(pay, min(len(pay), max(4, len(pay) // 8)), replace=False)
    v[at] = EDGE[np.arange(len(at)) % len(EDGE)]
    codes = oracle.decode_ints(oracle.encode_floats(v)).copy()
    codes[at[::2]] = EXTREME[np.arange(len(at[::2])) % len(EXTREME)]
    return oracle.encode_ints(codes)


_ref = {}


def reference(oracle, u):
    """(sumsq, max_abs) of a good upload, from the oracle's flat gradient; computed once."""
    if u not in _ref:
        flat = oracle.flat_gradient(u)
        f = oracle.decode_floats(flat)
        _ref[u] = (oracle.norm(flat) ** 2, np.float32(np.abs(f).max()) if len(f) else np.float32(0))
    return _ref[u]


def agrees(v, ref, status=0):
    assert v.status == status
    assert abs(v.sumsq - ref[0]) <= RTOL * ref[0], (v.sumsq, ref[0])
    assert bits(v.max_abs) == bits(ref[1]), (v.max_abs, ref[1])
    assert v.norm == float(np.sqrt(v.sumsq))


def fold_status(pool, picks, slot):
    """What Pool.update over `picks` reports for `slot`."""
    try:
        pool.update(picks, [1.0] * len(picks))
    except (F.Base64Error, F.LayoutError) as e:
        assert slot in e.slots
    return pool.slot_status(slot)


def spoil(u, at, ch=b"!"):
    return u[:at] + ch + u[at + 1:]


# 1 --------------------------------------------------------------- values and shapes

@pytest.fixture(scope="module")
def trios(oracle):
    out = {}
    for name, lay in SHAPES.items():
        out[name] = [upload_of(oracle, lay, kind) for kind in ("mix", "edge", "zeros")]
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_norm_and_max_against_the_oracle(codec, oracle, trios, name):
    lay, ups = SHAPES[name], trios[name]
    with codec.pool(len(ups[0]), lay.header_positions(), 4) as pool:
        for s, u in zip((2, 0, 3), ups):
            pool.put(s, u)
        with pool.gate(lay.header_values()) as gate, pool.gate() as plain:
            got = gate.vet([2, 0, 3])
            for v, u in zip(got, ups):
                agrees(v, reference(oracle, u))
            assert got[2].sumsq == 0.0 and got[2].max_abs == 0.0  # the payload of zeros
            assert plain.vet([2, 0, 3]) == got  # the header check changes no number
            assert gate.vet([3, 2]) == [got[2], got[0]]
        assert all(pool.slot_status(s) == 0 for s in range(4))


# 2 -------------------------------------------------------------------------- windows

def test_windows_add(codec, oracle, trios):
    """A window that begins inside a run of header slots (groups 63 | 64 of the dense layouts)
    with more than kAccLdsHdr headers: the two windows' sums add to the whole pool's, the
    larger max_abs is the whole's, and a header is checked against its index in the whole
    upload."""
    lay = SHAPES["dense1025"]
    a, _ = A.window_cuts(lay)
    G = A.groups_of(lay.n_up)
    assert A.header_bits(lay)[a - 1] == 7 and A.header_bits(lay)[a] == 7 and A.headers_before(lay, a) > 0
    last = len(lay.header_positions()) - 1
    ups = trios["dense1025"][:2] + [A.mismatch_upload(oracle, lay, last, 0)]
    res = []
    for gb, ge in ((0, G), (0, a), (a, G)):
        with codec.pool(len(ups[0]), lay.header_positions(), 3, gb, ge) as pool:
            for s, u in enumerate(ups):
                pool.put(s, u)
            with pool.gate(lay.header_values()) as gate:
                res.append(gate.vet([0, 1, 2]))
    whole, lo, hi = res
    for k in range(2):
        agrees(whole[k], reference(oracle, ups[k]))
        assert abs(lo[k].sumsq + hi[k].sumsq - whole[k].sumsq) <= RTOL * whole[k].sumsq
        assert bits(max(lo[k].max_abs, hi[k].max_abs)) == bits(whole[k].max_abs)
        assert lo[k].status == hi[k].status == 0 and 0 < lo[k].sumsq < whole[k].sumsq
    assert (whole[2].status, lo[2].status, hi[2].status) == (2, 0, 2)  # the last header lies in the second window


# 3 ---------------------------------------------------- launches and independence

@pytest.fixture(scope="module")
def pool65(codec, oracle):
    lay = synthetic(50)
    ups = [upload_of(oracle, lay, "edge" if c % 9 == 4 else "mix", seed=300 + c) for c in range(65)]
    pool = codec.pool(len(ups[0]), lay.header_positions(), 65)
    for s, u in enumerate(ups):
        pool.put(s, u)
    gate = pool.gate(lay.header_values())
    yield pool, gate, ups
    gate.close()
    pool.close()


@pytest.mark.parametrize("K", [1, BURST, BURST + 1])
def test_burst_sizes(oracle, pool65, K):
    assert F.ACC_BURST == BURST
    pool, gate, ups = pool65
    order = [int(s) for s in np.random.default_rng(K).permutation(65)[:K]]
    got = gate.vet(order)
    assert len(got) == K
    for v, s in zip(got, order):
        agrees(v, reference(oracle, ups[s]))


def test_device_form(pool65):
    import torch
    pool, gate, _ = pool65
    order = list(range(64, -1, -1))
    st = torch.full((66,), 9, dtype=torch.int32, device="cuda")
    ss = torch.full((66,), -1.0, dtype=torch.float64, device="cuda")
    mx = torch.full((66,), -1.0, dtype=torch.float32, device="cuda")
    gate.vet_device(order, st, ss, mx)
    torch.cuda.synchronize()
    host = gate.vet(order)
    assert st[:65].tolist() == [v.status for v in host] and int(st[65]) == 9
    assert ss[:65].tolist() == [v.sumsq for v in host] and float(ss[65]) == -1.0
    assert mx[:65].tolist() == [v.max_abs for v in host] and float(mx[65]) == -1.0
    with pytest.raises(ValueError):
        gate.vet_device(order, st, ss, mx[:10])
    with pytest.raises(ValueError):
        gate.vet_device(order, st.to(torch.int64), ss, mx)


def test_a_slot_does_not_depend_on_its_launch(codec, oracle, trios):
    """Several blocks (MNIST: 30 of them): a slot alone, in a burst of 64 at three positions,
    and twice gives the same bits; so do two slots that hold the same upload."""
    lay, ups = MNIST, trios["mnist"]
    with codec.pool(len(ups[0]), lay.header_positions(), BURST) as pool:
        for s in range(BURST):
            pool.put(s, ups[s % 3])
        with pool.gate(lay.header_values()) as gate:
            alone = gate.vet([5])[0]
            agrees(alone, reference(oracle, ups[2]))
            assert gate.vet([5])[0] == alone
            for order in (list(range(BURST)), list(range(BURST - 1, -1, -1)), [7, 5] + [s for s in range(BURST) if s not in (5, 7)]):
                got = gate.vet(order)
                assert got[order.index(5)] == alone
                assert all(got[order.index(s)] == got[order.index(s % 3)] for s in range(BURST))


# 4 ------------------------------------------------------------------ Base64 verdict

@pytest.mark.parametrize("name", ["synthetic7", "synthetic8", "synthetic50003"])
def test_base64_verdict_is_the_folds(codec, oracle, trios, name):
    lay, good = SHAPES[name], trios[name][0]
    L = len(good)
    pads = len(good) - len(good.rstrip(b"="))
    cases = {"first": spoil(good, 3), "middle": spoil(good, (L // 32) * 16 + 5), "last": spoil(good, L - pads - 1),
             "pad_inside": spoil(good, L // 2, b"=")}
    # a position the ragged last group does not need: its '=' characters
    unneeded = {f"unneeded{i}": spoil(good, L - 1 - i) for i in range(pads)}
    assert pads == {7: 2, 8: 1, 50_003: 1}[lay.n_up]
    texts = list(cases.values()) + list(unneeded.values()) + [good]
    with codec.pool(L, lay.header_positions(), len(texts)) as pool, pool.gate(lay.header_values()) as gate:
        for s, u in enumerate(texts):
            pool.put(s, u)
        got = gate.vet(list(range(len(texts))))
        assert all(pool.slot_status(s) == 0 for s in range(len(texts)))  # a vet leaves the pool's status alone
        with pool.gate() as plain:
            bare = plain.vet(list(range(len(texts))))
        good_slot = len(texts) - 1
        for s in range(len(texts)):
            # a single pick's fold compares no header: the gate without codes; beside a good first
            # pick it does, and a bad character inside a header slot then shows as both bits
            assert bare[s].status == fold_status(pool, [s], s), s
            if s != good_slot:
                assert got[s].status == fold_status(pool, [good_slot, s], s), s
        assert [v.status for v in bare] == [1] * len(cases) + [0] * (pads + 1)
        assert [v.status & 1 for v in got] == [1] * len(cases) + [0] * (pads + 1)
        assert got[0].status == 3 and got[1].status == 1  # character 3 lies in the first header slot, the middle one in no header
        for v in got[len(cases):]:
            agrees(v, reference(oracle, good))


# 5 ------------------------------------------------------------------ layout verdict

@pytest.mark.parametrize("name", ["mnist", "dense1025"])
def test_layout_verdict_is_the_folds(codec, oracle, trios, name):
    lay, good = SHAPES[name], trios[name][0]
    hp = lay.header_positions()
    at = [0, len(hp) // 2, len(hp) - 1]
    cands = [A.mismatch_upload(oracle, lay, j, 1) for j in at] + [A.uploads(oracle, lay, 2)[1]]
    codes = oracle.decode_ints(good)[hp]
    assert np.array_equal(F.header_codes(lay.header_values()), codes)  # the expected codes are a good upload's
    with codec.pool(len(good), hp, 5) as pool, pool.gate(lay.header_values()) as gate, pool.gate() as plain:
        pool.put(0, good)
        for s, u in enumerate(cands):
            pool.put(1 + s, u)
        got = gate.vet([1, 2, 3, 4, 0])
        for s in range(1, 5):
            assert got[s - 1].status == fold_status(pool, [0, s], s), s
        assert [v.status for v in got] == [2, 2, 2, 0, 0]
        agrees(got[3], reference(oracle, cands[3]))
        assert [v.status for v in plain.vet([1, 2, 3, 4, 0])] == [0] * 5  # without codes the bit is never set
        # the pool's status is what the last update saw, whatever was vetted since
        assert fold_status(pool, [0, 1], 1) == 2
        gate.vet([4, 0])
        assert pool.slot_status(1) == 2 and pool.slot_status(4) == 0
        with pytest.raises(F.FleetError):
            pool.gate(lay.header_values()[:-1])  # one code per header of the pool


# 6 -------------------------------------------------------------------------- Gate.put

def test_put_keeps_a_good_upload_and_refuses_the_rest(codec, oracle, trios):
    lay = MNIST
    ups = A.uploads(oracle, lay, 3)
    d = [1.0, 1 / 3, 0.25]
    with codec.pool(len(ups[0]), lay.header_positions(), 4) as pool, pool.gate(lay.header_values()) as gate:
        pool.put(0, ups[0])
        pool.put(1, ups[1])
        before = pool.update([1, 0], d[:2])
        v = gate.put(2, spoil(ups[2], 1000))
        assert v.status == 1 and not pool.occupied(2)
        v = gate.put(2, A.mismatch_upload(oracle, lay, 4, 2))
        assert v.status == 2 and not pool.occupied(2) and v.sumsq > 0
        assert pool.free_slot() == 2 and pool.update([1, 0], d[:2]) == before
        with pytest.raises(F.FleetError):
            pool.update([2], [1.0])  # nothing is there to pick
        with pytest.raises(F.FleetError) as ei:
            gate.put(0, ups[2])  # an occupied slot
        assert ei.value.code == F.FLEET_ERR_ARG and pool.update([1, 0], d[:2]) == before
        with pytest.raises(F.FleetError):
            gate.put(2, ups[2][:-16])  # another length
        v = gate.put(2, ups[2])
        agrees(v, reference(oracle, ups[2]))
        assert pool.occupied(2)
        assert pool.update([2, 0, 1], d) == codec.update([ups[2], ups[0], ups[1]], d)
        assert all(pool.slot_status(s) == 0 for s in range(4))


# 7 ------------------------------------------------------------------ argument errors

def test_argument_errors_launch_nothing(codec, pool65):
    _, _, ups = pool65
    lay = synthetic(50)
    L = F.lib()
    with codec.pool(len(ups[0]), lay.header_positions(), 4) as pool, pool.gate(lay.header_values()) as gate:
        pool.put(0, ups[0])
        pool.put(1, ups[1])
        st, ss, mx = np.full(4, 77, np.int32), np.full(4, 7.0), np.full(4, 5.0, np.float32)
        out = (st.ctypes.data, ss.ctypes.data, mx.ctypes.data)
        for slots in ([0, 9], [-1, 0], [0, 3], [0, 1, 0]):  # outside, outside, unoccupied, twice
            sl = np.array(slots, np.int32)
            assert L.fleet_gate_vet(gate._h, sl.ctypes.data, len(sl), *out) == F.FLEET_ERR_ARG, slots
            with pytest.raises(F.FleetError):
                gate.vet(slots)
        sl = np.array([0, 1], np.int32)
        for K in (0, -3):
            assert L.fleet_gate_vet(gate._h, sl.ctypes.data, K, *out) == F.FLEET_ERR_ARG
        assert L.fleet_gate_vet(gate._h, sl.ctypes.data, 2, None, ss.ctypes.data, mx.ctypes.data) == F.FLEET_ERR_ARG
        assert (st == 77).all() and (ss == 7.0).all() and (mx == 5.0).all()  # the outputs keep their sentinel
        with pytest.raises(F.FleetError):
            gate.vet([])
        assert [v.status for v in gate.vet([1, 0])] == [0, 0]
        gate.close()
        with pytest.raises(ValueError):
            gate.vet([0])  # a closed gate


# 8 ----------------------------------------------------------------------- end to end

def test_updater_refuses_at_the_door(codec, oracle):
    """A session with one malformed and one wrong-header arrival among good ones, through
    FleetUpdater(picker, vet=True, model=ResidentModel): the merged bytes and the model text
    of the same session without the two."""
    import os
    from fleet_amd.updater import FleetUpdater
    s = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "session_mnist.npz"))
    lay, lrates = MNIST, [0.05, 0.02, 0.01]
    good = A.uploads(oracle, lay, 6)
    bad = {2: spoil(good[2], 777), 4: A.mismatch_upload(oracle, lay, len(lay.header_positions()) - 1, 4)}
    arrivals = [(0, good[0]), (1, good[1]), (90, bad[2]), (2, good[2]), (3, good[3]), (91, bad[4]), (4, good[4]),
                (5, good[5])]
    fifo = lambda pending, epoch: (list(range(3)), [])
    out, models = [], []
    for vet in (True, False):
        rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1, max_versions=3)
        u = FleetUpdater(codec, lay, 3, lrates, None, None, policy=1, stale_size=2, picker=fifo, model=rm, vet=vet,
                         pool_slots=4)
        got = []
        for cid, text in arrivals:
            if not vet and cid >= 90:
                continue
            r = u.update(text, [cid % 10] * 10, u.curr_epoch, client_id=cid)
            if cid >= 90:
                assert r is None
            got.append(r)
        if vet:
            assert [(c, st) for c, st, _ in u.refused] == [(90, 1), (91, 2)]
            got = [r for r, (cid, _) in zip(got, arrivals) if cid < 90]
        else:
            assert u.refused == []
        assert [r is not None for r in got] == [False, False, True, False, False, True] and u.curr_epoch == 2
        assert u.acc == []
        out.append(got)
        models.append((rm.getModelParametersNative(rm.modelsSize() - 1), rm.export(-1)))
        if vet:
            u._gate.close()
        u._pool.close()
        rm.close()
    assert out[0] == out[1]
    assert models[0][0] == models[1][0]
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(models[0][1], models[1][1]))
    assert out[0][2] == codec.update(good[:3], [1.0, 1.0, 1.0])
