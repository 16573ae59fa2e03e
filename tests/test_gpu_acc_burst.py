"""Bursts of the streaming aggregation (Accumulator.push_many / push_finish and their
device forms, k_acc_push_many): K uploads folded by one kernel per ACC_BURST of them, the
completing burst also writing the merged gradient. Whatever way a batch is cut into
pushes and bursts, the bytes are the reference's chain over its uploads
(CppNNUpdater.java:383-391, 420-421, 463-464, 490-508). Every expected value is the
oracle's (the faithful per-op chain or the fused restatement) or a recorded fixture."""
import ctypes as C
import functools
import glob
import math
import os

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import MNIST, synthetic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the recorded chains that store their uploads
CHAINS = sorted(os.path.basename(p)[6:-4] for p in glob.glob(os.path.join(GOLDEN, "chain_*.npz"))
                if "uploads" in np.load(p).files)
EDGE = np.array([1e8, -1e8, 99999999.0, 999999999.0, 1e9, -1e9, 2.1e9, 3e9, -3e9, 9.99999e8,
                 float("inf"), float("-inf"), float("nan"), 1e-45, -1e-45, 1.1754942e-38, 3.4e38], np.float32)


def uploads_for(oracle, layout, M, seed):
    return [oracle.encode_floats(oracle.synth_upload(seed, c, list(layout.w_sizes), list(layout.b_sizes)))
            for c in range(M)]


def policy(name, M):
    if name == "inverse":  # 1/3 is no binary32 value: the f64 multiply
        return [1 / ((c % 3) + 1) for c in range(M)]
    if name == "exp":
        return [math.exp(-0.5 * min(c, 4)) for c in range(M)]
    raise KeyError(name)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def both_ways(codec, lay, ups, d, exp, oracle):
    """The whole batch as one push_finish, and as one push_many closed by finish."""
    exp32 = oracle.decode_floats(exp)
    with codec.accumulator(len(ups[0]), lay.header_positions()) as acc:
        merged, f32 = acc.push_finish(ups, d, want_f32=True)
        assert acc.count == 0
        assert merged == exp and same_bits(f32, exp32)
        acc.push_many(ups, d)
        assert acc.count == len(ups)
        merged, f32 = acc.finish(want_f32=True)
        assert merged == exp and same_bits(f32, exp32)


# 1 -------------------------------------------------------------------- partitions

@functools.lru_cache(maxsize=None)
def _partition_case(oracle, n_up, pol):
    lay = synthetic(n_up)
    ups = uploads_for(oracle, lay, 7, seed=300 + n_up)
    d = policy(pol, 7)
    exp = oracle.update_faithful(ups, d)
    return lay, ups, d, exp, oracle.decode_floats(exp)


@pytest.mark.parametrize("close", ["push_finish", "finish"])
@pytest.mark.parametrize("parts", [[7], [1, 6], [6, 1], [3, 4], [2, 2, 3], [1] * 7], ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("pol", ["exp", "inverse"])
@pytest.mark.parametrize("n_up", [3, 4, 5, 7, 100, 771])
def test_partitions(codec, oracle, n_up, pol, parts, close):
    """One partial group (3, 4, 5), an empty weight block, 257 groups = two blocks (771).
    close = "push_finish": single arrivals go through push, the last part through
    push_finish; "finish": every part, single ones too, through push_many, then finish."""
    lay, ups, d, exp, exp32 = _partition_case(oracle, n_up, pol)
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
            assert acc.count == 7
            merged, f32 = acc.finish(want_f32=True)
        assert acc.count == 0
    assert merged == exp
    assert same_bits(f32, exp32)


# 2 ------------------------------------------------------------- launch-chunk edges

@functools.lru_cache(maxsize=None)
def _chunk_uploads(oracle, M):
    lay = synthetic(50)
    return lay, uploads_for(oracle, lay, M, seed=77)


@pytest.mark.parametrize("dk", ["B-1", "B", "B+1", "2B+1"])
def test_launch_chunk_edges(codec, oracle, dk):
    """A burst longer than ACC_BURST runs as consecutive launches, the later ones on the
    spare state in place; every client has a factor of its own, so a factor taken from
    the wrong slot of a launch's block shows."""
    B = F.ACC_BURST
    K = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1}[dk]
    lay, pool = _chunk_uploads(oracle, 2 * B + 1)
    ups = pool[:K]
    d = [1 / (1 + 0.37 * c) for c in range(K)]
    assert len(set(d)) == K
    both_ways(codec, lay, ups, d, oracle.update_faithful(ups, d), oracle)


# 3 ---------------------------------------------------------------- recorded chains

@pytest.mark.parametrize("name", CHAINS)
def test_recorded_chains(codec, name):
    z = np.load(os.path.join(GOLDEN, f"chain_{name}.npz"))
    lens = z["upload_lens"]
    ups = [z["uploads"][c, : lens[c]].tobytes() for c in range(int(z["M"]))]
    lay = F.Layout(name, tuple(int(s) for s in z["w_sizes"]), tuple(int(s) for s in z["b_sizes"]))
    with codec.accumulator(len(ups[0]), lay.header_positions()) as acc:
        assert acc.push_finish(ups, [float(x) for x in z["dampen"]]) == z["merged"].tobytes()


def test_recorded_chains_are_found():
    assert len(CHAINS) >= 5 and "synth_m3_exp" in CHAINS


# 4 ------------------------------------------------------------------- grid stride

def test_grid_stride(codec, oracle):
    """More groups than the grid has lanes (8 blocks of 256 per CU): the blocks stride, and
    the last pass is a partial one."""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_up = 3 * (8 * 256 * cus + 300) + 1
    lay = synthetic(n_up)
    assert (n_up + 2) // 3 > 8 * 256 * cus
    ups = uploads_for(oracle, lay, 3, seed=41)
    d = policy("inverse", 3)
    hm = oracle.header_mask(list(lay.w_sizes), list(lay.b_sizes))
    with codec.accumulator(len(ups[0]), lay.header_positions()) as acc:
        assert acc.push_finish(ups, d) == oracle.update_fused(ups, d, hm)


# 5 ------------------------------------------------------------------ out of domain

def edge_uploads(oracle, lay, M, seed, at):
    """Gradient-like payloads; the edge values (|x| >= 1e8, >= 1e9, +-inf, NaN, denormals)
    appear in upload `at` alone."""
    rng = np.random.default_rng(seed)
    n = lay.n_up - 3
    ups = []
    for c in range(M):
        v = oracle.synth_upload(seed, c, list(lay.w_sizes), list(lay.b_sizes))
        p = rng.normal(0, 1e-2, n).astype(np.float32)
        if c == at:
            k = max(2, n // 10)
            p[rng.integers(0, n, k)] = rng.choice(EDGE, k)
        v[2:lay.n_up - 1] = p
        ups.append(oracle.encode_floats(v))
    return ups


@pytest.mark.parametrize("at", [0, 2, 4], ids=["first", "middle", "last"])
@pytest.mark.parametrize("n_up", [159, 1001])
def test_out_of_domain_in_one_upload(codec, oracle, n_up, at):
    """A step inside a burst has the running value and its own row only, as a single push
    has: a value outside the table stages' domain takes the general codec inside the step."""
    lay = synthetic(n_up)
    ups = edge_uploads(oracle, lay, 5, 5000 + n_up + at, at)
    d = [1 / 3, math.exp(-0.7), 7.25e3, 1.0, 1 / 3]
    both_ways(codec, lay, ups, d, oracle.update_faithful(ups, d), oracle)


def test_running_sum_leaves_the_domain_mid_burst(codec, oracle):
    """Every upload is inside the table domain, their sum is not: 6e7 three times in the
    same slots passes 1e8 at the second step of the burst."""
    lay = synthetic(159)
    rng = np.random.default_rng(8)
    slots = rng.choice(np.arange(2, lay.n_up - 1), 12, replace=False)
    ups = []
    for c in range(5):
        v = oracle.synth_upload(58, c, list(lay.w_sizes), list(lay.b_sizes))
        if c in (1, 2, 3):
            v[slots] = 6e7
            v[slots[:4]] = -6e7
        ups.append(oracle.encode_floats(v))
    d = [1.0, 1.0, 1.0, 1.0, 0.5]
    both_ways(codec, lay, ups, d, oracle.update_faithful(ups, d), oracle)


# 6 ---------------------------------------------------------------- all or nothing

@functools.lru_cache(maxsize=None)
def _txn_case(oracle):
    lay = synthetic(1001)
    good = uploads_for(oracle, lay, 6, seed=66)

    def with_header(c, value):
        v = oracle.synth_upload(66, c, list(lay.w_sizes), list(lay.b_sizes))
        v[0] = value
        return oracle.encode_floats(v)
    return lay, good, with_header


def spoil(kind, row, with_header, c):
    if kind == "base64":
        return row[:40] + b"*" + row[41:]
    out = with_header(c, 2.0)  # a differing header code
    assert len(out) == len(row) and out != row
    return out


@pytest.mark.parametrize("call", ["push_many", "push_finish"])
@pytest.mark.parametrize("pos", [0, 1, 2], ids=["first", "middle", "last"])
@pytest.mark.parametrize("kind", ["base64", "layout"])
def test_rejected_burst_leaves_no_trace(codec, oracle, kind, pos, call):
    lay, good, with_header = _txn_case(oracle)
    d = [1.0, 1 / 3, 0.5, math.exp(-0.7), 0.25, 1 / 7]
    exc, code = (F.Base64Error, F.FLEET_ERR_BASE64) if kind == "base64" else (F.LayoutError, F.FLEET_ERR_LAYOUT)
    burst = list(good[2:5])
    burst[pos] = spoil(kind, burst[pos], with_header, 2 + pos)
    with codec.accumulator(len(good[0]), lay.header_positions()) as acc:
        acc.push_many(good[:2], d[:2])
        with pytest.raises(exc) as ei:
            getattr(acc, call)(burst, d[2:5])
        assert ei.value.code == code and acc.count == 2
        # a good retry: the chain over the accepted uploads and exactly those
        if call == "push_finish":
            merged, f32 = acc.push_finish(good[2:5], d[2:5], want_f32=True)
        else:
            acc.push_many(good[2:5], d[2:5])
            assert acc.count == 5
            merged, f32 = acc.finish(want_f32=True)
        assert acc.count == 0
    exp = oracle.update_faithful(good[:5], d[:5])
    assert merged == exp
    assert same_bits(f32, oracle.decode_floats(exp))


@pytest.mark.parametrize("call", ["push_many", "push_finish"])
def test_rejected_first_burst_does_not_fix_the_header(codec, oracle, call):
    """A rejected first burst leaves the count at 0, so the next burst is the batch's
    first again and brings its own header codes; inside a first burst upload 0 defines
    them."""
    lay, good, with_header = _txn_case(oracle)
    d = [1.0, 1 / 3, 0.5]
    other = [with_header(c, 2.0) for c in range(3)]
    with codec.accumulator(len(good[0]), lay.header_positions()) as acc:
        with pytest.raises(F.Base64Error):
            getattr(acc, call)([good[0], spoil("base64", good[1], with_header, 1), good[2]], d)
        assert acc.count == 0
        with pytest.raises(F.LayoutError):  # uploads 0 and 1 of the batch's first burst differ
            getattr(acc, call)([good[0], other[1], good[2]], d)
        assert acc.count == 0
        with pytest.raises(F.LayoutError):
            getattr(acc, call)([other[0], good[1]], d[:2])
        assert acc.count == 0
        if call == "push_finish":
            merged = acc.push_finish(other, d)
        else:
            acc.push_many(other, d)
            merged = acc.finish()
    # (the accumulator's header slots are those of its creation; the faithful chain would
    # walk the layout the altered header describes, so the fused restatement with the mask)
    hm = oracle.header_mask(list(lay.w_sizes), list(lay.b_sizes))
    assert merged == oracle.update_fused(other, d, hm)


def test_argument_errors_change_nothing(codec, oracle):
    lay, good, _ = _txn_case(oracle)
    d = [1.0, 0.5, 0.25]
    with codec.accumulator(len(good[0]), lay.header_positions()) as acc:
        acc.push(good[0], d[0])
        for call in (acc.push_many, acc.push_finish):
            with pytest.raises(F.FleetError) as ei:
                call([good[1], good[2][:-4]], d[1:])  # a ragged burst
            assert ei.value.code == F.FLEET_ERR_ARG and acc.count == 1
            with pytest.raises(ValueError):
                call([good[1], good[2]], d[:1])
            with pytest.raises(ValueError):
                call([], [])
        L = F.lib()
        rows = (C.c_char_p * 2)(good[1], None)
        lens = np.array([len(good[1])] * 2, np.uint64)
        dd = np.array(d[1:], np.float64)
        assert L.fleet_acc_push_many(acc._h, rows, lens.ctypes.data, 2, dd.ctypes.data) == F.FLEET_ERR_ARG  # NULL entry
        assert L.fleet_acc_push_many(acc._h, rows, lens.ctypes.data, 1, None) == F.FLEET_ERR_ARG
        assert L.fleet_acc_push_many(acc._h, rows, lens.ctypes.data, 0, dd.ctypes.data) == F.FLEET_ERR_ARG
        assert acc.count == 1
        assert acc.push_finish(good[1:3], d[1:]) == oracle.update_faithful(good[:3], d)


# 7 ----------------------------------------------------------------------- windows

@pytest.mark.parametrize("cuts", [(0, 150), (0, 0, 100), (0, 1, 333), (0, 200, 334)], ids=str)
def test_windows(codec, oracle, cuts):
    """Accumulators over disjoint group windows of one upload, fed the same bursts, write
    disjoint parts of the merged buffers; a zero-group window writes nothing."""
    lay, good, _ = _txn_case(oracle)
    ups, d = good[:5], policy("inverse", 5)
    L = len(ups[0])
    G = (F.b64_count(L) + 2) // 3
    hp = lay.header_positions()
    exp = oracle.update_faithful(ups, d)
    exp_f32 = oracle.decode_floats(exp)
    merged = np.zeros(L + 16, np.uint8)
    f32 = np.zeros(F.b64_count(L) + 1, np.float32)
    edges = list(cuts) + [G]  # (0, 0, 100) and (0, 200, 334) hold a zero-group window
    for gb, ge in zip(edges, edges[1:]):
        with codec.accumulator(L, hp, gb, ge) as acc:
            acc.push_many(ups[:2], d[:2])
            assert acc.count == 2
            m, v = acc.push_finish(ups[2:], d[2:], want_f32=True)
            assert acc.count == 0
        b0, b1 = 16 * gb, min(L, 16 * ge)
        m = np.frombuffer(m, np.uint8)
        assert not m[:b0].any() and not m[b1:].any()  # only the window is written
        merged[b0:b1] = m[b0:b1]
        v0, v1 = 3 * gb, min(len(v), 3 * ge)
        assert not v[:v0].any() and not v[v1:].any()
        f32[v0:v1] = v[v0:v1]
    assert merged[:L].tobytes() == exp
    assert same_bits(f32[: len(exp_f32)], exp_f32)


# 8 ------------------------------------------------------------------ device forms

def test_device_forms(codec, oracle):
    """Rows read in place from a [K, pitch] tensor whose pitch exceeds the padded upload
    (the bytes past an upload's end are not Base64), on a stream of its own; the tensor is
    overwritten once that stream is through with it."""
    torch = pytest.importorskip("torch")
    lay = synthetic(1000)
    M = 5
    ups = uploads_for(oracle, lay, M, seed=81)
    d = policy("exp", M)
    L = len(ups[0])
    assert L % 16 != 0
    G = (L + 15) // 16
    pitch = 16 * G + 32
    host = np.full((M, pitch), ord("*"), np.uint8)
    for c, u in enumerate(ups):
        host[c, :L] = np.frombuffer(u, np.uint8)
    hp = lay.header_positions()
    exp = oracle.update_faithful(ups, d)
    exp32 = oracle.decode_floats(exp)
    s = torch.cuda.Stream()
    merged = torch.zeros(16 * G, dtype=torch.uint8, device="cuda")
    f32 = torch.zeros(3 * G, dtype=torch.float32, device="cuda")

    def check(exp, exp32):
        torch.cuda.synchronize()
        assert merged.cpu().numpy()[:L].tobytes() == exp
        assert same_bits(f32.cpu().numpy()[: lay.n_up], exp32)
        merged.zero_()
        f32.zero_()
        torch.cuda.synchronize()

    with codec.accumulator(L, hp) as acc:
        # push_many_device in two bursts, then finish_device
        dev = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        acc.push_many_device(dev[:2], d[:2], stream=s.cuda_stream)
        acc.push_many_device(dev[2:], d[2:], stream=s.cuda_stream)
        assert acc.count == M
        s.synchronize()
        dev.fill_(ord("!"))  # the accumulator keeps its own copy of the last row
        torch.cuda.synchronize()
        acc.finish_device(merged, f32, stream=s.cuda_stream)
        assert acc.count == 0
        check(exp, exp32)
        # push_finish_device alone, and after a device burst
        dev = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        acc.push_finish_device(dev, d, merged, f32, stream=s.cuda_stream)
        assert acc.count == 0
        check(exp, exp32)
        acc.push_many_device(dev[:3], d[:3], stream=s.cuda_stream)
        acc.push_finish_device(dev[3:], d[3:], merged, f32, stream=s.cuda_stream)
        assert acc.count == 0
        dev.fill_(ord("!"))
        check(exp, exp32)
        # a bad row in push_finish_device: the accumulator is as before the call
        bad = host.copy()
        bad[3, 333] = ord("*")
        dbad = torch.from_numpy(bad).cuda()
        dev = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        acc.push_many_device(dev[:2], d[:2], stream=s.cuda_stream)
        with pytest.raises(F.Base64Error) as ei:
            acc.push_finish_device(dbad[2:], d[2:], merged, f32, stream=s.cuda_stream)
        assert ei.value.code == F.FLEET_ERR_BASE64 and acc.count == 2
        merged.zero_()
        f32.zero_()
        torch.cuda.synchronize()
        acc.push_finish_device(dev[2:], d[2:], merged, f32, stream=s.cuda_stream)
        assert acc.count == 0
        check(exp, exp32)
        # a bad row in push_many_device is sticky until reset, and comes before a later
        # burst's own verdict
        acc.push_many_device(dev[:1], d[:1], stream=s.cuda_stream)
        acc.push_many_device(dbad[1:4], d[1:4], stream=s.cuda_stream)
        assert acc.count == 4
        with pytest.raises(F.Base64Error):
            acc.push_finish_device(dev[4:], d[4:], merged, f32, stream=s.cuda_stream)
        for call in (lambda: acc.push_many_device(dev[4:], d[4:], stream=s.cuda_stream),
                     lambda: acc.push_many(ups[4:], d[4:]), lambda: acc.push_finish(ups[4:], d[4:]),
                     lambda: acc.finish_device(merged, f32, stream=s.cuda_stream)):
            with pytest.raises(F.Base64Error):
                call()
        acc.reset()
        assert acc.count == 0
        merged.zero_()
        f32.zero_()
        torch.cuda.synchronize()
        # rows that cannot be read in place are refused before anything runs
        with pytest.raises(F.FleetError) as ei:
            acc.push_many_device(dev[:, 1:], d, stream=s.cuda_stream)
        assert ei.value.code == F.FLEET_ERR_ARG and acc.count == 0
        acc.push_many_device(dev[:4], d[:4], stream=s.cuda_stream)
        assert acc.push_finish(ups[4:], d[4:]) == exp  # host and device forms mix
        acc.push_finish_device(dev[:3], d[:3], merged, f32, stream=s.cuda_stream)
        e3 = oracle.update_faithful(ups[:3], d[:3])
        check(e3, oracle.decode_floats(e3))


# 9 ------------------------------------------------------------------------- reuse

def test_reuse(codec, oracle):
    lay, ups, _ = _txn_case(oracle)
    with codec.accumulator(len(ups[0]), lay.header_positions()) as acc:
        for M in (4, 6, 1):  # batches of different M through one accumulator, the staging kept
            d = policy("exp", M)
            assert acc.push_finish(ups[:M], d) == oracle.update_faithful(ups[:M], d)
            assert acc.count == 0
        with pytest.raises(F.FleetError) as ei:
            acc.finish()
        assert ei.value.code == F.FLEET_ERR_ARG
        acc.push_many(ups[4:6], [0.25, 0.5])  # a half-filled batch, dropped
        acc.reset()
        assert acc.count == 0
        assert acc.push_finish([ups[1], ups[0]], [1 / 3, 1.0]) == oracle.update_faithful([ups[1], ups[0]], [1 / 3, 1.0])


# 11 ---------------------------------------------------------------------- updater

def test_updater_update_many_equals_batch_update(codec, oracle):
    from fleet_amd.updater import FleetUpdater
    lay = MNIST
    rng = np.random.default_rng(9)
    w0 = rng.normal(0, 0.05, lay.n_weights).astype(np.float32)
    b0 = rng.normal(0, 0.05, lay.n_fc_bias).astype(np.float32)
    mk = lambda s: FleetUpdater(codec, lay, 4, [0.05, 0.02, 0.01], w0, b0, policy=4, alpha=0.3, has_outlier=True,
                                streaming=s)
    a, b = mk(True), mk(False)
    ups = uploads_for(oracle, lay, 8, seed=91)
    arrivals = []
    for i, u in enumerate(ups):
        labels = [int(x) for x in rng.integers(0, 30, 10)]
        if i % 5 == 0:
            labels = [0] * 9 + [40]
        arrivals.append((u, labels, max(0, i // 4 - i % 3), i))
    want = [b.update(*x) for x in arrivals]
    got = a.update_many(arrivals[:3]) + a.update_many(arrivals[3:])  # the second call crosses a batch boundary
    assert got == want and [w is not None for w in want] == [False, False, False, True] * 2
    assert same_bits(a.weights, b.weights) and same_bits(a.fc_bias, b.fc_bias)
    assert a.curr_epoch == b.curr_epoch == 2 and a.global_labels == b.global_labels and a.lr == b.lr
    assert len(a.acc) == len(b.acc) == 0
