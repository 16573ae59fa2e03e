"""Streaming aggregation (fleet_acc: Codec.accumulator, k_acc_push / k_acc_finish): every
upload folded into the resident sum when it arrives gives, at the finish, the bytes the
reference's chain over the same uploads gives (CppNNUpdater.java:383-391, 420-421,
463-464, 490-508). Every expected value is the oracle's (the faithful per-op chain or
the fused restatement) or a recorded fixture; the batch GPU path appears only beside
them."""
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
CHAINS = ["small_layout_m8_inverse", "plumbing_m1_avg", "synth_m3_exp", "synth_m5_classaware", "partial_group_n2"]
EDGE = np.array([1e8, -1e8, 99999999.0, 999999999.0, 1e9, -1e9, 2.1e9, 3e9, -3e9, 9.99999e8,
                 float("inf"), float("-inf"), float("nan"), 1e-45, -1e-45, 1.1754942e-38, 3.4e38], np.float32)
OUT_OF_DOMAIN = np.array([1e9, -2.1e9, float("inf"), float("nan"), 3e9], np.float32)


def uploads_for(oracle, layout, M, seed):
    return [oracle.encode_floats(oracle.synth_upload(seed, c, list(layout.w_sizes), list(layout.b_sizes)))
            for c in range(M)]


def policy(name, M):
    if name == "avg":
        return [1.0] * M
    if name == "inverse":
        return [1 / ((c % 3) + 1) for c in range(M)]
    if name == "exp":
        return [math.exp(-0.5 * min(c, 4)) for c in range(M)]
    raise KeyError(name)


def stream(codec, layout, ups, d, want_f32=False):
    with codec.accumulator(len(ups[0]), layout.header_positions()) as acc:
        for i, (u, f) in enumerate(zip(ups, d)):
            assert acc.count == i
            acc.push(u, f)
        assert acc.count == len(ups)
        out = acc.finish(want_f32=want_f32)
        assert acc.count == 0
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# 1 ---------------------------------------------------------------- recorded chains

@pytest.mark.parametrize("name", CHAINS)
def test_recorded_chains(codec, name):
    z = np.load(os.path.join(GOLDEN, f"chain_{name}.npz"))
    assert f"chain_{name}.npz" in [os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "chain_*.npz"))]
    lens = z["upload_lens"]
    ups = [z["uploads"][c, : lens[c]].tobytes() for c in range(int(z["M"]))]
    lay = F.Layout(name, tuple(int(s) for s in z["w_sizes"]), tuple(int(s) for s in z["b_sizes"]))
    assert stream(codec, lay, ups, [float(x) for x in z["dampen"]]) == z["merged"].tobytes()


# 2 ------------------------------------------------------------------ tiny layouts

@pytest.mark.parametrize("n_up", [3, 4, 5, 6, 7])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_tiny_layouts(codec, oracle, n_up, M):
    """One partial group, an empty weight block, and M = 1, where the first push is the whole chain."""
    lay = synthetic(n_up)
    ups = uploads_for(oracle, lay, M, seed=n_up * 10 + M)
    d = policy("exp", M)
    merged, f32 = stream(codec, lay, ups, d, want_f32=True)
    exp = oracle.update_faithful(ups, d)
    assert merged == exp
    assert same_bits(f32, oracle.decode_floats(exp))


# 3 ------------------------------------------------- multi-block and ragged tail

@pytest.fixture(scope="module")
def mnist8(oracle):
    return uploads_for(oracle, MNIST, 8, seed=108)


@pytest.mark.parametrize("pol", ["avg", "inverse", "exp"])
def test_mnist_vs_faithful_chain(codec, oracle, mnist8, pol):
    d = policy(pol, 8)
    merged, f32 = stream(codec, MNIST, mnist8, d, want_f32=True)
    exp = oracle.update_faithful(mnist8, d)
    assert merged == exp
    assert same_bits(f32, oracle.decode_floats(exp))


@pytest.mark.parametrize("n_up,M", [(100000, 9), (99998, 5)])
def test_multi_block_vs_fused_oracle(codec, oracle, n_up, M):
    lay = synthetic(n_up)
    ups = uploads_for(oracle, lay, M, seed=7)
    d = policy("inverse", M)
    hm = oracle.header_mask(list(lay.w_sizes), list(lay.b_sizes))
    assert stream(codec, lay, ups, d) == oracle.update_fused(ups, d, hm)


# 4 ------------------------------------------------------- out-of-domain payloads

def edge_uploads(oracle, lay, M, seed, where):
    """Gradient-like payloads. where = "mixed": edge values (|x| >= 1e8, >= 1e9, +-inf, NaN,
    denormals) sprinkled into every upload; "first" / "last": the values that leave the
    codec's table domain appear in that upload alone, the others stay gradient-like."""
    rng = np.random.default_rng(seed)
    n = lay.n_up - 3
    ups = []
    for c in range(M):
        v = oracle.synth_upload(seed, c, list(lay.w_sizes), list(lay.b_sizes))
        p = rng.normal(0, 1e-2, n).astype(np.float32)
        k = max(2, n // 40)
        if where == "mixed":
            p[rng.integers(0, n, k)] = rng.choice(EDGE, k)
        elif (where == "first" and c == 0) or (where == "last" and c == M - 1):
            p[rng.integers(0, n, k)] = rng.choice(OUT_OF_DOMAIN, k)
        v[2:lay.n_up - 1] = p
        ups.append(oracle.encode_floats(v))
    return ups


@pytest.mark.parametrize("where", ["mixed", "first", "last"])
@pytest.mark.parametrize("M", [2, 5])
@pytest.mark.parametrize("n_up", [159, 1001])
def test_out_of_domain_payloads(codec, oracle, n_up, M, where):
    """The fold-specific risk: a step has only this upload and the previous state, so a
    value outside the table stages' domain must take the general codec inside the step
    (the batch kernels recompute the lane's chain from all M uploads instead). Dampening
    factors that are no binary32 values take the f64 multiply."""
    lay = synthetic(n_up)
    ups = edge_uploads(oracle, lay, M, 4000 + n_up + 10 * M, where)
    d = [[1 / 3, math.exp(-0.7), 7.25e3, 1.0, 1 / 3][c] for c in range(M)]
    merged, f32 = stream(codec, lay, ups, d, want_f32=True)
    exp = oracle.update_faithful(ups, d)
    assert merged == exp
    assert same_bits(f32, oracle.decode_floats(exp))


# 5 ------------------------------------------------------------ transactional push

def test_transactional_push(codec, oracle):
    """Malformed uploads raise at their push and leave count, state and the last accepted
    upload untouched: the result is the oracle's chain over the accepted uploads only,
    its keep slots (the layout header) from the last accepted one. A '*' row arrives
    first, an '=' row and a truncated row mid-batch, a row whose first header float
    differs mid-batch and after the last good one, a '*' row after it too. (A differing
    header cannot be told from the first upload of a batch: it defines the batch's.)"""
    lay = synthetic(1001)
    good = uploads_for(oracle, lay, 4, seed=51)
    d = [1.0, 1 / 3, 0.5, math.exp(-0.7)]
    g = good[1]
    star = g[:40] + b"*" + g[41:]
    eq = g[:100] + b"=" + g[101:]
    trunc = g[:-4]
    v = oracle.synth_upload(51, 1, list(lay.w_sizes), list(lay.b_sizes))
    v[0] = 2.0
    hdr = oracle.encode_floats(v)
    assert len(hdr) == len(g)
    with codec.accumulator(len(g), lay.header_positions()) as acc:
        def rejected(row, exc, code):
            before = acc.count
            with pytest.raises(exc) as ei:
                acc.push(row, 0.75)
            assert ei.value.code == code and acc.count == before
        rejected(star, F.Base64Error, F.FLEET_ERR_BASE64)  # first
        acc.push(good[0], d[0])
        rejected(eq, F.Base64Error, F.FLEET_ERR_BASE64)
        rejected(hdr, F.LayoutError, F.FLEET_ERR_LAYOUT)
        acc.push(good[1], d[1])
        rejected(trunc, F.FleetError, F.FLEET_ERR_ARG)
        acc.push(good[2], d[2])
        rejected(star, F.Base64Error, F.FLEET_ERR_BASE64)
        acc.push(good[3], d[3])
        rejected(hdr, F.LayoutError, F.FLEET_ERR_LAYOUT)  # after the last good one
        rejected(star, F.Base64Error, F.FLEET_ERR_BASE64)
        assert acc.count == 4
        merged, f32 = acc.finish(want_f32=True)
    exp = oracle.update_faithful(good, d)
    assert merged == exp
    assert same_bits(f32, oracle.decode_floats(exp))


# 6 ----------------------------------------------------------------------- reuse

def test_reuse(codec, oracle):
    lay = synthetic(1000)
    ups = uploads_for(oracle, lay, 5, seed=61)
    with codec.accumulator(len(ups[0]), lay.header_positions()) as acc:
        with pytest.raises(F.FleetError) as ei:
            acc.finish()
        assert ei.value.code == F.FLEET_ERR_ARG
        for M in (3, 5):  # two batches of different M through one accumulator
            d = policy("exp", M)
            for u, f in zip(ups[:M], d):
                acc.push(u, f)
            assert acc.finish() == oracle.update_faithful(ups[:M], d)
        acc.push(ups[4], 0.25)  # a half-filled batch, dropped
        acc.push(ups[3], 0.5)
        assert acc.count == 2
        acc.reset()
        assert acc.count == 0
        with pytest.raises(F.FleetError):
            acc.finish()
        acc.push(ups[1], 1 / 3)
        acc.push(ups[0], 1.0)
        assert acc.finish() == oracle.update_faithful([ups[1], ups[0]], [1 / 3, 1.0])


# 7 --------------------------------------------------------------------- windows

def test_windows(codec, oracle):
    """Two accumulators over [0, k) and [k, G) write disjoint parts of one merged buffer:
    k in the middle of a header run of MNIST's layout (the adjacent header slots 21455 |
    21456 and 22241 | 22242 fall on the two sides of a group boundary), and k = 1."""
    lay = MNIST
    M = 3
    ups = uploads_for(oracle, lay, M, seed=71)
    d = policy("inverse", M)
    L = len(ups[0])
    G = (F.b64_count(L) + 2) // 3
    hp = lay.header_positions()
    ks = (7152, 7414, 1)
    assert all(3 * k - 1 in hp and 3 * k in hp for k in ks[:2])
    exp = oracle.update_faithful(ups, d)
    exp_f32 = oracle.decode_floats(exp)
    for k in ks:
        merged = np.zeros(L + 16, np.uint8)
        f32 = np.zeros(F.b64_count(L) + 1, np.float32)
        for gb, ge in ((0, k), (k, G)):
            with codec.accumulator(L, hp, gb, ge) as acc:
                for u, f in zip(ups, d):
                    acc.push(u, f)
                m, v = acc.finish(want_f32=True)
            b0, b1 = 16 * gb, min(L, 16 * ge)
            m = np.frombuffer(m, np.uint8)
            assert not m[:b0].any() and not m[b1:].any()  # only the window is written
            merged[b0:b1] = m[b0:b1]
            v0, v1 = 3 * gb, min(len(v), 3 * ge)
            assert not v[:v0].any() and not v[v1:].any()
            f32[v0:v1] = v[v0:v1]
        assert merged[:L].tobytes() == exp, k
        assert same_bits(f32[: len(exp_f32)], exp_f32), k


# 8 ----------------------------------------------------------------- device path

def test_device_path(codec, oracle):
    torch = pytest.importorskip("torch")
    lay = synthetic(99998)
    M = 5
    ups = uploads_for(oracle, lay, M, seed=81)
    d = policy("exp", M)
    L = len(ups[0])
    pitch = 16 * ((L + 15) // 16)
    G = pitch // 16
    host = np.zeros((M, pitch), np.uint8)
    for c, u in enumerate(ups):
        host[c, :L] = np.frombuffer(u, np.uint8)
    dev = torch.from_numpy(host).cuda()
    hp = lay.header_positions()
    exp = oracle.update_faithful(ups, d)
    merged = torch.zeros(pitch, dtype=torch.uint8, device="cuda")
    f32 = torch.zeros(3 * G, dtype=torch.float32, device="cuda")
    ref = torch.zeros(pitch, dtype=torch.uint8, device="cuda")
    ref32 = torch.zeros(3 * G, dtype=torch.float32, device="cuda")
    codec.update_device(dev, L, d, hp, ref, ref32)
    codec.check()
    with codec.accumulator(L, hp) as acc:
        scratch = torch.empty(pitch, dtype=torch.uint8, device="cuda")
        for c in range(M):
            scratch.copy_(dev[c])
            acc.push_device(scratch, d[c])  # the row is the accumulator's own copy from here on
            scratch.zero_()
        assert acc.count == M
        acc.finish_device(merged, f32)
        assert acc.count == 0
        torch.cuda.synchronize()
        assert torch.equal(merged, ref) and torch.equal(f32.view(torch.int32), ref32.view(torch.int32))
        assert merged.cpu().numpy()[:L].tobytes() == exp
        assert same_bits(f32.cpu().numpy()[: lay.n_up], oracle.decode_floats(exp))
        # a bad row surfaces at finish_device and at a further push, until reset()
        bad = host[1].copy()
        bad[333] = ord("*")
        acc.push_device(dev[0], d[0])
        acc.push_device(torch.from_numpy(bad).cuda(), d[1])
        with pytest.raises(F.Base64Error) as ei:
            acc.finish_device(merged, f32)
        assert ei.value.code == F.FLEET_ERR_BASE64
        with pytest.raises(F.Base64Error):
            acc.push_device(dev[2], d[2])
        with pytest.raises(F.Base64Error):
            acc.push(ups[2], d[2])
        with pytest.raises(F.Base64Error):
            acc.finish()
        acc.reset()
        assert acc.count == 0
        v = oracle.synth_upload(81, 1, list(lay.w_sizes), list(lay.b_sizes))
        v[1] = 5.0  # a differing header slot
        hrow = np.zeros(pitch, np.uint8)
        hrow[:L] = np.frombuffer(oracle.encode_floats(v), np.uint8)
        acc.push_device(dev[0], d[0])
        acc.push_device(torch.from_numpy(hrow).cuda(), d[1])
        with pytest.raises(F.LayoutError):
            acc.finish_device(merged, f32)
        acc.reset()
        for c in (0, 1):  # mixed host and device pushes after the reset
            acc.push_device(dev[c], d[c])
        acc.push(ups[2], d[2])
        assert acc.finish() == oracle.update_faithful(ups[:3], d[:3])


# 9 ----------------------------------------------------------------------- updater

def test_updater_streaming_equals_batch(codec, oracle):
    from fleet_amd.updater import FleetUpdater
    lay = MNIST
    rng = np.random.default_rng(9)
    w0 = rng.normal(0, 0.05, lay.n_weights).astype(np.float32)
    b0 = rng.normal(0, 0.05, lay.n_fc_bias).astype(np.float32)
    mk = lambda s: FleetUpdater(codec, lay, 4, [0.05, 0.02, 0.01], w0, b0, policy=4, alpha=0.3, has_outlier=True,
                                streaming=s)
    a, b = mk(True), mk(False)

    class Recording:  # the batch object's codec, noting what each batch was made of
        def __init__(self, inner):
            self.inner, self.batches = inner, []

        def update(self, picked, dampen, want_f32=False):
            self.batches.append((list(picked), list(dampen)))
            return self.inner.update(picked, dampen, want_f32=want_f32)

        def __getattr__(self, name):
            return getattr(self.inner, name)

    b.codec = Recording(codec)
    ups = uploads_for(oracle, lay, 12, seed=91)
    for i, u in enumerate(ups):
        labels = [int(x) for x in rng.integers(0, 30, 10)]
        if i % 5 == 0:
            labels = [0] * 9 + [40]
        epoch = max(0, i // 4 - i % 3)  # stale by 0..2 epochs from the second batch on
        ra, rb = a.update(u, labels, epoch, client_id=i), b.update(u, labels, epoch, client_id=i)
        assert ra == rb and (ra is not None) == (i % 4 == 3)
        assert same_bits(a.weights, b.weights) and same_bits(a.fc_bias, b.fc_bias)
        assert a.curr_epoch == b.curr_epoch and a.global_labels == b.global_labels and a.lr == b.lr
        assert len(a.acc) == len(b.acc)
        if ra is not None:  # and both are the oracle's chain over the batch
            picked, dampen = b.codec.batches[-1]
            assert picked == ups[i - 3: i + 1]
            assert ra == oracle.update_faithful(picked, dampen)
    assert a.curr_epoch == 3 and len(b.codec.batches) == 3
    assert len({f for _, dampen in b.codec.batches for f in dampen}) > 2  # stale picks were dampened
