"""The Kardam ledger (fleet_kledger: Pool.ledger, k_pool_fold_kd): an update through the
ledger gives the pool's merged bytes and, per pick in pick order, what kardam.setGrad(id,
pickedGrad.scalarMultiply(getLrate()), epoch) leaves (CppNNUpdater.java:463-481,
Kardam.java:56-71). Every expected value is the oracle's per-op chain:
  g = scalar_mul(scalar_mul(flat_gradient(u), d), lr), norm(g), norm(subtract(g, prev)),
the rows bitwise decode_floats(g) in upload coordinates, the norms within 1e-12 relative
(getNorm's fp64 sum in another order, as for fleet_norm), the merged bytes
oracle.update_faithful's and Pool.update's."""
import math

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import MNIST, synthetic
from test_gpu_kardam_fused import scatter_flat
from test_gpu_pool import MIXED, filled, mixed, same_bits, scrambled, uploads_for

pytestmark = pytest.mark.gpu

LR = float(np.float32(0.05))  # getLrate() returns the float rate widened


class Book:
    """Kardam's `grads` in plain Python over the oracle: worker -> (g text, epoch)."""

    def __init__(self, oracle, layout):
        self.oracle, self.layout = oracle, layout
        self.grads = {}
        self._g = {}

    def g_text(self, up, d, lr):
        key = (up, d, lr)
        if key not in self._g:
            o = self.oracle
            self._g[key] = o.scalar_mul(o.scalar_mul(o.flat_gradient(up), d), lr)
        return self._g[key]

    def set_grads(self, picked, dampen, workers, epochs, lr):
        """(norm_g, norm_diff, set) per pick, in pick order (Kardam.java:56-71)."""
        out = []
        for up, d, w, ep in zip(picked, dampen, workers, epochs):
            if w < 0:
                out.append((None, None, False))
                continue
            g = self.g_text(up, d, lr)
            ng = self.oracle.norm(g)
            if w in self.grads:
                if self.grads[w][1] == ep:
                    out.append((ng, None, False))
                    continue
                out.append((ng, self.oracle.norm(self.oracle.subtract(g, self.grads[w][0])), True))
            else:
                out.append((ng, None, False))
            self.grads[w] = (g, ep)
        return out

    def check_ledger(self, ledger):
        for w in range(ledger.workers):
            assert ledger.has(w) == (w in self.grads), w
            if w in self.grads:
                g, ep = self.grads[w]
                assert ledger.epoch(w) == ep, w
                assert same_bits(ledger.read(w), scatter_flat(self.oracle.decode_floats(g), self.layout)), w


def check_outputs(exp, ng, nd, st):
    for k, (eg, ed, es) in enumerate(exp):
        assert bool(st[k]) == es, k
        if eg is None:
            assert math.isnan(ng[k]), k
        else:
            np.testing.assert_allclose(ng[k], eg, rtol=1e-12, atol=0, err_msg=f"norm_g[{k}]")
        if ed is None:
            assert math.isnan(nd[k]), k
        else:
            np.testing.assert_allclose(nd[k], ed, rtol=1e-12, atol=1e-300, err_msg=f"norm_diff[{k}]")


def run(oracle, book, pool, ledger, ups, slot_of, order, d, workers, epochs, lr=LR, plain=True, faithful=True):
    """One Ledger.update over the uploads `order` (indices into ups) against the book."""
    picks = [slot_of[i] for i in order]
    picked = [ups[i] for i in order]
    merged, f32, ng, nd, st = ledger.update(picks, d, workers, epochs, lr, want_f32=True)
    if faithful:
        exp_m = oracle.update_faithful(picked, d)
        assert merged == exp_m
        assert same_bits(f32, oracle.decode_floats(exp_m))
    if plain:
        pm, pf = pool.update(picks, d, want_f32=True)
        assert merged == pm and same_bits(f32, pf)
    check_outputs(book.set_grads(picked, d, workers, epochs, lr), ng, nd, st)
    return ng, nd, st


# 1 ------------------------------------------------------------------------ layouts

def big_layout():
    """More groups than the grid's lanes (8 blocks of 256 per CU): a lane takes a second
    grid-stride pass and a wave adds partials across iterations."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return synthetic(3 * (8 * cus * 256) + 3 * 700 + 2)


@pytest.mark.parametrize("name", ["mnist", "synthetic8", "synthetic3001", "two_passes"])
def test_layouts(codec, oracle, name):
    lay = {"mnist": MNIST, "synthetic8": synthetic(8), "synthetic3001": synthetic(3001)}.get(name) or big_layout()
    K = 2 if name == "two_passes" else 4
    if name == "mnist":
        assert lay.n_up % 3 != 0 and any(p % 3 for p in lay.header_positions())
    ups = uploads_for(oracle, lay, 2 * K, seed=len(name))
    where = scrambled(2 * K + 1, 2 * K, seed=3)
    book = Book(oracle, lay)
    with filled(codec, lay.header_positions(), ups, 2 * K + 1, where) as pool, pool.ledger(K + 1) as ledger:
        assert ledger.workers == K + 1 and not any(ledger.has(w) for w in range(K + 1))
        first, second = list(range(K)), list(range(2 * K - 1, K - 1, -1))
        _, nd, st = run(oracle, book, pool, ledger, ups, where, first, mixed(K), list(range(K)), [0] * K)
        assert not st.any() and np.isnan(nd).all()
        book.check_ledger(ledger)
        _, nd, st = run(oracle, book, pool, ledger, ups, where, second, mixed(K)[::-1], list(range(K)), [1] * K)
        assert st.all() and not np.isnan(nd).any()
        book.check_ledger(ledger)


# 2 ------------------------------------------------------------- picks per launch

@pytest.fixture(scope="module")
def pool140(codec, oracle):
    lay = synthetic(3001)
    ups = uploads_for(oracle, lay, 140, seed=2001)
    where = scrambled(140, 140, seed=14)
    pool = filled(codec, lay.header_positions(), ups, 140, where)
    yield pool, ups, where, lay
    pool.close()


@pytest.mark.parametrize("K", [1, 2, 3, 63, 64, 65, 129])
def test_picks_per_launch(oracle, pool140, K):
    """The odd and even ends of the pairwise wave reduction and the 64-pick launch
    boundaries; every pick in turn new (norm + store) and known (norm + diff + store)."""
    pool, ups, where, lay = pool140
    order = scrambled(140, K, seed=K)
    book = Book(oracle, lay)
    with pool.ledger(140) as ledger:
        run(oracle, book, pool, ledger, ups, where, order, mixed(K), order, [0] * K)
        book.check_ledger(ledger)
        d2 = [MIXED[(k + 1) % len(MIXED)] for k in range(K)]
        _, _, st = run(oracle, book, pool, ledger, ups, where, order[::-1], d2, order[::-1], [1] * K)
        assert st.all()
        book.check_ledger(ledger)


# 3 ------------------------------------------------- consecutive updates, one ledger

def test_three_updates_over_one_ledger(oracle, pool140):
    pool, ups, where, lay = pool140
    book = Book(oracle, lay)
    with pool.ledger(12, max_store=8) as ledger:
        # all new
        _, nd, st = run(oracle, book, pool, ledger, ups, where, [0, 1, 2, 3, 4, 5], mixed(6), [0, 1, 2, 3, 4, 5], [0] * 6)
        assert not st.any() and np.isnan(nd).all()
        book.check_ledger(ledger)
        rows_before = {w: ledger.read(w) for w in (2, 3)}
        # known at another epoch (0, 1), known at the same epoch (2, 3: ignored), new (6, 7), none (-1)
        workers = [0, 2, 6, -1, 1, 3, 7, -1]
        epochs = [1, 0, 1, 5, 2, 0, 1, 5]
        ng, nd, st = run(oracle, book, pool, ledger, ups, where, [10, 11, 12, 13, 14, 15, 16, 17], mixed(8), workers, epochs)
        assert st.tolist() == [True, False, False, False, True, False, False, False]
        assert np.isnan(ng).tolist() == [False, False, False, True, False, False, False, True]
        assert [ledger.epoch(w) for w in (0, 1, 2, 3, 6, 7)] == [1, 2, 0, 0, 1, 1]
        for w in (2, 3):  # the ignored pushes left row and epoch alone
            assert same_bits(ledger.read(w), rows_before[w])
        book.check_ledger(ledger)
        # all known
        _, nd, st = run(oracle, book, pool, ledger, ups, where, [20, 21, 22, 23, 24, 25, 26, 27], mixed(8),
                        [7, 6, 3, 2, 1, 0, 4, 5], [9] * 8)
        assert st.all() and not np.isnan(nd).any()
        book.check_ledger(ledger)
        ledger.forget(4)
        del book.grads[4]
        book.check_ledger(ledger)


# 4 ------------------------------------------------------- a worker twice in an update

def test_a_worker_twice(oracle, pool140):
    pool, ups, where, lay = pool140
    book = Book(oracle, lay)
    with pool.ledger(100) as ledger:
        # inside one launch, the worker new: the second pick's diff is against the first's G
        _, nd, st = run(oracle, book, pool, ledger, ups, where, [0, 1, 2, 3], mixed(4), [5, 6, 5, 7], [0, 0, 1, 0])
        assert st.tolist() == [False, False, True, False] and not math.isnan(nd[2])
        assert ledger.epoch(5) == 1
        book.check_ledger(ledger)
        # the first occurrence ignored by its epoch, the second not
        _, nd, st = run(oracle, book, pool, ledger, ups, where, [4, 5, 6], mixed(3), [5, 6, 5], [1, 3, 2])
        assert st.tolist() == [False, True, True] and ledger.epoch(5) == 2
        book.check_ledger(ledger)
        # across the launch boundary: k = 10 and k = 70 of K = 80, the worker known
        order = list(range(20, 100))
        workers = [20 + k for k in range(80)]
        workers[10] = workers[70] = 5
        epochs = [0] * 80
        epochs[10], epochs[70] = 7, 8
        _, nd, st = run(oracle, book, pool, ledger, ups, where, order, mixed(80), workers, epochs)
        assert st[10] and st[70] and int(st.sum()) == 2 and ledger.epoch(5) == 8
        book.check_ledger(ledger)


# 5 ----------------------------------------------------------------- rejected updates

def snapshot(ledger):
    return {w: (ledger.epoch(w), ledger.read(w)) for w in range(ledger.workers) if ledger.has(w)}


def same_snapshot(a, b):
    return a.keys() == b.keys() and all(a[w][0] == b[w][0] and same_bits(a[w][1], b[w][1]) for w in a)


@pytest.mark.parametrize("kind", ["base64", "layout"])
def test_a_rejected_update_leaves_no_trace(codec, oracle, kind):
    lay = synthetic(1001)
    ups = uploads_for(oracle, lay, 8, seed=55)
    if kind == "base64":
        bad = ups[1][:40] + b"*" + ups[1][41:]
    else:
        v = oracle.synth_upload(55, 1, list(lay.w_sizes), list(lay.b_sizes))
        v[0] = 2.0  # a differing header slot
        bad = oracle.encode_floats(v)
    assert len(bad) == len(ups[0])
    book = Book(oracle, lay)
    with filled(codec, lay.header_positions(), ups + [bad], 10) as pool, pool.ledger(6) as ledger:
        run(oracle, book, pool, ledger, ups, list(range(8)), [0, 1, 2], mixed(3), [0, 1, 2], [0, 0, 0])
        before = snapshot(ledger)
        rows = [pool.update([s], [1.0]) for s in range(8)]
        picks, d, workers, epochs = [3, 8, 4, 5], mixed(4), [0, 1, 3, 2], [1, 1, 1, 1]
        with pytest.raises(F.Base64Error if kind == "base64" else F.LayoutError) as ei:
            ledger.update(picks, d, workers, epochs, LR, want_f32=True)
        assert ei.value.code == (F.FLEET_ERR_BASE64 if kind == "base64" else F.FLEET_ERR_LAYOUT)
        assert ei.value.slots == [8] and [s for s in range(10) if pool.slot_status(s)] == [8]
        assert same_snapshot(snapshot(ledger), before) and not ledger.has(3)
        book.check_ledger(ledger)
        assert all(pool.occupied(s) for s in range(9)) and [pool.update([s], [1.0]) for s in range(8)] == rows
        # without the bad pick: what the update gives had the failed call never happened
        run(oracle, book, pool, ledger, ups, list(range(8)), [3, 4, 5], [d[0], d[2], d[3]], [0, 3, 2], [1, 1, 1])
        book.check_ledger(ledger)
        assert [s for s in range(10) if pool.slot_status(s)] == []


# 6 ---------------------------------------------------------------- argument errors

def test_argument_errors_before_launch(codec, oracle):
    lay = synthetic(1001)
    ups = uploads_for(oracle, lay, 5, seed=66)
    book = Book(oracle, lay)
    with codec.pool(len(ups[0]), lay.header_positions(), 4, group_begin=1) as windowed:
        with pytest.raises(F.FleetError) as ei:
            windowed.ledger(4)
        assert ei.value.code == F.FLEET_ERR_ARG
    with codec.pool(len(ups[0]), lay.header_positions(), 4, group_end=100) as windowed:
        with pytest.raises(F.FleetError) as ei:
            windowed.ledger(4)
        assert ei.value.code == F.FLEET_ERR_ARG
    with filled(codec, lay.header_positions(), ups, 6) as pool, pool.ledger(4, max_store=2) as ledger:
        for w, m in ((0, 2), (4, 0), (4, -1)):
            with pytest.raises(F.FleetError) as ei:
                pool.ledger(w, max_store=m)
            assert ei.value.code == F.FLEET_ERR_ARG
        run(oracle, book, pool, ledger, ups, list(range(5)), [0, 1], [1.0, 0.5], [0, 1], [0, 0])
        before = snapshot(ledger)

        def refused(picks, workers, epochs, lr=LR):
            with pytest.raises(F.FleetError) as ei:
                ledger.update(picks, mixed(len(picks)), workers, epochs, lr)
            assert ei.value.code == F.FLEET_ERR_ARG
            assert same_snapshot(snapshot(ledger), before) and [s for s in range(6) if pool.slot_status(s)] == []

        refused([2, 3], [0, 4], [1, 1])                  # a worker >= workers
        refused([2, 3, 4], [0, 1, 2], [1, 1, 1])         # three storing picks, max_store = 2
        refused([2, 3, 4], [2, 2, 2], [1, 2, 3])         # the same worker storing three times
        refused([2, 3], [0, 1], [1, 1], lr=float("nan"))
        refused([2, 3], [0, 1], [1, 1], lr=float("inf"))
        refused([2, 5], [0, 1], [1, 1])                  # the pool's own checks: an empty slot,
        refused([2, 2], [0, 1], [1, 1])                  # a slot twice
        for call in (ledger.has, ledger.epoch, ledger.read, ledger.forget):
            for w in (-1, 4):
                with pytest.raises(F.FleetError) as ei:
                    call(w)
                assert ei.value.code == F.FLEET_ERR_ARG
        for call in (ledger.epoch, ledger.read, ledger.forget):  # not in the ledger
            with pytest.raises(F.FleetError) as ei:
                call(3)
            assert ei.value.code == F.FLEET_ERR_ARG
        # two storing picks and an ignored one fit; nothing above left a trace
        run(oracle, book, pool, ledger, ups, list(range(5)), [2, 3, 4], mixed(3), [0, 1, 2], [1, 0, 1])
        book.check_ledger(ledger)


# 7 ------------------------------------------------------- repeatability and forms

def test_repeatable_and_the_forms_agree(oracle, pool140):
    torch = pytest.importorskip("torch")
    pool, ups, where, lay = pool140
    K = 70
    order = scrambled(140, K, seed=7)
    picks = [where[i] for i in order]
    workers = [k % 50 for k in range(K)]  # twenty workers twice, across the launch boundary too
    epochs = list(range(K))
    outs = []
    for form in ("host", "host", "device"):
        with pool.ledger(50, max_store=K) as ledger:
            first = ledger.update(picks[:50][::-1], mixed(50), workers[:50], [-1] * 50, LR)
            if form == "device":
                G = (len(ups[0]) + 15) // 16
                mu = torch.zeros(16 * G, dtype=torch.uint8, device="cuda")
                mf = torch.zeros(3 * G, dtype=torch.float32, device="cuda")
                side = torch.cuda.Stream()
                torch.cuda.synchronize()
                ng, nd, st = ledger.update_device(picks, mixed(K), workers, epochs, LR, mu, mf, stream=side.cuda_stream)
                merged, f32 = mu.cpu().numpy()[: len(ups[0])].tobytes(), mf.cpu().numpy()[: lay.n_up]
            else:
                merged, f32, ng, nd, st = ledger.update(picks, mixed(K), workers, epochs, LR, want_f32=True)
            outs.append((first[2], first[3], merged, f32, ng, nd, st, [ledger.read(w) for w in range(50)]))
    a = outs[0]
    assert not np.isnan(a[4]).any() and not np.isnan(a[5]).any() and a[6].all()
    for b in outs[1:]:
        assert same_bits(a[0], b[0]) and same_bits(a[4], b[4]) and same_bits(a[5], b[5])  # bitwise: np.float64 as 2 x u32
        assert a[2] == b[2] and same_bits(a[3], b[3]) and (a[6] == b[6]).all()
        assert all(same_bits(x, y) for x, y in zip(a[7], b[7]))
    assert a[2] == pool.update(picks, mixed(K))


# 8 ------------------------------------------------------- FleetUpdater end to end

def test_updater_with_kardam(codec, oracle):
    """Three updates at MNIST size, M = 3, against a plain-Python replay of
    CppNNUpdater.java:463-481 over Codec.kardam_grads and the text-keeping Kardam."""
    from fleet_amd.updater import FleetUpdater, Kardam, get_dampen
    lay = MNIST
    rng = np.random.default_rng(8)
    w = rng.normal(0, 0.05, lay.n_weights).astype(np.float32)
    b = rng.normal(0, 0.05, lay.n_fc_bias).astype(np.float32)
    lrates = [0.05, 0.02, 0.01]
    ups = uploads_for(oracle, lay, 9, seed=808)
    # arrival i: (client, epoch); client 1 twice in update 2, client 3 at an unchanged epoch in update 3
    arrivals = [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1), (1, 0), (3, 0), (2, 2), (4, -1)]
    script = [([2, 0, 1], []), ([1, 0, 2], []), ([0, 2, 1], [])]
    versions = [oracle.encode_floats(rng.normal(0, 1, 50).astype(np.float32)) for _ in range(12)]
    asked = []

    def kardam_model(tau):  # a new recorded text per call; none for a pick older than two epochs
        asked.append(tau)
        return None if tau > 2 else versions[len(asked) - 1]

    kd = Kardam(codec, 6)
    u = FleetUpdater(codec, lay, 3, lrates, w, b, policy=1, stale_size=2, picker=lambda p, e: script.pop(0),
                     kardam=kd, kardam_model=kardam_model)
    ref = Kardam(codec, 6)
    epoch, n_asked, lr = 0, 0, np.float32(lrates[0])
    for i, (cid, ep) in enumerate(arrivals):
        got = u.update(ups[i], [i % 10] * 10, ep, client_id=cid)
        if i % 3 != 2:
            assert got is None
            continue
        base = i - 2
        order = {2: [2, 0, 1], 5: [1, 0, 2], 8: [0, 2, 1]}[i]
        ids = [base + j for j in order]
        d = [get_dampen(1, epoch - arrivals[c][1]) for c in ids]
        assert got == oracle.update_faithful([ups[c] for c in ids], d)
        for c, dk in zip(ids, d):  # :463-481
            tau = epoch - arrivals[c][1]
            model = None if tau > 2 else versions[n_asked]
            n_asked += 1
            if model is None:
                continue
            ref.set_model(arrivals[c][0], model)
            if ref.set_grads([arrivals[c][0]], [ups[c]], [dk], float(lr), [arrivals[c][1]])[0]:
                ref.update_lip(arrivals[c][0])
        lr = np.float32(lrates[epoch])
        epoch += 1
        assert kd.lips.keys() == ref.lips.keys() and kd.grad_diff_norm.keys() == ref.grad_diff_norm.keys()
        for wk in ref.grad_diff_norm:
            np.testing.assert_allclose(kd.grad_diff_norm[wk], ref.grad_diff_norm[wk], rtol=1e-12, atol=0)
        for wk in ref.lips:
            np.testing.assert_allclose(kd.lips[wk], ref.lips[wk], rtol=1e-12, atol=0)
        assert kd.models == ref.models and kd.model_diff_norm == ref.model_diff_norm
        for wk, (g, gep) in ref.grads.items():
            assert kd.ledger.epoch(wk) == gep
            assert same_bits(kd.ledger.read(wk), scatter_flat(oracle.decode_floats(g), lay))
    assert sorted(ref.lips) == [1, 2] and len(ref.lips[1]) == 2 and not kd.ledger.has(4) and script == []
    assert kd.grads == {}  # the texts are never computed
