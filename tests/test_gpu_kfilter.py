"""Kardam's Byzantine filter on the upload pool (fleet_kfilter: Ledger.filter, k_pool_fold_kf):
KardamFilter.update is Ledger.update plus, per pick, the two norms Kardam.checkByz reads of it
(Kardam.java:158-161), and KardamFilter.resolve the average over the accepted picks merged into
the last pick's upload (CppNNUpdater.java:488-511 without the `true ||`). Every expected value
is the oracle's per-op chain:
  p = scalar_mul(flat_gradient(u), d), norm(p), norm(subtract(p, avg_prev)),
  avg = the add chain over the accepted picks, then scalar_mul(1 / accepted),
  merged = merge_flat_gradient(last pick's upload, avg),
the norms within 1e-12 relative (getNorm's fp64 sum in another order, as for fleet_norm), bytes
and rows bitwise."""
import math
import os

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import MNIST, synthetic
from test_gpu_kledger import LR, big_layout, same_snapshot, snapshot
from test_gpu_pool import MIXED, filled, mixed, same_bits, scrambled, uploads_for

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (7, 3, 2)  # a small model for the filters whose model rows are not what the test is about


class Chain:
    """The oracle's per-op chain over texts, each p computed once."""

    def __init__(self, oracle):
        self.o = oracle
        self._p = {}

    def p(self, up, d):
        if (up, d) not in self._p:
            self._p[(up, d)] = self.o.scalar_mul(self.o.flat_gradient(up), d)
        return self._p[(up, d)]

    def avg(self, picked, d, accept):
        o, a, n = self.o, None, 0
        for up, dk, ok in zip(picked, d, accept):
            if ok:
                a = self.p(up, dk) if a is None else o.add(a, self.p(up, dk))
                n += 1
        return None if a is None else o.scalar_mul(a, 1.0 / n)

    def merged(self, picked, d, accept):
        a = self.avg(picked, d, accept)
        return None if a is None else self.o.merge_flat_gradient(picked[-1], a)

    def check_norms(self, picked, d, last_avg, norm_p, norm_pdiff):
        o = self.o
        for k, (up, dk) in enumerate(zip(picked, d)):
            np.testing.assert_allclose(norm_p[k], o.norm(self.p(up, dk)), rtol=1e-12, atol=0, err_msg=f"norm_p[{k}]")
            if last_avg is None:
                assert math.isnan(norm_pdiff[k]), k
            else:
                np.testing.assert_allclose(norm_pdiff[k], o.norm(o.subtract(self.p(up, dk), last_avg)), rtol=1e-12,
                                           atol=1e-300, err_msg=f"norm_pdiff[{k}]")


def update_like_the_ledger(filt, twin, picks, d, workers, epochs, lr=LR):
    """KardamFilter.update beside Ledger.update on a twin ledger: every output the two share is
    the same bit for bit, the ledgers' rows and tables included. Returns the filter's outputs."""
    out = filt.update(picks, d, workers, epochs, lr, want_f32=True)
    m2, f2, ng2, nd2, st2 = twin.update(picks, d, workers, epochs, lr, want_f32=True)
    assert out[0] == m2 and same_bits(out[1], f2)
    assert same_bits(out[2], ng2) and same_bits(out[3], nd2) and (out[4] == st2).all()  # bitwise: f64 as 2 x u32
    assert same_snapshot(snapshot(filt.ledger), snapshot(twin))
    return out


def two_rounds(oracle, pool, ups, where, lay, first, second, d1, d2, workers1, workers2):
    """An update without a lastGrad, resolved with every pick accepted, then one against that
    average; both beside a twin ledger."""
    ch = Chain(oracle)
    with pool.ledger(len(ups)) as ledger, pool.ledger(len(ups)) as twin, ledger.filter(*SHAPE) as filt:
        assert not filt.has_last
        picked = [ups[i] for i in first]
        out = update_like_the_ledger(filt, twin, [where[i] for i in first], d1, workers1, [0] * len(first))
        ch.check_norms(picked, d1, None, out[5], out[6])
        assert np.isnan(out[6]).all()
        m, f32 = filt.resolve([True] * len(first), want_f32=True)
        assert m == out[0] and same_bits(f32, out[1]) and m == oracle.update_faithful(picked, d1)
        assert m == ch.merged(picked, d1, [True] * len(first)) and filt.has_last
        last = ch.avg(picked, d1, [True] * len(first))
        picked = [ups[i] for i in second]
        out = update_like_the_ledger(filt, twin, [where[i] for i in second], d2, workers2, [1] * len(second))
        ch.check_norms(picked, d2, last, out[5], out[6])
        assert not np.isnan(out[6]).any()
        assert filt.resolve([True] * len(second)) == out[0]


# 1 ------------------------------------------------------------------------ layouts

@pytest.mark.parametrize("name", ["mnist", "synthetic8", "synthetic3001", "two_passes"])
def test_layouts(codec, oracle, name):
    lay = {"mnist": MNIST, "synthetic8": synthetic(8), "synthetic3001": synthetic(3001)}.get(name) or big_layout()
    K = 2 if name == "two_passes" else 4
    ups = uploads_for(oracle, lay, 2 * K, seed=10 + len(name))
    where = scrambled(2 * K + 1, 2 * K, seed=3)
    with filled(codec, lay.header_positions(), ups, 2 * K + 1, where) as pool:
        # the second round: a Kardam-gated pick (worker -1) still has the filter's norms
        w2 = list(range(K))
        w2[-1] = -1
        two_rounds(oracle, pool, ups, where, lay, list(range(K)), list(range(2 * K - 1, K - 1, -1)), mixed(K),
                   mixed(K)[::-1], list(range(K)), w2)


# 2 ------------------------------------------------------------- picks per launch

@pytest.fixture(scope="module")
def pool140(codec, oracle):
    lay = synthetic(3001)
    ups = uploads_for(oracle, lay, 140, seed=2002)
    where = scrambled(140, 140, seed=15)
    pool = filled(codec, lay.header_positions(), ups, 140, where)
    yield pool, ups, where, lay
    pool.close()


@pytest.mark.parametrize("K", [1, 2, 3, 63, 64, 65, 129])
def test_picks_per_launch(oracle, pool140, K):
    """The odd and even ends of the pairwise wave reduction and the 64-pick launch boundaries,
    with four sums a pick."""
    pool, ups, where, lay = pool140
    order = scrambled(140, K, seed=K)
    d2 = [MIXED[(k + 1) % len(MIXED)] for k in range(K)]
    two_rounds(oracle, pool, ups, where, lay, order, order[::-1], mixed(K), d2, order, order[::-1])


# 3 --------------------------------------------------------------------- resolve masks

MASKS = {"all": lambda K: [True] * K,
         "first_rejected": lambda K: [False] + [True] * (K - 1),
         "last_rejected": lambda K: [True] * (K - 1) + [False],
         "alternating": lambda K: [k % 2 == 0 for k in range(K)],
         "only_one": lambda K: [k == K // 2 for k in range(K)],
         "none": lambda K: [False] * K}


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("K", [5, 65])
def test_resolve_masks(oracle, pool140, K, mask):
    """The refold over the accepted picks, merged into the last pick's upload whether it was
    accepted or not. The slots that come from the last pick are the layout's header slots: a
    pool's layout covers the whole upload (its walk ends at the last value), so no layout it
    accepts has slots at or past the walk's end, and an update whose picks differ in a header
    slot is a LayoutError (test_rejected_updates) -- uploads that differ where the last pick is
    copied cannot be built."""
    torch = pytest.importorskip("torch")
    pool, ups, where, lay = pool140
    ch = Chain(oracle)
    order = scrambled(140, K, seed=100 + K)
    picks, picked, d = [where[i] for i in order], [ups[i] for i in order], mixed(K)
    accept = MASKS[mask](K)
    exp = ch.merged(picked, d, accept)
    with pool.ledger(140) as ledger, ledger.filter(*SHAPE) as filt:
        out = filt.update(picks, d, order, [0] * K, LR, want_f32=True)
        got = filt.resolve(accept, want_f32=True)
        if mask == "none":
            assert got is None and exp is None and not filt.has_last
        else:
            assert got[0] == exp and same_bits(got[1], oracle.decode_floats(exp)) and filt.has_last
        if mask == "all":
            assert got[0] == out[0] and same_bits(got[1], out[1]) and got[0] == pool.update(picks, d)
        # the device forms, on a stream of the caller's
        G = (len(ups[0]) + 15) // 16
        mu = torch.zeros(16 * G, dtype=torch.uint8, device="cuda")
        mf = torch.zeros(3 * G, dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        dev = filt.update_device(picks, d, order, [1] * K, LR, mu, mf, stream=side.cuda_stream)
        assert mu.cpu().numpy()[: len(ups[0])].tobytes() == out[0] and same_bits(mf.cpu().numpy()[: lay.n_up], out[1])
        assert same_bits(dev[3], out[5])
        ok = filt.resolve_device(accept, mu, mf, stream=side.cuda_stream)
        assert ok == (mask != "none")
        if ok:
            assert mu.cpu().numpy()[: len(ups[0])].tobytes() == exp
            assert same_bits(mf.cpu().numpy()[: lay.n_up], oracle.decode_floats(exp))


# 4 ------------------------------------------------------- lastGrad over several updates

def test_an_update_without_an_average_keeps_the_last_gradient(oracle, pool140):
    pool, ups, where, lay = pool140
    ch = Chain(oracle)
    with pool.ledger(140) as ledger, ledger.filter(*SHAPE) as filt:
        rounds = [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9, 10, 11]]
        picked = [[ups[i] for i in r] for r in rounds]
        d = [mixed(len(r)) for r in rounds]
        filt.update([where[i] for i in rounds[0]], d[0], rounds[0], [0] * 4, LR)
        assert filt.resolve([True] * 4) is not None
        first_avg = ch.avg(picked[0], d[0], [True] * 4)
        out = filt.update([where[i] for i in rounds[1]], d[1], rounds[1], [0] * 3, LR)
        ch.check_norms(picked[1], d[1], first_avg, out[5], out[6])
        assert filt.resolve([False] * 3) is None and filt.has_last
        out = filt.update([where[i] for i in rounds[2]], d[2], rounds[2], [0] * 5, LR)
        ch.check_norms(picked[2], d[2], first_avg, out[5], out[6])  # not against the middle update's optimistic result
        assert filt.resolve([True] * 5) is not None


def test_a_refold_advances_the_last_gradient_to_the_refolded_average(oracle, pool140):
    pool, ups, where, lay = pool140
    ch = Chain(oracle)
    with pool.ledger(140) as ledger, ledger.filter(*SHAPE) as filt:
        a, b = list(range(20, 27)), list(range(30, 34))
        pa, pb, da, db = [ups[i] for i in a], [ups[i] for i in b], mixed(7), mixed(4)[::-1]
        accept = [True, False, True, True, False, True, False]
        filt.update([where[i] for i in a], da, a, [0] * 7, LR)
        assert filt.resolve(accept) == ch.merged(pa, da, accept)
        refolded, optimistic = ch.avg(pa, da, accept), ch.avg(pa, da, [True] * 7)
        assert refolded != optimistic
        out = filt.update([where[i] for i in b], db, b, [0] * 4, LR)
        ch.check_norms(pb, db, refolded, out[5], out[6])
        far = oracle.norm(oracle.subtract(ch.p(pb[0], db[0]), optimistic))
        assert abs(out[6][0] - far) > 1e-9 * far  # the test can tell the two apart
        # a second update discards the pending one: the first's decisions no longer apply
        out2 = filt.update([where[i] for i in b[:3]], db[:3], b[:3], [1] * 3, LR)
        ch.check_norms(pb[:3], db[:3], refolded, out2[5], out2[6])
        with pytest.raises(F.FleetError) as ei:
            filt.resolve([True] * 4)
        assert ei.value.code == F.FLEET_ERR_ARG
        assert filt.resolve([True, True, False]) == ch.merged(pb[:3], db[:3], [True, True, False])


# 5 ----------------------------------------------------------------------------- errors

@pytest.mark.parametrize("kind", ["base64", "layout"])
def test_rejected_updates(codec, oracle, kind):
    lay = synthetic(1001)
    ups = uploads_for(oracle, lay, 8, seed=56)
    if kind == "base64":
        bad = ups[1][:40] + b"*" + ups[1][41:]
    else:
        v = oracle.synth_upload(56, 1, list(lay.w_sizes), list(lay.b_sizes))
        v[0] = 2.0  # a differing header slot
        bad = oracle.encode_floats(v)
    ch = Chain(oracle)
    with filled(codec, lay.header_positions(), ups + [bad], 10) as pool, pool.ledger(6) as ledger, \
            ledger.filter(*SHAPE) as filt:
        d3 = mixed(3)
        filt.update([0, 1, 2], d3, [0, 1, 2], [0, 0, 0], LR)
        assert filt.resolve([True, False, True]) is not None
        last = ch.avg(ups[:3], d3, [True, False, True])
        before = snapshot(ledger)
        rows = [pool.update([s], [1.0]) for s in range(8)]
        picks, d, workers, epochs = [3, 8, 4, 5], mixed(4), [0, 1, 3, 2], [1, 1, 1, 1]
        with pytest.raises(F.Base64Error if kind == "base64" else F.LayoutError) as ei:
            filt.update(picks, d, workers, epochs, LR, want_f32=True)
        assert ei.value.slots == [8] and [s for s in range(10) if pool.slot_status(s)] == [8]
        assert same_snapshot(snapshot(ledger), before) and not ledger.has(3) and filt.has_last
        assert all(pool.occupied(s) for s in range(9)) and [pool.update([s], [1.0]) for s in range(8)] == rows
        with pytest.raises(F.FleetError) as ei:  # nothing is pending after the failed update
            filt.resolve([True] * 4)
        assert ei.value.code == F.FLEET_ERR_ARG
        # the read row of lastGrad is the one from before the failed optimistic pass
        out = filt.update([3, 4, 5], [d[0], d[2], d[3]], [0, 3, 2], [1, 1, 1], LR)
        ch.check_norms([ups[3], ups[4], ups[5]], [d[0], d[2], d[3]], last, out[5], out[6])
        assert [s for s in range(10) if pool.slot_status(s)] == []


def test_resolve_argument_errors(codec, oracle):
    lay = synthetic(1001)
    ups = uploads_for(oracle, lay, 5, seed=67)
    ch = Chain(oracle)
    L = F.lib()
    with filled(codec, lay.header_positions(), ups, 6) as pool, pool.ledger(5) as ledger, ledger.filter(*SHAPE) as filt:
        def refused(accept):
            with pytest.raises(F.FleetError) as ei:
                filt.resolve(accept)
            assert ei.value.code == F.FLEET_ERR_ARG

        refused([True, True])  # no update is pending
        d = mixed(3)
        out = filt.update([0, 1, 2], d, [0, 1, 2], [0, 0, 0], LR)
        before = snapshot(ledger)
        refused([True, True])              # K differs
        refused([True, True, True, True])
        import ctypes as C
        n = C.c_size_t(9)
        buf = np.zeros(len(ups[0]) + 16, np.uint8)
        acc = np.ones(3, np.uint8)
        for args in ((None, 3, buf.ctypes.data, len(buf), C.byref(n), None),
                     (acc.ctypes.data, 3, None, len(buf), C.byref(n), None),
                     (acc.ctypes.data, 3, buf.ctypes.data, len(buf), None, None)):
            assert L.fleet_kfilter_resolve(filt._h, *args) == F.FLEET_ERR_ARG
        assert L.fleet_kfilter_resolve(filt._h, acc.ctypes.data, 3, buf.ctypes.data, 8, C.byref(n), None) == \
            F.FLEET_ERR_CAPACITY
        assert n.value == 9 and (buf == 0).all()
        pool.drop(1)                       # a picked slot is no longer occupied
        refused([True, True, True])
        refused([True, False, True])
        assert not filt.has_last and same_snapshot(snapshot(ledger), before)
        pool.put(1, ups[1])                # everything was left untouched: the update is still pending
        assert filt.resolve([True, False, True]) == ch.merged(ups[:3], d, [True, False, True])
        assert filt.has_last and out[0] == ch.merged(ups[:3], d, [True] * 3)
        refused([True, True, True])        # resolved: nothing is pending
        with pytest.raises(F.FleetError):
            ledger.filter(0, 0, 1)         # a model of no values


# 6 ------------------------------------------------------------------------ model rows

def test_model_rows(codec, oracle):
    """set_model from a host Model and set_model_device from a ResidentModel give the same
    norms, the oracle's over the getModelParametersNative texts; the last row advances only
    when a resolve ends with an average."""
    s = np.load(os.path.join(HERE, "golden", "session_mnist.npz"))
    lay = synthetic(8)
    ups = uploads_for(oracle, lay, 3, seed=68)
    m = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    rm = F.ResidentModel(codec, bytes(s["init"]), distillation_mode=1)
    for x in (m, rm):
        x.initUpdater(s["lrates"])
    nw, nb, ge, _ = m.shape()
    with filled(codec, lay.header_positions(), ups, 3) as pool, pool.ledger(3) as l1, pool.ledger(3) as l2, \
            l1.filter(nw, nb, ge) as fh, l2.filter(nw, nb, ge) as fd:
        texts = []

        def stage():
            v = m.modelsSize() - 1
            texts.append(m.getModelParametersNative(v))
            assert rm.getModelParametersNative(v) == texts[-1]
            a = fh.set_model(*m.export(v))
            b = fd.set_model_device(*rm.version_tensors(v))
            assert a[0] == b[0] and (a[1] == b[1] or (math.isnan(a[1]) and math.isnan(b[1])))
            np.testing.assert_allclose(a[0], oracle.norm(texts[-1]), rtol=1e-12, atol=0)
            return a

        def update(accept):
            for f in (fh, fd):
                f.update([0, 1, 2], mixed(3), [0, 1, 2], [len(texts)] * 3, LR)
                f.resolve(accept)

        def step(i):
            for x in (m, rm):
                x.descentNative(bytes(s[f"merged{i}"]), int(s["batch"]), 2)

        assert math.isnan(stage()[1])          # no last model yet
        update([False] * 3)                    # no average: the staged model does not become the last one
        step(0)
        assert math.isnan(stage()[1])
        update([True, False, True])            # texts[1] becomes lastModel
        step(1)
        nd = stage()[1]
        np.testing.assert_allclose(nd, oracle.norm(oracle.subtract(texts[2], texts[1])), rtol=1e-12, atol=0)
        update([False] * 3)                    # lastModel stays texts[1]
        step(2)
        nd = stage()[1]
        np.testing.assert_allclose(nd, oracle.norm(oracle.subtract(texts[3], texts[1])), rtol=1e-12, atol=0)
        far = oracle.norm(oracle.subtract(texts[3], texts[2]))
        assert abs(nd - far) > 1e-9 * far
        with pytest.raises(ValueError):
            fh.set_model(np.zeros(nw + 1, np.float32), np.zeros(nb, np.float32))
    m.close()
    rm.close()


# 7 ------------------------------------------------------- FleetUpdater end to end

class TextKardam:
    """utils/Kardam.java over host texts and the oracle's per-op functions: setGrad (:56-71) and
    setModel (:114-125) transcribed here, checkByz and updateLip (:136-203) by the
    transcription of test_kfilter_cpu, fed the norms the reference takes of the texts."""

    def __init__(self, oracle, workers):
        from test_kfilter_cpu import JavaKardam
        self.o = oracle
        self.j = JavaKardam(workers)
        self.grads, self.models = {}, {}

    def setGrad(self, w, g, epoch):  # noqa: N802
        if w in self.grads:
            if self.grads[w][1] == epoch:
                return False
            self.j.gradDiffNorm[w] = self.o.norm(self.o.subtract(g, self.grads[w][0]))
            self.grads[w] = (g, epoch)
            return True
        self.grads[w] = (g, epoch)
        return False

    def setModel(self, w, m):  # noqa: N802
        if w in self.models:
            norm = self.o.norm(self.o.subtract(m, self.models[w]))
            if norm == 0:
                return
            self.j.modelDiffNorm[w] = norm
        self.models[w] = m

    def checkByz(self, g, lastGrad, currModel, lastModel):  # noqa: N802
        """The decision, and whether it read the norms; then |checkNorm - high| > 1e-9 high is
        asserted: both sides carry the 1e-12 of a reordered getNorm."""
        o = self.o
        if lastGrad is None:
            ok = self.j.checkByz(o.norm(g), math.nan, o.norm(currModel), math.nan, True)
        else:
            ok = self.j.checkByz(o.norm(g), o.norm(o.subtract(g, lastGrad)), o.norm(currModel),
                                 o.norm(o.subtract(currModel, lastModel)), False)
        if self.j.last is not None:
            cn, high = self.j.last
            assert abs(cn - high) > 1e-9 * high, (cn, high)
        return ok, self.j.last


@pytest.mark.parametrize("resident", [False, True], ids=["host_model", "resident_model"])
def test_updater_session_with_the_filter(codec, oracle, resident):
    """Eight updates at MNIST size, M = 4, staleSize = 2, 10 workers, against a restatement of
    CppNNUpdater.java:417-516 (the `true ||` of :488 removed) over host texts. Worker 9 uploads
    gradients 40 times the others' size."""
    from fleet_amd.updater import FleetUpdater, Kardam, get_dampen, similarity
    o = oracle
    s = np.load(os.path.join(HERE, "golden", "session_mnist.npz"))
    lay, M, STALE, WORKERS, UPDATES = MNIST, 4, 2, 10, 8
    lrates = [1.0, 0.5] * 5
    batch = int(s["batch"])
    cls = F.ResidentModel if resident else F.Model
    model = cls(codec, bytes(s["init"]), distillation_mode=1)
    ref = F.Model(codec, bytes(s["init"]), distillation_mode=1)  # the restatement's cnn and `models`
    model.initUpdater(lrates), ref.initUpdater(lrates)
    rng = np.random.default_rng(21)
    ups = uploads_for(o, lay, M * UPDATES, seed=2121)
    mask = np.asarray(o.header_mask(list(lay.w_sizes), list(lay.b_sizes))).astype(bool)
    cids = []
    for u_i in range(UPDATES):  # worker 9 once per update, at a position that moves; the others in turn
        row = [(3 * u_i + j) % 9 for j in range(3)]
        row.insert(u_i % 4, 9)
        cids += row
    for i, cid in enumerate(cids):
        if cid == 9:
            v = o.decode_floats(ups[i]).copy()
            v[: len(mask)][~mask[: len(v)]] *= np.float32(40.0)
            ups[i] = o.encode_floats(v)
    kd = Kardam(codec, WORKERS)
    pick_first = lambda pending, epoch: (list(range(M)), [])  # noqa: E731
    if resident:
        u = FleetUpdater(codec, lay, M, lrates, None, None, policy=1, stale_size=STALE, picker=pick_first, kardam=kd,
                         kardam_models=model, model=model, kardam_filter=True)
    else:
        w0 = rng.normal(0, 0.05, lay.n_weights).astype(np.float32)
        b0 = rng.normal(0, 0.05, lay.n_fc_bias).astype(np.float32)
        u = FleetUpdater(codec, lay, M, lrates, w0, b0, policy=1, stale_size=STALE, picker=pick_first, kardam=kd,
                         kardam_models=model, kardam_filter=True)
    tk = TextKardam(o, WORKERS)
    epoch, lr = 0, np.float32(lrates[0])
    global_labels = [0] * 10
    lastGrad = lastModel = None
    pending, trace = [], []
    for i, cid in enumerate(cids):
        ep = max(0, epoch - (1 if i % 5 == 3 else 0))  # most uploads on the current model, some one behind
        labels = [(i + j) % 3 for j in range(10)]
        weights_before = None if resident else u.weights.copy()
        got = u.update(ups[i], labels, ep, client_id=cid)
        pending.append((ups[i], labels, ep, cid))
        if len(pending) < M:
            assert got is None
            continue
        # ---- the restatement (:417-516)
        n = ref.modelsSize()
        currModel = ref.getModelParametersNative(n - 1)
        avg, avgSize, decisions, window = None, 0, [], [0] * 10
        for up, lab, pep, pid in pending:
            tau = epoch - pep
            d = get_dampen(1, tau, similarity(lab, global_labels), STALE, 0.0, False)
            pickedGrad = o.scalar_mul(o.flat_gradient(up), d)
            window = [a + b for a, b in zip(window, lab)]
            if n - 1 - tau >= 0:
                pickedModel = ref.getModelParametersNative(n - 1 - tau)
                if n == STALE:
                    tk.setModel(pid, pickedModel)
                    if tk.setGrad(pid, o.scalar_mul(pickedGrad, float(lr)), pep):
                        tk.j.updateLip(pid)
            if n < STALE:
                ok, read = True, None
            else:
                ok, read = tk.checkByz(pickedGrad, lastGrad, currModel, lastModel)
            decisions.append(ok)
            trace.append((len(trace) // M, pid, ok, read))
            if ok:
                avg = pickedGrad if avg is None else o.add(avg, pickedGrad)
                avgSize += 1
        global_labels = [a + b for a, b in zip(global_labels, window)]
        expected = None
        if avg is not None:
            avg = o.scalar_mul(avg, 1.0 / avgSize)
            expected = o.merge_flat_gradient(pending[-1][0], avg)
            ref.descentNative(expected, batch, STALE)
            lastGrad, lastModel = avg, currModel
            lr = np.float32(lrates[epoch]) if epoch < len(lrates) else lr
            epoch += 1
        pending = []
        # ---- the updater against it
        print(f"update {len(trace) // M}: accept {decisions} rejects {tk.j.subsequentRejects}", trace[-M:])
        assert u.last_accept == decisions
        assert got == expected
        assert u.curr_epoch == epoch and kd.subsequent_rejects == tk.j.subsequentRejects
        assert u.global_labels == global_labels and u.acc == []
        assert kd.lips.keys() == tk.j.lips.keys()
        for wk in tk.j.lips:
            assert len(kd.lips[wk]) == len(tk.j.lips[wk])
            np.testing.assert_allclose(kd.lips[wk], tk.j.lips[wk], rtol=1e-12, atol=0)
        if not resident:
            if got is None:
                assert same_bits(u.weights, weights_before)
            else:
                model.descentNative(got, batch, STALE)
        assert model.modelsSize() == ref.modelsSize()
        assert model.getModelParametersNative(ref.modelsSize() - 1) == ref.getModelParametersNative(ref.modelsSize() - 1)
        assert float(model.getLrate()) == float(ref.getLrate())
    by_norm = [t for t in trace if t[3] is not None]
    assert len(trace) == M * UPDATES and by_norm
    assert any(pid == 9 and not ok for _, pid, ok, _ in by_norm)       # the scaled worker is filtered
    assert any(ok for _, pid, ok, _ in by_norm)                        # and the filter lets picks through
    per_update = [[t[2] for t in trace if t[0] == k] for k in range(UPDATES)]
    assert any(0 < sum(a) < M for a in per_update)                     # a refolded update
    assert any(sum(a) == 0 for a in per_update)                        # an update without an average
    assert any(ok and read[0] > read[1] for _, _, ok, read in by_norm)  # the `== workers` escape
    for x in (u._filter, u._ledger, u._mledger):
        if x is not None:
            x.close()
    model.close(), ref.close()
