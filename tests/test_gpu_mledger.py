"""The Kardam model ledger (fleet_mledger: ModelLedger, k_mrow_stage, k_mrow_pair_norms):
model versions resident as fp32 rows, and kardam.setModel (CppNNUpdater.java:472-476,
Kardam.java:114-125) for every pick of an update from one device pass. Every expected value
is the oracle's per-op chain over the texts the reference would hold:
  T = encode_floats(getModelParams vector), norm(subtract(T_cur, T_prev)), norm(T),
the rows bitwise decode_floats(T), the norms within 1e-12 relative (getNorm's fp64 sum in
another order, as for fleet_norm and the gradient ledger), a norm the oracle gives as exactly
0.0 exactly 0.0.

Case 5's NaN-norm leg: no parameter values give the oracle a non-finite norm (every value,
inf and nan included, encodes to a code that decodes to a finite float of magnitude at most
about 1e8, so D * D and its double sum stay finite; test_special_values asserts this premise
on the oracle). "A NaN norm is not 0 and stores, status 3" is therefore pinned where a NaN
can be fed in: tests/native/check_mledger_table.cpp, driven by tests/test_mledger_cpu.py."""
import ctypes as C_
import math
import os

import numpy as np
import pytest

import fleet_amd as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def params_vector(w, b, edges):
    """network::getModelParams (network.h:708-723): the biases once per layer-graph edge, then the weights."""
    return np.concatenate([np.asarray(b, np.float32)] * edges + [np.asarray(w, np.float32)]).astype(np.float32)


class Version:
    """One model version: its vectors and the text the reference would hand to setModel."""

    def __init__(self, oracle, vid, w, b, edges):
        self.id, self.w, self.b = vid, np.asarray(w, np.float32), np.asarray(b, np.float32)
        self.text = oracle.encode_floats(params_vector(self.w, self.b, edges))
        self.row = oracle.decode_floats(self.text)
        self.norm = oracle.norm(self.text)


class Book:
    """Kardam's `models` and `modelDiffNorm` in plain Python over the oracle (Kardam.java:114-125)."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.models = {}  # worker -> Version
        self.model_diff_norm = {}
        self._norms = {}

    def pair_norm(self, cur, prev):
        key = (cur.text, prev.text)
        if key not in self._norms:
            self._norms[key] = self.oracle.norm(self.oracle.subtract(cur.text, prev.text))
        return self._norms[key]

    def set_model(self, worker, mcurr):
        """(status, norm) of one setModel call."""
        status, norm = 1, None
        if worker in self.models:
            norm = self.pair_norm(mcurr, self.models[worker])
            if norm == 0:
                return 2, norm
            self.model_diff_norm[worker] = norm
            status = 3
        self.models[worker] = mcurr
        return status, norm

    def update(self, versions, workers):
        return [(0, None, None) if w < 0 else self.set_model(w, v) + (v.norm,) for v, w in zip(versions, workers)]

    def check_ledger(self, ledger):
        for w in range(ledger.workers):
            assert ledger.has(w) == (w in self.models), w
            if w in self.models:
                assert ledger.version(w) == self.models[w].id, w
                assert same_bits(ledger.read(w), self.models[w].row), w
            else:
                with pytest.raises(F.FleetError):
                    ledger.version(w)


def check_outputs(exp, nm, nd, st):
    assert len(nm) == len(nd) == len(st) == len(exp)
    for k, (es, ed, em) in enumerate(exp):
        assert int(st[k]) == es, (k, int(st[k]), es)
        if em is None:
            assert math.isnan(nm[k]), k
        else:
            np.testing.assert_allclose(nm[k], em, rtol=1e-12, atol=0, err_msg=f"norm_model[{k}]")
        if es in (0, 1):
            assert math.isnan(nd[k]), k
        elif es == 2:
            assert ed == 0.0 and nd[k] == 0.0, (k, nd[k])
        elif math.isnan(ed):
            assert math.isnan(nd[k]), k
        else:
            assert nd[k] != 0.0, k
            np.testing.assert_allclose(nd[k], ed, rtol=1e-12, atol=0, err_msg=f"norm_diff[{k}]")


def run(book, ledger, versions, workers):
    """One ModelLedger.update against the book; the versions must be resident."""
    nm, nd, st = ledger.update([v.id for v in versions], workers)
    check_outputs(book.update(versions, workers), nm, nd, st)
    book.check_ledger(ledger)
    return nm, nd, st


def ordinary(rng, n):
    """N(0, 0.1) parameters with a few of magnitude above 1 (another digit count in the codec)."""
    x = rng.normal(0, 0.1, n).astype(np.float32)
    if n:
        x[rng.integers(0, n, max(1, n // 16))] *= np.float32(37.0)
    return x


def make_versions(oracle, rng, count, n_w, n_b, edges, first_id=100):
    return [Version(oracle, first_id + 7 * i, ordinary(rng, n_w), ordinary(rng, n_b), edges) for i in range(count)]


def stage_all(ledger, versions):
    for v in versions:
        ledger.stage(v.id, v.w, v.b)
        assert ledger.resident(v.id)


# 1 ------------------------------------------------------------------------- shapes

def shape_edges():
    """Where the kernels change path, from their own constants: a lane owns 4 values, so a wave
    64 * 4 and a block `block_values`; a row or pair runs on at most `max_blocks` blocks, so
    past block_values * max_blocks values a lane takes a second pass."""
    wave, block_values, max_blocks = F.ModelLedger.launch_shape()
    lane = block_values // 256
    assert (wave, lane) == (64, 4)
    w, b, g = wave * lane, block_values, block_values * max_blocks
    return [1, 2, 3, 4, 5, w - 1, w, w + 1, b - 1, b, b + 1, g + 5]


SHAPES = [(n_b, i) for n_b in (0, 3) for i in range(12)]


@pytest.mark.parametrize("n_b,i", SHAPES)
def test_shapes(codec, oracle, n_b, i):
    """n_b = 3 over 2 edges: the bias / weight seam (value 6) and the bias repeat (value 3) fall
    inside a lane's values; there n = 6 + n_w, so the small sizes are n_w = 0, 1, 2, ..."""
    edges = 2 if n_b else 0
    n = shape_edges()[i]
    n_w = n if not n_b else (i if i < 5 else n - n_b * edges)
    rng = np.random.default_rng(1000 + 31 * i + n_b)
    a, b = make_versions(oracle, rng, 2, n_w, n_b, edges)
    with codec.model_ledger(n_w, n_b, edges, workers=2, max_versions=2) as led:
        assert led.n == len(a.row) == n_b * edges + n_w
        stage_all(led, [a, b])
        for v in (a, b):
            assert same_bits(led.read_version(v.id), v.row)
            text = codec.getModelParametersNative(v.w, v.b, edges)
            assert text == v.text and same_bits(codec.decode_floats(text), led.read_version(v.id))
        book = Book(oracle)
        run(book, led, [a], [0])
        _, nd, st = run(book, led, [b, b], [0, 1])
        assert list(st) == [3, 1] and nd[0] > 0
        # the ordered pair the other way round, and the same bits from the same inputs
        _, nd2, _ = run(book, led, [a], [0])
        led.forget(0)
        book.models.pop(0)
        run(book, led, [b], [0])
        _, nd3, _ = run(book, led, [a], [0])
        assert nd2[0] == nd3[0]


def test_stage_device_matches_stage(codec, oracle):
    """The device-pointer form on a stream of the caller's: the same rows, and the update that
    follows on the ledger's own stream sees them."""
    import torch
    n_w, n_b, edges = 1500, 3, 2
    rng = np.random.default_rng(11)
    a, b = make_versions(oracle, rng, 2, n_w, n_b, edges)
    side = torch.cuda.Stream()
    with codec.model_ledger(n_w, n_b, edges, workers=2, max_versions=2) as led:
        with torch.cuda.stream(side):
            dev = [(torch.from_numpy(v.w).cuda(), torch.from_numpy(v.b).cuda()) for v in (a, b)]
            for v, (dw, db) in zip((a, b), dev):
                led.stage_device(v.id, dw, db, stream=side.cuda_stream)
        book = Book(oracle)
        run(book, led, [a, b], [0, 0])
        for v in (a, b):
            assert led.resident(v.id) and same_bits(led.read_version(v.id), v.row)
        side.synchronize()
        with pytest.raises(ValueError):
            led.stage_device(999, dev[0][0][:-1], dev[0][1])


# 2 ------------------------------------------------------------ the four statuses

def test_statuses_over_three_rounds(codec, oracle):
    n_w, n_b, edges = 700, 3, 2
    rng = np.random.default_rng(2)
    A, B, C = make_versions(oracle, rng, 3, n_w, n_b, edges)
    with codec.model_ledger(n_w, n_b, edges, workers=5, max_versions=3) as led:
        stage_all(led, [A, B, C])
        book = Book(oracle)
        book.check_ledger(led)
        _, _, st = run(book, led, [A, A, B], [0, 1, 2])  # first models
        assert list(st) == [1, 1, 1]
        # set, with a skipped pick (its id names nothing) and a worker the ledger does not know yet
        ghost = Version(oracle, -5, A.w, A.b, edges)
        _, _, st = run(book, led, [B, ghost, C, C], [0, -1, 3, 2])
        assert list(st) == [3, 0, 1, 3]
        # a re-pick of the same version (ignored) and a worker moved to another version
        _, nd, st = run(book, led, [B, A, C], [0, 2, 1])
        assert list(st) == [2, 3, 3] and nd[0] == 0.0
        assert not led.has(4)


# 3 ------------------------------------------- zero norm between different texts

def zero_twins(oracle, pad):
    """Two parameter vectors whose texts differ and whose difference has norm exactly 0 both
    ways: Q(x) = 0 for |x| <= 1e-8, so D = Q(a - b) is 0 where a and b differ by less."""
    q = lambda x: oracle.decode_floats(oracle.encode_floats(np.asarray(x, np.float32)))
    a = q([0.01, 0.02, -0.03, 0.5])
    b = q((a + np.array([5e-9, -4e-9, 6e-9, 0], np.float32)).astype(np.float32))
    tail = np.linspace(-0.4, 0.4, pad).astype(np.float32)
    return np.concatenate([a, tail]), np.concatenate([b, tail])


def test_zero_norm_between_different_texts_keeps_the_old_model(codec, oracle):
    """The reference ignores the pick (Kardam.java:118-121): the worker keeps the OLD model, so
    the next pick is differenced against it. Storing unconditionally fails here."""
    pa, pb = zero_twins(oracle, 300)
    none = np.zeros(0, np.float32)
    A, B = Version(oracle, 1, pa, none, 0), Version(oracle, 2, pb, none, 0)
    assert A.text != B.text and not same_bits(A.row, B.row)
    assert oracle.norm(oracle.subtract(B.text, A.text)) == 0.0 and oracle.norm(oracle.subtract(A.text, B.text)) == 0.0
    # a third version that tells the two apart: its difference to A is not its difference to B
    # (A and B are 5e-9 apart and Q keeps 1e-8 steps, so only some third versions do: the first
    # of a fixed series that does on the oracle)
    for seed in range(64):
        C = Version(oracle, 3, pa + ordinary(np.random.default_rng(300 + seed), len(pa)) * np.float32(1e-3), none, 0)
        to_a, to_b = oracle.norm(oracle.subtract(C.text, A.text)), oracle.norm(oracle.subtract(C.text, B.text))
        if abs(to_a - to_b) > 1e-9 * to_a:
            break
    else:
        pytest.fail("no third version tells the twins apart")
    with codec.model_ledger(len(pa), 0, 0, workers=2, max_versions=3) as led:
        stage_all(led, [A, B, C])
        book = Book(oracle)
        run(book, led, [A, B], [0, 1])
        _, nd, st = run(book, led, [B, A], [0, 1])
        assert list(st) == [2, 2] and list(nd) == [0.0, 0.0]
        assert led.version(0) == A.id and same_bits(led.read(0), A.row)
        assert led.version(1) == B.id and same_bits(led.read(1), B.row)
        _, nd, st = run(book, led, [C, C], [0, 1])
        assert list(st) == [3, 3] and nd[0] != nd[1]
        np.testing.assert_allclose(nd[0], oracle.norm(oracle.subtract(C.text, A.text)), rtol=1e-12, atol=0)
        np.testing.assert_allclose(nd[1], oracle.norm(oracle.subtract(C.text, B.text)), rtol=1e-12, atol=0)


# 4 ------------------------------------------------- a worker several times per update

@pytest.fixture(scope="module")
def trio(oracle):
    """A, its zero-norm twin B and a third version C, as (n_w, n_b, edges, [A, B, C])."""
    pa, pb = zero_twins(oracle, 509)
    rng = np.random.default_rng(4)
    pc = (pa + ordinary(rng, len(pa)) * np.float32(1e-2)).astype(np.float32)
    # the first three values as biases (there twice in getModelParams), the rest as weights
    vs = [Version(oracle, 10 + i, p[3:].copy(), p[:3].copy(), 2) for i, p in enumerate((pa, pb, pc))]
    return len(pa) - 3, 3, 2, vs


def test_a_worker_twice_and_three_times(codec, oracle, trio):
    n_w, n_b, edges, (A, B, C) = trio
    assert oracle.norm(oracle.subtract(B.text, A.text)) == 0.0 and A.text != B.text
    with codec.model_ledger(n_w, n_b, edges, workers=3, max_versions=3) as led:
        stage_all(led, [A, B, C])
        book = Book(oracle)
        # the earlier pick stores (first model), the later one is ignored against it
        _, _, st = run(book, led, [A, B], [0, 0])
        assert list(st) == [1, 2]
        # the earlier pick is ignored (B against A), so the later one is differenced against A
        _, _, st = run(book, led, [B, C], [0, 0])
        assert list(st) == [2, 3] and led.version(0) == C.id
        # the earlier pick stores, the later one is differenced against it; A -> C -> A: ordered pairs
        _, nd, st = run(book, led, [A, C, A], [0, 0, 0])
        assert list(st) == [3, 3, 3]
        # three picks of a worker without a model, the middle one ignored, beside another worker
        _, _, st = run(book, led, [A, C, B, A, C], [1, 2, 1, 2, 1])
        assert list(st) == [1, 1, 2, 3, 3]


@pytest.mark.parametrize("K", [65, 130])
def test_many_picks_over_few_workers(codec, oracle, trio, K):
    n_w, n_b, edges, vs = trio
    rng = np.random.default_rng(40 + K)
    with codec.model_ledger(n_w, n_b, edges, workers=10, max_versions=3) as led:
        stage_all(led, vs)
        book = Book(oracle)
        for _ in range(2):
            picks = [vs[i] for i in rng.integers(0, 3, K)]
            workers = [int(w) for w in rng.integers(-1, 10, K)]
            _, _, st = run(book, led, picks, workers)
        assert {0, 2, 3} <= set(int(s) for s in st)


def test_more_pairs_than_one_launch(codec, oracle):
    """12 versions over 10 workers and 130 picks: more distinct ordered pairs than one launch of
    fleet_acc_burst() = 64 takes."""
    n_w, n_b, edges = 90, 3, 2
    rng = np.random.default_rng(41)
    vs = make_versions(oracle, rng, 12, n_w, n_b, edges)
    with codec.model_ledger(n_w, n_b, edges, workers=10, max_versions=12) as led:
        stage_all(led, vs)
        book = Book(oracle)
        run(book, led, [vs[i % 12] for i in range(10)], list(range(10)))
        picks = [vs[i] for i in rng.integers(0, 12, 130)]
        workers = [int(w) for w in rng.integers(0, 10, 130)]
        pairs = set()
        held = {w: {book.models[w].id} for w in range(10)}
        for v, w in zip(picks, workers):
            pairs |= {(v.id, p) for p in held[w]}
            held[w].add(v.id)
        assert len(pairs) > F.ACC_BURST
        run(book, led, picks, workers)


# 5 --------------------------------------------------- out-of-domain and non-finite

SPECIALS = np.array([np.inf, -np.inf, np.nan, 2e9, -3e8, 1e8, 1e-40, -1e-40, 0.0, -0.0, 3e38, -2147483648.0],
                    np.float32)


def test_special_values(codec, oracle):
    n_w, n_b, edges = 600, 3, 2
    rng = np.random.default_rng(5)
    vs = make_versions(oracle, rng, 3, n_w, n_b, edges)
    for j, v in enumerate(vs):  # each special in every version at another place, and among the biases
        w, b = v.w.copy(), v.b.copy()
        w[rng.permutation(n_w)[: len(SPECIALS)]] = np.roll(SPECIALS, j)
        b[j] = SPECIALS[j]
        vs[j] = Version(oracle, v.id, w, b, edges)
    assert all(np.isfinite(v.row).all() for v in vs)  # the codec gives every value a finite decode
    np.testing.assert_allclose(oracle.decode_floats(oracle.encode_floats(np.array([np.inf, np.nan, 1e8], np.float32))),
                               [214748.34, 214748.34, 1.0000001e8], rtol=1e-6)
    with codec.model_ledger(n_w, n_b, edges, workers=3, max_versions=3) as led:
        stage_all(led, vs)
        for v in vs:
            assert same_bits(led.read_version(v.id), v.row)
        book = Book(oracle)
        run(book, led, vs, [0, 1, 2])
        _, nd, st = run(book, led, [vs[1], vs[2], vs[0], vs[2]], [0, 1, 2, 0])
        assert list(st) == [3, 3, 3, 3]
        # the premise of the module's note: these norms are large and finite, never NaN
        assert np.isfinite(nd).all() and (nd > 1e5).all()


# 6 ---------------------------------------------------------- eviction and capacity

def test_eviction_and_capacity(codec, oracle):
    n_w, n_b, edges = 40, 0, 0
    rng = np.random.default_rng(6)
    V = make_versions(oracle, rng, 6, n_w, n_b, edges)
    with codec.model_ledger(n_w, n_b, edges, workers=2, max_versions=2) as led:
        stage_all(led, V[:2])
        led.stage(V[2].id, V[2].w, V[2].b)  # a third version that no worker holds: the oldest leaves
        assert [led.resident(v.id) for v in V[:3]] == [False, True, True]
        book = Book(oracle)
        run(book, led, [V[1]], [0])  # worker 0 holds V1
        led.stage(V[3].id, V[3].w, V[3].b)  # unreferenced: V2, V3
        led.stage(V[4].id, V[4].w, V[4].b)  # V2 leaves; V1 is held and stays
        assert [led.resident(v.id) for v in V[:5]] == [False, True, False, True, True]
        # a pick naming an evicted id: rejected, outputs and ledger untouched
        ids = np.array([V[3].id, V[2].id], np.int64)
        wk = np.array([1, 0], np.int32)
        nm, nd, st = np.full(2, 7.0), np.full(2, 7.0), np.full(2, 9, np.uint8)
        rc = led._L.fleet_mledger_update(led._h, ids.ctypes.data, wk.ctypes.data, 2, nm.ctypes.data, nd.ctypes.data,
                                         st.ctypes.data)
        assert rc == F.FLEET_ERR_ARG and (nm == 7.0).all() and (nd == 7.0).all() and (st == 9).all()
        book.check_ledger(led)
        assert not led.has(1)
        # staging a resident version renews its age: V3, staged before V4, now outlives it
        led.stage(V[3].id, V[3].w, V[3].b)
        led.stage(V[5].id, V[5].w, V[5].b)
        assert [led.resident(v.id) for v in V] == [False, True, False, True, False, True]
        # forget releases the row: V1 is unreferenced now and the oldest
        led.forget(0)
        book.models.pop(0)
        book.check_ledger(led)
        assert led.resident(V[1].id)
        led.stage(V[0].id, V[0].w, V[0].b)
        assert [led.resident(v.id) for v in V] == [True, False, False, False, False, True]
        run(book, led, [V[0], V[5]], [0, 0])


# 7 ------------------------------------------------------------- argument contract

def test_argument_errors_before_launch(codec, oracle):
    n_w, n_b, edges = 30, 3, 2
    rng = np.random.default_rng(7)
    A, B, C = make_versions(oracle, rng, 3, n_w, n_b, edges)
    L = F.lib()
    h = C_.c_void_p(0x1234)
    for bad in ((n_w, n_b, edges, 0, 2), (n_w, n_b, edges, 2, 0), (n_w, n_b, -1, 2, 2), (0, 0, 0, 2, 2), (0, 5, 0, 2, 2)):
        assert L.fleet_mledger_create(codec._h, *bad, C_.byref(h)) == F.FLEET_ERR_ARG and not h.value, bad
        h = C_.c_void_p(0x1234)
    assert L.fleet_mledger_create(None, n_w, n_b, edges, 2, 2, C_.byref(h)) == F.FLEET_ERR_ARG
    assert L.fleet_mledger_create(codec._h, n_w, n_b, edges, 2, 2, None) == F.FLEET_ERR_ARG
    with codec.model_ledger(n_w, n_b, edges, workers=3, max_versions=2) as led:
        stage_all(led, [A, B])
        book = Book(oracle)
        run(book, led, [A], [0])
        ids = np.array([A.id, B.id], np.int64)
        wk = np.array([1, 0], np.int32)
        nm, nd, st = np.full(2, 7.0), np.full(2, 7.0), np.full(2, 9, np.uint8)
        good = [led._h, ids.ctypes.data, wk.ctypes.data, 2, nm.ctypes.data, nd.ctypes.data, st.ctypes.data]

        def rejected(args):
            assert L.fleet_mledger_update(*args) == F.FLEET_ERR_ARG
            assert (nm == 7.0).all() and (nd == 7.0).all() and (st == 9).all()
            book.check_ledger(led)
            assert not led.has(1) and not led.has(2)

        for i in (0, 1, 2, 4, 5, 6):  # each NULL in turn
            a = list(good)
            a[i] = None
            rejected(a)
        a = list(good)
        a[3] = -1
        rejected(a)
        for bad_worker in (3, 1000):
            wk[0] = bad_worker
            rejected(good)
        wk[0] = 1
        ids[1] = C.id  # never staged
        rejected(good)
        ids[1] = B.id
        # K = 0 and all workers < 0: nothing happens, nothing is written for K = 0
        assert L.fleet_mledger_update(led._h, ids.ctypes.data, wk.ctypes.data, 0, nm.ctypes.data, nd.ctypes.data,
                                      st.ctypes.data) == F.FLEET_OK
        assert (nm == 7.0).all() and (st == 9).all()
        wk[:] = -1
        ids[:] = -99
        assert L.fleet_mledger_update(*good) == F.FLEET_OK
        assert np.isnan(nm).all() and np.isnan(nd).all() and (st == 0).all()
        book.check_ledger(led)
        # the other entry points
        buf = np.full(led.n, 5.0, np.float32)
        vid = C_.c_int64(77)
        assert L.fleet_mledger_has(led._h, 3) == F.FLEET_ERR_ARG and L.fleet_mledger_has(led._h, -1) == F.FLEET_ERR_ARG
        assert L.fleet_mledger_version(led._h, 1, C_.byref(vid)) == F.FLEET_ERR_ARG and vid.value == 77
        assert L.fleet_mledger_forget(led._h, 1) == F.FLEET_ERR_ARG
        assert L.fleet_mledger_read(led._h, 1, buf.ctypes.data, led.n) == F.FLEET_ERR_ARG
        assert L.fleet_mledger_read(led._h, 0, buf.ctypes.data, led.n - 1) == F.FLEET_ERR_CAPACITY
        assert (buf == 5.0).all()
        assert L.fleet_mledger_stage(led._h, C.id, None, C.b.ctypes.data) == F.FLEET_ERR_ARG
        assert L.fleet_mledger_stage(led._h, C.id, C.w.ctypes.data, None) == F.FLEET_ERR_ARG
        assert not led.resident(C.id)
        with pytest.raises(ValueError):
            led.stage(C.id, C.w[:-1], C.b)
        # more picked versions that no worker holds than max_versions: forget leaves three of them
        run(book, led, [B], [1])
        led.stage(C.id, C.w, C.b)  # resident: A (worker 0), B (worker 1), C
        led.forget(0), led.forget(1)
        book.models.clear()
        ids3 = np.array([A.id, B.id, C.id], np.int64)
        wk3 = np.array([0, 1, 2], np.int32)
        nm3, nd3, st3 = np.full(3, 7.0), np.full(3, 7.0), np.full(3, 9, np.uint8)
        assert L.fleet_mledger_update(led._h, ids3.ctypes.data, wk3.ctypes.data, 3, nm3.ctypes.data, nd3.ctypes.data,
                                      st3.ctypes.data) == F.FLEET_ERR_ARG
        assert (nm3 == 7.0).all() and (st3 == 9).all()
        book.check_ledger(led)


# 8 ------------------------------------------------------- stage_model / version_id

@pytest.fixture(scope="module")
def session():
    return np.load(os.path.join(HERE, "golden", "session_mnist.npz"))


def stepped_model(codec, s, steps=3):
    m = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    m.initUpdater(s["lrates"])
    for i in range(steps):
        m.descentNative(bytes(s[f"merged{i}"]), int(s["batch"]), 2)
    return m


def test_stage_model_and_version_ids(codec, oracle, session):
    s = session
    m = F.Model(codec, bytes(s["init"]), distillation_mode=1)
    m.initUpdater(s["lrates"])
    assert m.version_id(0) == 0
    texts = {0: m.getModelParametersNative(0)}
    with m.kardam_ledger(workers=4, max_versions=4) as led:
        nw, nb, ge, _ = m.shape()
        assert (led.n_weights, led.n_biases, led.graph_edges) == (nw, nb, ge)
        assert led.stage_model(m, 0) == 0
        for i in range(3):
            m.descentNative(bytes(s[f"merged{i}"]), int(s["batch"]), 2)
            n = m.modelsSize()
            assert n == min(i + 2, 2)
            # the ids stay with their versions across the pop_front
            assert [m.version_id(v) for v in range(n)] == [i + 2 - n + v for v in range(n)]
            for v in range(n):
                vid = m.version_id(v)
                text = m.getModelParametersNative(v)
                assert texts.setdefault(vid, text) == text
                assert led.stage_model(m, v) == vid and led.resident(vid)
                assert same_bits(led.read_version(vid), oracle.decode_floats(text))
        with pytest.raises(F.FleetError):
            m.version_id(2)
        with pytest.raises(F.FleetError):
            m.version_id(-1)
        with pytest.raises(F.FleetError):
            led.stage_model(m, 2)
        assert sorted(texts) == [0, 1, 2, 3] and len(set(texts.values())) == 4
        # setModel over staged versions against the texts
        nm, nd, st = led.update([2, 3, 3], [0, 1, 0])
        assert list(st) == [1, 1, 3]
        np.testing.assert_allclose(nd[2], oracle.norm(oracle.subtract(texts[3], texts[2])), rtol=1e-12, atol=0)
        np.testing.assert_allclose(nm[0], oracle.norm(texts[2]), rtol=1e-12, atol=0)
    for shape in ((nw + 1, nb, ge), (nw, nb + 1, ge), (nw, nb, ge + 1)):
        with codec.model_ledger(*shape, workers=1) as other:
            with pytest.raises(F.FleetError):
                other.stage_model(m, 0)
            assert not other.resident(m.version_id(0))
    m.close()


# 9 --------------------------------- FleetUpdater: kardam_models against kardam_model

def test_updater_with_kardam_models_matches_the_callback_path(codec, oracle, session):
    """The same arrivals, picker and model through FleetUpdater(kardam_model=callback), which
    builds texts and subtracts them per pick, and FleetUpdater(kardam_models=model), which asks
    the model ledger once per update. The merged bytes, the gradient side, the keys and which
    picks set a model are identical; modelDiffNorm and the lips are the same getNorm summed in
    another order on each path (fleet_norm's partials against the ledger's), so they agree to
    the project's 1e-12 for a norm and not bit for bit: on one MI355X seven of the eight norms
    of this run came out bit-identical and one as 79403.83234368917 against 79403.83234368915."""
    from fleet_amd.layouts import MNIST
    from fleet_amd.updater import FleetUpdater, Kardam
    from test_gpu_pool import uploads_for
    lay = MNIST
    model = stepped_model(codec, session, steps=1)
    assert model.modelsSize() == 2
    rng = np.random.default_rng(9)
    w = rng.normal(0, 0.05, lay.n_weights).astype(np.float32)
    b = rng.normal(0, 0.05, lay.n_fc_bias).astype(np.float32)
    lrates = [0.05, 0.02, 0.01, 0.01]
    ups = uploads_for(oracle, lay, 12, seed=909)
    # (client, epoch) per arrival: client 1 twice in updates 2 and 4, client 4 too old for a model in update 3
    arrivals = [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1), (1, 0), (3, 2), (2, 1), (4, 0), (1, 3), (3, 3), (1, 2)]
    scripts = [[([2, 0, 1], []), ([1, 0, 2], []), ([0, 2, 1], []), ([0, 1, 2], [])] for _ in range(2)]

    def text_of(tau):
        n = model.modelsSize()
        v = n - 1 - tau
        return model.getModelParametersNative(v) if v >= 0 and n == 2 else None

    ka, kb = Kardam(codec, 6), Kardam(codec, 6)
    ua = FleetUpdater(codec, lay, 3, lrates, w, b, policy=1, stale_size=2, picker=lambda p, e: scripts[0].pop(0),
                      kardam=ka, kardam_model=text_of)
    ub = FleetUpdater(codec, lay, 3, lrates, w, b, policy=1, stale_size=2, picker=lambda p, e: scripts[1].pop(0),
                      kardam=kb, kardam_models=model)
    updates = 0
    for i, (cid, ep) in enumerate(arrivals):
        ga = ua.update(ups[i], [i % 10] * 10, ep, client_id=cid)
        gb = ub.update(ups[i], [i % 10] * 10, ep, client_id=cid)
        assert ga == gb and (ga is None) == (i % 3 != 2)
        if ga is None:
            continue
        updates += 1
        assert kb.models == {} and kb.model_ledger is not None  # the texts are never built
        assert kb.grad_diff_norm == ka.grad_diff_norm and kb.lips.keys() == ka.lips.keys()
        assert kb.model_diff_norm.keys() == ka.model_diff_norm.keys()
        for wk in ka.model_diff_norm:
            print(f"update {updates} worker {wk}: modelDiffNorm {kb.model_diff_norm[wk]!r} (ledger) "
                  f"{ka.model_diff_norm[wk]!r} (texts)")
            np.testing.assert_allclose(kb.model_diff_norm[wk], ka.model_diff_norm[wk], rtol=1e-12, atol=0)
        for wk in ka.lips:
            assert len(kb.lips[wk]) == len(ka.lips[wk])
            np.testing.assert_allclose(kb.lips[wk], ka.lips[wk], rtol=1e-12, atol=0)
        for wk in range(6):
            assert kb.model_ledger.has(wk) == (wk in ka.models), wk
            if wk in ka.models:
                assert same_bits(kb.model_ledger.read(wk), oracle.decode_floats(ka.models[wk])), wk
        assert np.array_equal(ua.weights, ub.weights)
        model.descentNative(ga, 8, 2)  # a new version for the next update, for both paths
    assert updates == 4 and scripts == [[], []]
    assert sorted(ka.lips) == [1, 2, 3] and len(ka.lips[1]) >= 2 and not kb.model_ledger.has(4)
    ub._mledger.close()
    model.close()
