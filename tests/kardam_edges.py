"""Shared inputs of the Kardam edge tests (test_gpu_kardam_edges.py on the GPU,
test_kardam_edges_inputs.py on the CPU): uploads whose Kardam stage inputs leave the table
stages' domain -1e8 < x < 1e9, the learning rates that put them there, and the expected
values of every case as the oracle's per-op chain. A plain module: it holds no test.

Kardam's bookkeeping quantises three times, each stage with a table path and a per-lane
fallback to the general codec behind a wave ballot:
  G = Q(f32(f64(p) * lr))   every form          leaves the domain by lr > 1
  D = Q(G - prev)           every form          leaves it as a difference of two G
  E = Q(p - lastGrad)       the filter          leaves it as a difference of p and an average
p itself never does: it is a Q output, and Base64::encode saturates what it cannot hold. The
finish stage Q(f32(f64(A) * inv)) of the filter's average never does either: A is a Q output
and inv = 1 / accepted <= 1 (test_kardam_edges_inputs.py counts both over every case here:
0 and 0).

The cases are scripts (lists of updates) that both test modules replay: the GPU module runs
each update on the device against the values the replay expects, the CPU module counts what
the replay's stage inputs reach. Expected values come from test_gpu_kledger.Book and
test_gpu_kfilter.Chain -- flat_gradient, scalar_mul, subtract, add, norm, decode_floats --
and oracle.update_faithful; no device path computes one."""
import math

import numpy as np

import layout_axis as A
from fleet_amd.layouts import synthetic
from test_gpu_gate import EXTREME
from test_gpu_kfilter import Chain
from test_gpu_kledger import Book
from test_gpu_pool import MIXED, uploads_for

# magnitudes at the edges of the domain: inside it one by one, outside it as differences,
# and, times a rate above 1, as products
EDGE_VALUES = np.array([9e7, -9e7, 6e7, -6e7, 9.9e8, -9.9e7, 1e8, -1e8, 99999999.0, 9.99999e8], np.float32)
ROTATE = 3  # upload c holds the values rotated by 3 c and, for odd c, negated
TINY_VALUES = np.array([9.9e8, -9e7], np.float32)  # for the layouts of one to four payload slots

# binary32 (dampen_stage's f32 multiply); not binary32 (its f64 multiply); p * lr leaves the
# domain; p * lr overflows to +-inf for large p and passes 1e9 for gradient-sized p
LRS = (float(np.float32(0.05)), 1 / 3, 16.0, 1e32)
LR_IDS = ("lr0.05", "lr1over3", "lr16", "lr1e32")
DAMPENS = MIXED + (2.0,)


def dampens(K, turn=0):
    return [DAMPENS[(k + turn) % len(DAMPENS)] for k in range(K)]


def out_of_domain(x):
    """Where a stage input leaves the table stages' domain (NaN and +-inf do)."""
    x = np.asarray(x)
    return ~((x > np.float32(-1e8)) & (x < np.float32(1e9)))


def payload_mask(lay):
    m = np.ones(lay.n_up, bool)
    m[lay.header_positions()] = False
    return m


def edge_slots(lay):
    """The upload positions that carry edge values. A wave of the stream and pool kernels is
    64 consecutive groups of 3 values: the even waves carry them, and the last wave (the
    ragged last group is in it) once there are four, so an odd wave stays clean wherever
    there are two. Inside a carrying wave lane 4 i + 1 holds them in its three slots and
    lane 8 i + 4 in one, the others none. A layout in which the pattern meets no payload
    slot (synthetic(4): its one payload slot is in lane 0) carries them in every one."""
    pay = payload_mask(lay)
    pos = np.arange(lay.n_up)
    g = pos // 3
    lane, wave = g % 64, g // 64
    n_waves = (A.groups_of(lay.n_up) + 63) // 64
    carrying = (wave % 2 == 0) | ((wave == n_waves - 1) & (n_waves >= 4))
    in_lane = (lane % 4 == 1) | ((lane % 8 == 4) & (pos % 3 == (lane // 8) % 3))
    at = np.flatnonzero(pay & carrying & in_lane)
    return at if len(at) else np.flatnonzero(pay)


_edge = {}


def edge_uploads(oracle, layout, M, seed):
    """M uploads of the synthetic mix with EDGE_VALUES written over edge_slots(layout):
    upload c holds them rotated by ROTATE * c and negated for odd c, so the difference of
    two uploads leaves the domain where neither does; every seventh edge slot then gets one
    of the gate's EXTREME codes (|dec(code)| >= 1e9) through encode_ints."""
    out = []
    at = edge_slots(layout)
    j = np.arange(len(at))
    for c in range(M):
        key = (layout, seed, c)
        if key not in _edge:
            v = oracle.synth_upload(seed, c, list(layout.w_sizes), list(layout.b_sizes))
            if len(at) < len(EDGE_VALUES):  # synthetic(4 .. 7): 9.9e8 and -9e7 in turn, over slots and uploads
                v[at] = TINY_VALUES[(j + c) % 2]
            else:
                v[at] = EDGE_VALUES[(j + ROTATE * c) % len(EDGE_VALUES)] * np.float32(-1.0 if c % 2 else 1.0)
            codes = oracle.decode_ints(oracle.encode_floats(v)).copy()
            if len(at) >= len(EDGE_VALUES):
                ext = at[(c % 7)::7]
                codes[ext] = EXTREME[(np.arange(len(ext)) + c) % len(EXTREME)]
            _edge[key] = oracle.encode_ints(codes)
        out.append(_edge[key])
    return out


def plain_uploads(oracle, layout, M, seed):
    return uploads_for(oracle, layout, M, seed)


def scatter(flat, lay, fill=0.0):
    """flat (getFlatGradient order) -> upload coordinates, header slots `fill`."""
    out = np.full(lay.n_up, fill, np.float32)
    out[payload_mask(lay)] = flat
    return out


class Stages:
    """What the stage inputs of a replay reach. Per stage name ("p", "G", "D", "E", "F"): the
    number of inputs outside the domain, of infinite ones, and whether some evaluation (one
    pick of one update) had a wave of 64 groups that mixes lanes outside with lanes inside
    and, where the upload has more than one wave, a wave with none outside beside it."""

    def __init__(self, lay):
        self.lay = lay
        self.outside = {}
        self.inf = {}
        self.mixed_beside_clean = {}
        self.seen = {}

    def see(self, stage, x):
        """x: the stage's inputs in getFlatGradient order, float32."""
        x = np.asarray(x, np.float32)
        out = out_of_domain(x)
        self.seen[stage] = self.seen.get(stage, 0) + len(x)
        self.outside[stage] = self.outside.get(stage, 0) + int(out.sum())
        self.inf[stage] = self.inf.get(stage, 0) + int(np.isinf(x).sum())
        G = A.groups_of(self.lay.n_up)
        up = np.zeros(3 * G, bool)
        up[: self.lay.n_up][payload_mask(self.lay)] = out
        lanes = up.reshape(G, 3).any(axis=1)
        waves = [lanes[w: w + 64] for w in range(0, G, 64)]
        mixed = any(w.any() and not w.all() for w in waves)
        clean = len(waves) == 1 or any(not w.any() for w in waves)
        self.mixed_beside_clean[stage] = self.mixed_beside_clean.get(stage, False) or (mixed and clean)


def times(x, a):
    """scalarMultiply's product before its Q: (float)((double)x * a)."""
    with np.errstate(over="ignore"):
        return (np.asarray(x, np.float32).astype(np.float64) * a).astype(np.float32)


class EdgeBook(Book):
    """test_gpu_kledger.Book; with `stages`, its setGrad chain also reports the inputs of the
    G and D stages (and p, the G stage's operand) pick by pick."""

    def __init__(self, oracle, layout, stages=None):
        super().__init__(oracle, layout)
        self.stages = stages

    def set_grads(self, picked, dampen, workers, epochs, lr):
        out = []
        o = self.oracle
        for up, d, w, ep in zip(picked, dampen, workers, epochs):
            if self.stages is not None and w >= 0:
                p = o.decode_floats(o.scalar_mul(o.flat_gradient(up), d))
                self.stages.see("p", p)
                self.stages.see("G", times(p, lr))
                if w in self.grads and self.grads[w][1] != ep:
                    g = o.decode_floats(self.g_text(up, d, lr))
                    self.stages.see("D", g - o.decode_floats(self.grads[w][0]))
            out += super().set_grads([up], [d], [w], [ep], lr)  # a pick at a time: the same chain
        return out


class EdgeChain(Chain):
    """test_gpu_kfilter.Chain; with `stages`, the inputs of the E stage (norms) and of the
    finish stage A * inv (avg) are reported too."""

    def __init__(self, oracle, stages=None):
        super().__init__(oracle)
        self.stages = stages

    def norms(self, picked, d, last_avg):
        """[(norm_p, norm_pdiff or None)] per pick: what check_norms compares against."""
        o, out = self.o, []
        for up, dk in zip(picked, d):
            p = self.p(up, dk)
            if self.stages is not None:
                self.stages.see("p", o.decode_floats(p))
                if last_avg is not None:
                    self.stages.see("E", o.decode_floats(p) - o.decode_floats(last_avg))
            out.append((o.norm(p), None if last_avg is None else o.norm(o.subtract(p, last_avg))))
        return out

    def avg(self, picked, d, accept):
        if self.stages is not None and any(accept):
            o, a = self.o, None
            for up, dk, ok in zip(picked, d, accept):
                if ok:
                    a = self.p(up, dk) if a is None else o.add(a, self.p(up, dk))
            self.stages.see("F", times(o.decode_floats(a), 1.0 / sum(accept)))
        return super().avg(picked, d, accept)


# -- a: the batch form ----------------------------------------------------------------
BATCH_SIZES = ((3001, 4), (50_003, 3))
ROUNDS = ("none", "alternate", "all")  # test_gpu_kardam_fused.check_side_outputs' rounds
_batch = {}


def batch_rounds(oracle, n_up, M, lr, stages=None):
    """The three rounds of check_side_outputs over edge uploads: per round a dict of the
    uploads, the factors, has (None in the first round), in_place, the merged bytes, the G
    texts and the norms ng[c], nd[c] (None: no norm). Computed once per (n_up, M, lr)."""
    key = (n_up, M, lr)
    if key in _batch and stages is None:
        return _batch[key]
    lay = synthetic(n_up)
    book = EdgeBook(oracle, lay, stages)
    rounds = []
    for r, kind in enumerate(ROUNDS):
        ups = edge_uploads(oracle, lay, M, 31 + r)
        d = dampens(M, r)
        has = None if kind == "none" else [c % 2 == 0 for c in range(M)] if kind == "alternate" else [True] * M
        # a book per round: worker c's previous G is the last round's, where has[c]
        if has is None:
            book.grads = {}
        else:
            book.grads = {c: g for c, g in book.grads.items() if has[c]}
        exp = book.set_grads(ups, d, list(range(M)), [r] * M, lr)
        rounds.append(dict(ups=ups, d=d, has=has, in_place=kind == "all", merged=oracle.update_faithful(ups, d),
                           g=[book.g_text(u, dk, lr) for u, dk in zip(ups, d)], ng=[e[0] for e in exp],
                           nd=[e[1] for e in exp]))
        book.grads = {c: (rounds[-1]["g"][c], r) for c in range(M)}
    _batch[key] = rounds
    return rounds


# -- b: the ledger ----------------------------------------------------------------------
POOL_SIZES = (159, 1001)  # one partial wave; two blocks and a ragged last group


def twice(K):
    """Workers 0 .. K - 2 and worker 0 again as the last pick."""
    return list(range(K - 1)) + [0]


def ledger_script(K):
    """[(order, dampen, workers, epochs)], order the indices into the case's 2 K uploads. The
    first update stores a G for workers 0 .. K - 1; in the second every pick has a prev, and
    its last pick names worker 0 again at another epoch: its prev is the G the first pick
    stored in the same update (for K = 66 in an earlier launch of it)."""
    return [(list(range(K)), dampens(K), list(range(K)), [0] * K),
            (list(range(K, 2 * K)), dampens(K, 1), twice(K), [1] * (K - 1) + [2])]


LEDGER_CASES = [(n_up, K, i) for n_up in POOL_SIZES for K in (3, 4) for i in range(len(LRS))] + \
               [(159, 66, 1), (159, 66, 2)]


def case_id(case):
    return f"n{case[0]}-K{case[1]}-{LR_IDS[case[2]]}"


# -- c: the filter ----------------------------------------------------------------------
def filter_script(K):
    """[(order, dampen, workers, epochs, accept)] over the case's 4 K uploads: no lastGrad;
    lastGrad an average of edge values; one pick rejected (the refold); an update that reads
    the refolded average."""
    gated = list(range(K))
    gated[1] = -1  # a Kardam-gated pick still has the filter's norms
    reject = [k != 1 for k in range(K)]
    return [(list(range(K)), dampens(K), list(range(K)), [0] * K, [True] * K),
            (list(range(K, 2 * K)), dampens(K, 1), list(range(K)), [1] * K, [True] * K),
            (list(range(2 * K, 3 * K)), dampens(K, 2), twice(K), [2] * (K - 1) + [3], reject),
            (list(range(3 * K, 4 * K)), dampens(K, 3), gated, [4] * K, [True] * K)]


FILTER_CASES = [(n_up, K, i) for n_up in POOL_SIZES for K in (3, 4) for i in range(len(LRS))]


# -- d: layout edges for the ledger and the filter ----------------------------------------
def layout_of(name):
    kind, n = name.split(":")
    return synthetic(int(n)) if kind == "syn" else A.dense(int(n))


# (layout, picks per update, payload, rate index). syn:3 has no payload slot, so no edge
# payload; the plain mix runs at the small binary32 rate, the edge payload at the rates that
# take the D / E and the G stage out of the domain.
LAYOUT_NAMES = [f"syn:{n}" for n in (3, 4, 5, 6, 7)] + [f"dense:{A.ACC_LDS_HDR}", f"dense:{A.ACC_LDS_HDR + 1}"]
LAYOUT_CASES = [(name, 3, "plain", 0) for name in LAYOUT_NAMES] + \
               [(name, 3, "edge", i) for name in LAYOUT_NAMES[1:] for i in (1, 2)] + \
               [("syn:99998", 5, "plain", 0), ("syn:99998", 5, "edge", 1), ("syn:99998", 5, "edge", 2)]


def layout_case_id(case):
    return f"{case[0].replace(':', '')}-K{case[1]}-{case[2]}-{LR_IDS[case[3]]}"


def case_uploads(oracle, lay, M, payload, seed):
    return (edge_uploads if payload == "edge" else plain_uploads)(oracle, lay, M, seed)


# -- the replay both modules run ---------------------------------------------------------
def replay_ledger(oracle, lay, ups, script, lr, stages=None):
    """Per update of a ledger script: dict(picked, d, workers, epochs, merged, outputs
    [(norm_g, norm_diff, set)], grads: the book after it)."""
    book = EdgeBook(oracle, lay, stages)
    steps = []
    for order, d, workers, epochs in script:
        picked = [ups[i] for i in order]
        outputs = book.set_grads(picked, d, workers, epochs, lr)
        steps.append(dict(order=order, picked=picked, d=d, workers=workers, epochs=epochs, outputs=outputs,
                          merged=oracle.update_faithful(picked, d), grads=dict(book.grads)))
    return steps


def replay_filter(oracle, lay, ups, script, lr, stages=None):
    """Per update of a filter script: replay_ledger's dict plus norms [(norm_p, norm_pdiff)],
    accept, and resolved: the merged bytes of the accepted picks."""
    book, chain = EdgeBook(oracle, lay, stages), EdgeChain(oracle, stages)
    steps, last = [], None
    for order, d, workers, epochs, accept in script:
        picked = [ups[i] for i in order]
        outputs = book.set_grads(picked, d, workers, epochs, lr)
        norms = chain.norms(picked, d, last)
        resolved = chain.merged(picked, d, accept)
        steps.append(dict(order=order, picked=picked, d=d, workers=workers, epochs=epochs, outputs=outputs,
                          merged=oracle.update_faithful(picked, d), grads=dict(book.grads), norms=norms,
                          accept=accept, resolved=resolved, last=last))
        new = chain.avg(picked, d, accept)
        last = new if new is not None else last
    return steps


def finite(values):
    return all(v is None or math.isfinite(v) for v in values)
