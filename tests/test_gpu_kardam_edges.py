"""Kardam's side outputs where a stage input leaves the table stages' domain: the batch form
(fleet_update_kardam_device: kardam_lane_step, kardam_items, the pipelined tiles), the
two-pass Codec.kardam_grads, the ledger (k_pool_fold_kd), the filter (k_pool_fold_kf) and
its refold (k_acc_finish + k_acc_avg_row), each on uploads and rates that take G = Q(p * lr),
D = Q(G - prev) and E = Q(p - lastGrad) through the per-lane fallback to the general codec
in some lanes of a wave and not in others (kardam_edges.py; test_kardam_edges_inputs.py
proves on the CPU that every case here reaches the stage it names). The ledger and the
filter also run the layout edges that decide their `flat` mask: uploads of 3 to 7 values,
header lists on both sides of kAccLdsHdr, a ragged last group in a grid of many blocks.

Every expected value is the oracle's per-op chain (kardam_edges.replay_*): merged bytes,
merged_f32 and the stored G rows bit for bit, norms within 1e-12 relative (an fp64 sum of
the same fp32 products in another order; the terms are non-negative, so large ones cancel
nothing). A norm that must be absent is NaN, one that must be there is not: both are asserted
before any comparison."""
import math

import numpy as np
import pytest
import torch

import fleet_amd as F
import kardam_edges as KE
from fleet_amd.layouts import synthetic
from test_gpu_kardam_fused import PLANS, scatter_flat
from test_gpu_kfilter import SHAPE, update_like_the_ledger
from test_gpu_kledger import Book, check_outputs, same_snapshot, snapshot
from test_gpu_pool import filled, same_bits, scrambled

pytestmark = pytest.mark.gpu


def check_norm(got, exp, what):
    if exp is None:
        assert math.isnan(got), what
    else:
        assert not math.isnan(got), what
        np.testing.assert_allclose(got, exp, rtol=1e-12, atol=1e-300, err_msg=what)


def device_rows(ups):
    L = len(ups[0])
    pitch = 16 * ((L + 15) // 16)
    host = np.zeros((len(ups), pitch), np.uint8)
    for c, u in enumerate(ups):
        host[c, :L] = np.frombuffer(u, np.uint8)
    return torch.from_numpy(host).cuda(), L, pitch


# a ------------------------------------------------------------------- the batch form

def run_batch(codec, oracle, n_up, M, lr):
    lay = synthetic(n_up)
    hpos = lay.header_positions()
    vpitch = n_up + 3
    prev_dev = None
    for r, rnd in enumerate(KE.batch_rounds(oracle, n_up, M, lr)):
        t, L, pitch = device_rows(rnd["ups"])
        merged = torch.zeros(pitch, dtype=torch.uint8, device="cuda")
        merged_f32 = torch.zeros(3 * (pitch // 16), dtype=torch.float32, device="cuda")
        # in_place: this round's G replaces prev in the same rows
        g_out = prev_dev if rnd["in_place"] else torch.zeros((M, vpitch), dtype=torch.float32, device="cuda")
        ng, nd = codec.update_kardam_device(t, L, rnd["d"], hpos, lr, merged, merged_f32, prev_dev, rnd["has"], g_out)
        codec.check()
        torch.cuda.synchronize()
        assert merged.cpu().numpy()[:L].tobytes() == rnd["merged"], (n_up, r)
        assert same_bits(merged_f32.cpu().numpy()[:n_up], oracle.decode_floats(rnd["merged"])), (n_up, r)
        G = g_out.cpu().numpy()[:, :n_up]
        for c in range(M):
            assert same_bits(G[c], scatter_flat(oracle.decode_floats(rnd["g"][c]), lay)), (n_up, r, c)
            check_norm(ng[c], rnd["ng"][c], f"norm_g[{c}] of round {r}, {n_up}")
            check_norm(nd[c], rnd["nd"][c], f"norm_diff[{c}] of round {r}, {n_up}")
        prev_dev = g_out


@pytest.mark.parametrize("lr", KE.LRS, ids=KE.LR_IDS)
@pytest.mark.parametrize("spec", [""] + PLANS)
def test_batch_form_under_every_plan(codec, oracle, plan, spec, lr):
    """The default plan and every forced one: the stream kernel's lanes, the flat tiles at
    each width, the classic and the pipelined tiles, over the three rounds of
    check_side_outputs (no prev, prev on every other client, prev on all and G in place)."""
    plan(spec)
    for n_up, M in KE.BATCH_SIZES:
        run_batch(codec, oracle, n_up, M, lr)


@pytest.mark.parametrize("lr", KE.LRS, ids=KE.LR_IDS)
@pytest.mark.parametrize("n_up,M", KE.BATCH_SIZES)
def test_two_pass_path_equals_the_oracle(codec, oracle, n_up, M, lr):
    """Codec.kardam_grads, the reference of test_gpu_kardam_fused.py and of the client-axis and
    layout-axis suites, pinned to the oracle at these values: the same G texts, the same norms."""
    prev = None
    for r, rnd in enumerate(KE.batch_rounds(oracle, n_up, M, lr)):
        prev_arg = None if rnd["has"] is None else [p if h else None for p, h in zip(prev, rnd["has"])]
        g, ng, nd = codec.kardam_grads(rnd["ups"], rnd["d"], lr, prev_arg)
        assert g == rnd["g"], r
        for c in range(M):
            check_norm(ng[c], rnd["ng"][c], f"norm_g[{c}] of round {r}")
            check_norm(nd[c], rnd["nd"][c], f"norm_diff[{c}] of round {r}")
        prev = rnd["g"]


# b ----------------------------------------------------------------------- the ledger

def book_at(oracle, lay, grads):
    book = Book(oracle, lay)
    book.grads = grads
    return book


def device_tensors(ups):
    G = (len(ups[0]) + 15) // 16
    return (torch.zeros(16 * G, dtype=torch.uint8, device="cuda"),
            torch.zeros(3 * G, dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("case", KE.LEDGER_CASES, ids=KE.case_id)
def test_ledger(codec, oracle, case):
    """Two updates over one ledger, the second with a prev for every pick and worker 0 twice
    (its second prev the G stored earlier in the same update; for K = 66 the two picks lie on
    either side of the 64-pick launch boundary). Ledger.update against the oracle;
    update_device on a twin ledger bit for bit the same."""
    n_up, K, i = case
    lr, lay = KE.LRS[i], synthetic(n_up)
    ups = KE.edge_uploads(oracle, lay, 2 * K, 1000 + n_up + K)
    where = scrambled(2 * K + 1, 2 * K, seed=K)
    mu, mf = device_tensors(ups)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with filled(codec, lay.header_positions(), ups, 2 * K + 1, where) as pool, pool.ledger(K) as ledger, \
            pool.ledger(K) as twin:
        for s in KE.replay_ledger(oracle, lay, ups, KE.ledger_script(K), lr):
            picks = [where[j] for j in s["order"]]
            merged, f32, ng, nd, st = ledger.update(picks, s["d"], s["workers"], s["epochs"], lr, want_f32=True)
            assert merged == s["merged"] and same_bits(f32, oracle.decode_floats(s["merged"]))
            check_outputs(s["outputs"], ng, nd, st)
            assert [math.isnan(x) for x in nd] == [o[1] is None for o in s["outputs"]]
            book_at(oracle, lay, s["grads"]).check_ledger(ledger)
            ng2, nd2, st2 = twin.update_device(picks, s["d"], s["workers"], s["epochs"], lr, mu, mf,
                                               stream=side.cuda_stream)
            assert same_bits(ng, ng2) and same_bits(nd, nd2) and (st == st2).all()  # bitwise: f64 as 2 x u32
            assert mu.cpu().numpy()[: len(ups[0])].tobytes() == merged and same_bits(mf.cpu().numpy()[: len(f32)], f32)
            assert same_snapshot(snapshot(ledger), snapshot(twin))


# c, d ------------------------------------------------------------------- the filter

def run_filter(codec, oracle, lay, ups, K, lr):
    """kardam_edges.filter_script on the device: every update beside a twin ledger
    (update_like_the_ledger: the shared outputs bit for bit), its norms and ledger outputs
    against the replay, the resolve's bytes against Chain.merged."""
    where = scrambled(4 * K + 1, 4 * K, seed=K)
    steps = KE.replay_filter(oracle, lay, ups, KE.filter_script(K), lr)
    with filled(codec, lay.header_positions(), ups, 4 * K + 1, where) as pool, pool.ledger(K) as ledger, \
            pool.ledger(K) as twin, ledger.filter(*SHAPE) as filt:
        for u, s in enumerate(steps):
            assert filt.has_last == (s["last"] is not None)
            picks = [where[j] for j in s["order"]]
            out = update_like_the_ledger(filt, twin, picks, s["d"], s["workers"], s["epochs"], lr)
            assert out[0] == s["merged"] and same_bits(out[1], oracle.decode_floats(s["merged"])), u
            check_outputs(s["outputs"], out[2], out[3], out[4])
            for k, (n_p, n_pdiff) in enumerate(s["norms"]):
                check_norm(out[5][k], n_p, f"norm_p[{k}] of update {u}")
                check_norm(out[6][k], n_pdiff, f"norm_pdiff[{k}] of update {u}")
            book_at(oracle, lay, s["grads"]).check_ledger(ledger)
            got = filt.resolve(s["accept"], want_f32=True)
            assert got[0] == s["resolved"] and same_bits(got[1], oracle.decode_floats(s["resolved"])), u
            if all(s["accept"]):
                assert got[0] == out[0]
    return steps


@pytest.mark.parametrize("case", KE.FILTER_CASES, ids=KE.case_id)
def test_filter(codec, oracle, case):
    """Four updates: no lastGrad; lastGrad an average of edge values, so E leaves the domain;
    one pick rejected (the refold of a state built from edge values); an update that reads
    the refolded average."""
    n_up, K, i = case
    lay = synthetic(n_up)
    run_filter(codec, oracle, lay, KE.edge_uploads(oracle, lay, 4 * K, 2000 + n_up + K), K, KE.LRS[i])


@pytest.mark.parametrize("case", KE.LAYOUT_CASES, ids=KE.layout_case_id)
def test_layout_edges(codec, oracle, case):
    """The layouts that decide `flat`, which the pool's own fold never reads: uploads of 3 to
    7 values (3: an empty flat gradient; 4: one flat slot), dense header lists at kAccLdsHdr
    and one more (header-only groups, the LDS against the global lookup), a ragged last
    group with live lanes in a grid of many blocks; the plain mix and the edge payload."""
    name, K, payload, i = case
    lay = KE.layout_of(name)
    ups = KE.case_uploads(oracle, lay, 4 * K, payload, 3000 + lay.n_up)
    steps = run_filter(codec, oracle, lay, ups, K, KE.LRS[i])
    if lay.n_flat == 0:  # every norm there is 0 (run_filter held the device to it), every row all zero
        assert all(x == 0.0 for s in steps for o in s["outputs"] for x in o[:2] if x is not None)
        assert all(not oracle.decode_floats(g).size for s in steps for g, _ in s["grads"].values())
