"""The inputs of test_gpu_kardam_edges.py, validated without a GPU: the oracle's chain is
replayed for every case of that module and the stage inputs are counted, so each case
provably reaches the stage fallback it exists for.

What the counts show (DESIGN.md §4.4 states it next to the stages):
  G = Q(f32(f64(p) * lr))  outside the table domain at lr = 16 and 1e32, never at 0.05 or 1/3;
                           +-inf at 1e32;
  D = Q(G - prev)          outside at lr = 1/3, where every p * lr is inside;
  E = Q(p - lastGrad)      outside in every filter case with the edge payload;
  p                        never outside: Base64::encode saturates, getFlatGradient requantises
                           the crafted codes;
  A * inv (the finish)     never outside: A is a Q output and inv = 1 / accepted <= 1. It is
                           counted over every filter case here, refolds included, and is 0, so
                           the GPU module has no case for it.
At lr = 1e32 almost every lane is outside (a gradient-sized p times 1e32 is past 1e9), so the
mixed-wave-beside-clean-wave placement is asserted at the rates where placement decides it:
lr = 16 for G, lr = 1/3 for D, every rate for E."""
import numpy as np
import pytest

import kardam_edges as KE
from fleet_amd.layouts import synthetic


def check_rate(st, lr, placed):
    """The G / D conditions of a replay at rate lr; placed: the layout is large enough for
    the wave placement to mean something."""
    assert st.seen["p"] > 0 and st.outside["p"] == 0 and st.inf["p"] == 0
    if lr in (16.0, 1e32):
        assert st.outside["G"] > 0
    else:
        assert st.outside["G"] == 0
    if lr == 1e32:
        assert st.inf["G"] > 0
    if lr == 1 / 3:
        assert st.outside["D"] > 0
    if placed and lr == 16.0:
        assert st.mixed_beside_clean["G"]
    if placed and lr == 1 / 3:
        assert st.mixed_beside_clean["D"]


def test_the_domain_helper():
    x = np.array([-1e8, -99999992.0, 0.0, 9.99999e8, 1e9, np.inf, -np.inf, np.nan, 1e-45], np.float32)
    assert KE.out_of_domain(x).tolist() == [True, False, False, False, True, True, True, True, False]
    assert KE.LRS[0] == float(np.float32(KE.LRS[0])) and KE.LRS[1] != float(np.float32(KE.LRS[1]))
    assert KE.DAMPENS[-1] == 2.0 and len(KE.DAMPENS) == 7


@pytest.mark.parametrize("n_up", [159, 1001, 3001, 50_003, 99_998])
def test_edge_uploads_place_their_values(oracle, n_up):
    """Rotated and negated copies of the edge values in the carrying lanes of the carrying
    waves, the headers untouched, an odd wave clean, the ragged last group carrying."""
    lay = synthetic(n_up)
    at = KE.edge_slots(lay)
    ups = KE.edge_uploads(oracle, lay, 4, 5)
    plain = [oracle.synth_upload(5, c, list(lay.w_sizes), list(lay.b_sizes)) for c in range(4)]
    v = np.stack([oracle.decode_floats(u) for u in ups])
    hp = lay.header_positions()
    assert np.array_equal(v[:, hp], np.tile(np.asarray(lay.header_values(), np.float32), (4, 1)))
    rest = np.setdiff1d(np.arange(lay.n_up), at)
    for c in range(4):
        assert np.array_equal(v[c, rest], oracle.decode_floats(oracle.encode_floats(plain[c]))[rest])
        # the mix stops at 2^20; -1e8 and some crafted codes read back small, the others stay large
        assert np.abs(v[c, rest]).max() < 2.0 ** 21 and (np.abs(v[c, at]) > 5e7).mean() > 0.5
    codes = np.stack([oracle.decode_ints(u) for u in ups])
    assert all(np.isin(codes[c, at], KE.EXTREME).sum() >= len(at) // 7 for c in range(4))
    waves = (at // 3) // 64
    n_waves = (KE.A.groups_of(n_up) + 63) // 64
    if n_waves > 1:
        assert 1 not in waves and 0 in waves
    if n_waves >= 4:
        assert n_waves - 1 in waves and ((n_up - 2) // 3) // 64 == n_waves - 1  # the last payload slot's wave
    # as differences of two uploads' values they leave the domain where neither value does
    inside = ~KE.out_of_domain(v[0, at]) & ~KE.out_of_domain(v[1, at])
    assert (KE.out_of_domain(v[0, at] - v[1, at]) & inside).any()


@pytest.mark.parametrize("lr", KE.LRS, ids=KE.LR_IDS)
@pytest.mark.parametrize("n_up,M", KE.BATCH_SIZES)
def test_batch_cases_reach_their_stages(oracle, n_up, M, lr):
    st = KE.Stages(synthetic(n_up))
    rounds = KE.batch_rounds(oracle, n_up, M, lr, st)
    check_rate(st, lr, placed=True)
    assert [r["has"] is None for r in rounds] == [True, False, False]
    for r in rounds:
        assert KE.finite(r["ng"]) and KE.finite(r["nd"]) and all(x is not None for x in r["ng"])
        assert [x is not None for x in r["nd"]] == (r["has"] or [False] * M)


@pytest.mark.parametrize("case", KE.LEDGER_CASES, ids=KE.case_id)
def test_ledger_cases_reach_their_stages(oracle, case):
    n_up, K, i = case
    lay = synthetic(n_up)
    st = KE.Stages(lay)
    ups = KE.edge_uploads(oracle, lay, 2 * K, 1000 + n_up + K)
    steps = KE.replay_ledger(oracle, lay, ups, KE.ledger_script(K), KE.LRS[i], st)
    check_rate(st, KE.LRS[i], placed=True)
    first, second = steps
    assert all(not s and nd is None for _, nd, s in first["outputs"])
    assert all(s and nd is not None for _, nd, s in second["outputs"])  # a prev for every pick
    assert second["workers"][-1] == second["workers"][0] and second["epochs"][-1] != second["epochs"][0]
    for step in steps:
        assert KE.finite([x for o in step["outputs"] for x in o[:2]])
    if K == 66:
        assert second["workers"].index(0) < 64 <= K - 1  # stored in one launch, read in the next


@pytest.mark.parametrize("case", KE.FILTER_CASES, ids=KE.case_id)
def test_filter_cases_reach_their_stages(oracle, case):
    n_up, K, i = case
    lay = synthetic(n_up)
    st = KE.Stages(lay)
    ups = KE.edge_uploads(oracle, lay, 4 * K, 2000 + n_up + K)
    steps = KE.replay_filter(oracle, lay, ups, KE.filter_script(K), KE.LRS[i], st)
    check_rate(st, KE.LRS[i], placed=True)
    assert st.outside["E"] > 0 and st.mixed_beside_clean["E"]
    assert st.seen["F"] > 0 and st.outside["F"] == 0  # the finish stage stays inside (module docstring)
    assert steps[0]["last"] is None and all(s["last"] is not None for s in steps[1:])
    assert not all(steps[2]["accept"]) and any(steps[2]["accept"]) and steps[2]["resolved"] != steps[2]["merged"]
    assert steps[3]["last"] != steps[2]["last"] and -1 in steps[3]["workers"]
    for step in steps:
        assert KE.finite([x for o in step["outputs"] for x in o[:2]])
        assert KE.finite([x for n in step["norms"] for x in n])
        assert all((n[1] is None) == (step["last"] is None) for n in step["norms"])


@pytest.mark.parametrize("case", KE.LAYOUT_CASES, ids=KE.layout_case_id)
def test_layout_cases_reach_their_stages(oracle, case):
    name, K, payload, i = case
    lay = KE.layout_of(name)
    st = KE.Stages(lay)
    ups = KE.case_uploads(oracle, lay, 4 * K, payload, 3000 + lay.n_up)
    steps = KE.replay_filter(oracle, lay, ups, KE.filter_script(K), KE.LRS[i], st)
    assert st.outside["p"] == 0 and st.outside["F"] == 0
    for step in steps:
        assert KE.finite([x for o in step["outputs"] for x in o[:2]])
        assert KE.finite([x for n in step["norms"] for x in n])
    if lay.n_flat == 0:  # syn:3: an empty flat gradient, every norm 0
        assert all(x == 0.0 for s in steps for o in s["outputs"] for x in o[:2] if x is not None)
        assert all(x == 0.0 for s in steps for n in s["norms"] for x in n if x is not None)
    elif payload == "edge":
        check_rate(st, KE.LRS[i], placed=lay.n_up > 1000)
        assert st.outside["E"] > 0
    else:
        assert st.outside["G"] == 0 and st.outside["D"] == 0 and st.outside["E"] == 0
    if name.startswith("dense"):
        hp = lay.header_positions()
        assert len(hp) == int(name.split(":")[1]) and 7 in KE.A.header_bits(lay)  # header-only groups
    if name == "syn:99998":
        assert lay.n_up % 3 == 2 and KE.A.groups_of(lay.n_up) > 8 * 256  # a ragged last group, many blocks


def test_deleting_the_edge_values_is_noticed(oracle, monkeypatch):
    """The conditions above hang on the edge values: with none written, the same replay
    reaches no stage fallback at the rates up to 16."""
    monkeypatch.setattr(KE, "edge_slots", lambda lay: np.zeros(0, np.int64))
    monkeypatch.setattr(KE, "_edge", {})
    lay = synthetic(1001)
    for i in (0, 1, 2):
        st = KE.Stages(lay)
        ups = KE.edge_uploads(oracle, lay, 12, 2000 + 1001 + 3)
        KE.replay_filter(oracle, lay, ups, KE.filter_script(3), KE.LRS[i], st)
        assert st.outside["G"] == 0 and st.outside["D"] == 0 and st.outside["E"] == 0
