#!/usr/bin/env python3
"""The arrival gate (fleet_gate, k_pool_vet) against the pool's own update, on one GPU.

In one process on an otherwise idle GPU, on bench.py's synthetic uploads (1M floats and
MNIST), per workload:

  (a) vet_device        fleet_gate_vet_device of K = 1 and K = 64 resident slots, by device
                        events around the call, with and without the header codes;
  (b) update_device     fleet_pool_update_device over the same slots (K = 1 and 64): the
                        fold an update pays to find the same malformed upload;
  (c) put               fleet_gate_put (the ingress plus the vet of the slot, synchronous)
                        against fleet_pool_put + fleet_pool_drop, by the host's clock.

(a) and (b) alternate. Every figure is the median of `reps` with the minimum and the maximum
beside it, and the whole measurement runs twice in the process ("run1", "run2"). The vet's
results are checked against a host vet before anything is timed. No fallback: without a GPU
the script fails.

  python scripts/pool_vet_latency.py [--workloads synth1m_256,mnist64] [--out FILE.json]
      # writes profiles/pool_vet/pool_vet_latency.json unless told otherwise
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from acc_latency import host_rows, spread  # noqa: E402

KS = (1, 64)


def measure(torch, codec, name, reps):
    import fleet_amd as F
    layout, M, L, rows, d = host_rows(torch, codec, name)
    groups = (F.b64_count(L) + 2) // 3
    S = max(KS)
    assert M >= S
    pool = codec.pool(L, layout.header_positions(), S + 1)
    texts = [rows[c].tobytes() for c in range(S)]
    for c in range(S):
        pool.put(c, texts[c])
    gate, plain = pool.gate(layout.header_values()), pool.gate()
    merged = torch.zeros(16 * groups, dtype=torch.uint8, device="cuda")
    st = torch.zeros(S, dtype=torch.int32, device="cuda")
    ss = torch.zeros(S, dtype=torch.float64, device="cuda")
    mx = torch.zeros(S, dtype=torch.float32, device="cuda")
    host = gate.vet(list(range(S)))
    if any(v.status for v in host):
        raise RuntimeError("a synthetic upload was refused")
    gate.vet_device(list(range(S)), st, ss, mx)
    torch.cuda.synchronize()
    if ss.tolist() != [v.sumsq for v in host] or mx.tolist() != [v.max_abs for v in host] or any(st.tolist()):
        raise RuntimeError("the device form differs from the host form")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def clock(ts, call, keep):
        a.record()
        call()
        b.record()
        b.synchronize()
        if keep:
            ts.append(a.elapsed_time(b) * 1e-3)

    out = {"workload": name, "upload_bytes": L, "groups": groups, "slots_per_launch": F.ACC_BURST, "device": {}}
    for K in KS:
        slots = list(range(K))
        t_vet, t_plain, t_upd = [], [], []
        for r in range(reps + 1):  # the measurements alternate; the first round is not kept
            clock(t_vet, lambda: gate.vet_device(slots, st, ss, mx), r)
            clock(t_plain, lambda: plain.vet_device(slots, st, ss, mx), r)
            clock(t_upd, lambda: pool.update_device(slots, d[:K], merged), r)
        out["device"][f"K{K}"] = {"vet_device": spread(t_vet), "vet_device_no_header_codes": spread(t_plain),
                                  "pool_update_device": spread(t_upd),
                                  "vet_over_update_median": spread(t_vet)["median_ms"] / spread(t_upd)["median_ms"]}
    t_gate, t_put = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        v = gate.put(S, texts[0])
        t1 = time.perf_counter()
        pool.drop(S)
        t2 = time.perf_counter()
        pool.put(S, texts[0])
        t3 = time.perf_counter()
        pool.drop(S)
        if v != host[0]:
            raise RuntimeError("Gate.put's verdict differs from the vet of the same upload")
        if r:
            t_gate.append(t1 - t0)
            t_put.append(t3 - t2)
    out["host"] = {"gate_put": spread(t_gate), "pool_put": spread(t_put),
                   "gate_put_minus_pool_put_median_ms": spread(t_gate)["median_ms"] - spread(t_put)["median_ms"]}
    # per vet of K slots, from the shapes: the rows' 16 bytes per group; an update of K picks reads the same and writes 16
    out["algorithmic_bytes"] = {f"K{K}": {"vet": 16 * groups * K, "pool_update": 16 * groups * (K + 1)} for K in KS}
    gate.close()
    plain.close()
    pool.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="synth1m_256,mnist64")
    ap.add_argument("--reps", type=int, default=0, help="0: 15 for the large workload, 50 for the small")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_vet", "pool_vet_latency.json"),
                    help="'' writes no file")
    a = ap.parse_args()
    import torch
    import fleet_amd as F
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device paths only")
    codec = F.Codec(0)
    doc = {"device": torch.cuda.get_device_name(0), "clock": "device events (device), time.perf_counter (host)"}
    for run in ("run1", "run2"):
        doc[run] = [measure(torch, codec, name, a.reps or (15 if name.startswith("synth") else 50))
                    for name in a.workloads.split(",")]
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
