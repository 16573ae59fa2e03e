#!/usr/bin/env python3
"""Kardam's filter on the upload pool (fleet_kfilter) against the ledger update it extends
and the per-pick host path it replaces, on one GPU.

In one process, alternating the measurements on the same uploads (bench.py's synthetic
workloads), per workload, by device events around the calls:

  (a) ledger_update_device          fleet_kledger_update_device of K = M resident picks,
                                    every worker known at another epoch;
  (b) filter_update_device          fleet_kfilter_update_device of the same picks with a
                                    lastGrad (k_pool_fold_kf: the ledger's work plus the
                                    extra Q stage and two sums per pick, and the copies
                                    into the caller's tensors), without the resolve;
  (c) filter_update_all_accept      (b) plus fleet_kfilter_resolve_device with every pick
                                    accepted (no fold is launched);
  (d) filter_update_one_rejected    (b) plus the resolve with the middle pick rejected
                                    (the refold: k_pool_fold without finish, k_acc_finish,
                                    k_acc_avg_row);
  (e) set_model                     fleet_kfilter_set_model of a model of as many values as
                                    the upload has, from the host, by the wall clock;
  (f) host_subtract_norm_per_pick   what the filter replaces: subtractNative + getNorm over
                                    two gradient texts for one pick, by the wall clock, and
                                    that times M.

Every figure is the minimum of `reps` with the median and the maximum beside it. No
fallback: without a GPU the script fails.

  python scripts/kfilter_latency.py [--workloads synth1m_256,mnist64] [--out FILE.json]
      # writes profiles/kfilter/kfilter_latency.json unless told otherwise
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from acc_latency import host_rows, spread  # noqa: E402


def measure(torch, codec, name, reps):
    import fleet_amd as F
    layout, M, L, rows, d = host_rows(torch, codec, name)
    n = F.b64_count(L)
    groups = (n + 2) // 3
    order = [int(s) for s in np.random.default_rng(M).permutation(M)]
    workers = list(range(M))
    lr = float(np.float32(0.05))
    pool = codec.pool(L, layout.header_positions(), M)
    for c in range(M):
        pool.put(c, rows[c].tobytes())
    merged = torch.zeros(16 * groups, dtype=torch.uint8, device="cuda")
    f32 = torch.zeros(3 * groups + 4, dtype=torch.float32, device="cuda")
    expect = pool.update(order, d)
    ledger, fledger = pool.ledger(M), pool.ledger(M)
    filt = fledger.filter(n, 0, 0)
    all_ok = [True] * M
    one_out = [k != M // 2 for k in range(M)]
    epoch = [0]

    def ledger_update():
        epoch[0] += 1
        return ledger.update_device(order, d, workers, [epoch[0]] * M, lr, merged, f32)

    def filter_update(accept):
        epoch[0] += 1
        v = filt.update_device(order, d, workers, [epoch[0]] * M, lr, merged, f32)
        if accept is not None and not filt.resolve_device(accept, merged, f32):
            raise RuntimeError("a resolve with accepted picks gave no average")
        return v

    ledger_update()
    filter_update(all_ok)  # every worker new; the filter has a lastGrad from here on
    if merged.cpu().numpy()[:L].tobytes() != expect or not filt.has_last:
        raise RuntimeError("the filter's first update differs from the pool's")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = {k: [] for k in ("ledger", "update", "all", "one")}

    def clock(ts, call, keep):
        a.record()
        v = call()
        b.record()
        b.synchronize()
        if keep:
            ts.append(a.elapsed_time(b) * 1e-3)
        return v

    for r in range(reps + 1):  # the measurements alternate
        ng, nd, st = clock(t["ledger"], ledger_update, r)
        out = clock(t["update"], lambda: filter_update(None), r)
        if not np.array_equal(out[0], ng) or not st.all() or np.isnan(out[4]).any():
            raise RuntimeError("the filter's ledger outputs differ from the ledger's")
        clock(t["all"], lambda: filter_update(all_ok), r)
        if merged.cpu().numpy()[:L].tobytes() != expect:
            raise RuntimeError("an all-accept resolve differs from the pool's update")
        clock(t["one"], lambda: filter_update(one_out), r)
    if merged.cpu().numpy()[:L].tobytes() == expect:
        raise RuntimeError("the refold left the optimistic result")
    # (e) set_model from the host
    w = np.random.default_rng(1).normal(0, 0.05, n).astype(np.float32)
    t_model = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        filt.set_model(w, np.zeros(0, np.float32))
        if r:
            t_model.append(time.perf_counter() - t0)
    # (f) the host path per pick: subtract + getNorm over two gradient texts
    p_text = codec.scalarMulNative(codec.getFlatGradient(rows[order[0]].tobytes()), d[0])
    last_text = codec.scalarMulNative(codec.getFlatGradient(rows[order[1]].tobytes()), d[1])
    t_host = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        codec.getNorm(codec.subtractNative(p_text, last_text))
        if r:
            t_host.append(time.perf_counter() - t0)
    filt.close(), fledger.close(), ledger.close(), pool.close()
    return {"workload": name, "M": M, "upload_bytes": L, "groups": groups, "picks_per_launch": F.ACC_BURST,
            "device": {"ledger_update_device": spread(t["ledger"]), "filter_update_device": spread(t["update"]),
                       "filter_update_all_accept": spread(t["all"]), "filter_update_one_rejected": spread(t["one"]),
                       "filter_update_over_ledger": min(t["update"]) / min(t["ledger"]),
                       "all_accept_over_ledger": min(t["all"]) / min(t["ledger"]),
                       "one_rejected_over_ledger": min(t["one"]) / min(t["ledger"])},
            "host": {"set_model": spread(t_model), "subtract_norm_per_pick": spread(t_host),
                     "subtract_norm_times_M_ms": min(t_host) * 1e3 * M}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="synth1m_256,mnist64")
    ap.add_argument("--reps", type=int, default=0, help="0: 7 for the large workload, 30 for the small")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfilter", "kfilter_latency.json"))
    a = ap.parse_args()
    import torch
    import fleet_amd as F
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device paths only")
    codec = F.Codec(0)
    runs = []
    for run in range(2):  # the whole set twice: the second run shows the spread between runs
        runs.append([measure(torch, codec, name, a.reps or (7 if name.startswith("synth") else 30))
                     for name in a.workloads.split(",")])
    doc = {"device": torch.cuda.get_device_name(0), "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
