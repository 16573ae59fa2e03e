#!/usr/bin/env python3
"""The Kardam ledger (fleet_kledger) against the plain pool update and the batch path's
Kardam form, on one GPU.

In one process, alternating the measurements on the same uploads (bench.py's synthetic
workloads), per workload:

  (a) ledger_update_device   fleet_kledger_update_device of K = M resident picks, every
                             worker known at another epoch (norm + diff + store for every
                             pick), by device events around the call;
  (b) pool_update_device     fleet_pool_update_device of the same picks;
  (c) batch_kardam_device    fleet_update_kardam_device over the same rows laid out
                             contiguously in pick order, with prev on every row and G
                             written over prev in place; beside it fleet_update_device over
                             those rows, the batch path's own plain form;
  (d) post_arrival           the M-th upload on the host to merged bytes and norms on the
                             host: fleet_pool_put + fleet_kledger_update (M - 1 uploads put
                             before the clock), beside fleet_pool_put + fleet_pool_update.

Every figure is the minimum of `reps` with the median and the maximum beside it. The picks
are a fixed scrambled order of the slots; worker k is pick k's. No fallback: without a GPU
the script fails. `--pool-only` measures (b) alone and asks nothing of the ledger, so it
also runs against a library built from a commit that predates the ledger
(FLEET_CODEC_LIB=...): k_pool_fold from two commits in one session.

  python scripts/pool_kardam_latency.py [--workloads synth1m_256,mnist64] [--out FILE.json]
      # writes profiles/pool_kardam/pool_kardam_latency.json unless told otherwise
  FLEET_CODEC_LIB=parent/libfleetcodec.so python scripts/pool_kardam_latency.py --pool-only --out FILE.json
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


def timed(torch, reps, call):
    """Device events around `call`, once unrecorded and then `reps` times."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for r in range(reps + 1):
        a.record()
        call(r)
        b.record()
        b.synchronize()
        if r:
            ts.append(a.elapsed_time(b) * 1e-3)
    return ts


def measure(torch, codec, name, reps, pool_only):
    import fleet_amd as F
    layout, M, L, rows, d = host_rows(torch, codec, name)
    groups = (F.b64_count(L) + 2) // 3
    hp = layout.header_positions()
    order = [int(s) for s in np.random.default_rng(M).permutation(M)]
    workers = list(range(M))
    lr = float(np.float32(0.05))
    pitch = 16 * groups
    pool = codec.pool(L, hp, M)
    for c in range(M):
        pool.put(c, rows[c].tobytes())
    merged = torch.zeros(pitch, dtype=torch.uint8, device="cuda")
    expect = pool.update(order, d)
    out = {"workload": name, "M": M, "upload_bytes": L, "groups": groups, "picks_per_launch": F.ACC_BURST}
    if pool_only:
        ts = timed(torch, reps, lambda r: pool.update_device(order, d, merged))
        if merged.cpu().numpy()[:L].tobytes() != expect:
            raise RuntimeError("the pool's device form differs from its host form")
        out["device"] = {"pool_update_device": spread(ts)}
        pool.close()
        return out
    ledger = pool.ledger(M)
    # the batch path: the rows in pick order, prev on every row, G in place
    picked = torch.zeros((M, pitch), dtype=torch.uint8, device="cuda")
    picked[:, :L] = torch.from_numpy(np.ascontiguousarray(rows[order])).cuda()
    vpitch = 3 * groups + 4
    prev = torch.zeros((M, vpitch), dtype=torch.float32, device="cuda")
    codec.update_kardam_device(picked, L, d, hp, lr, merged, None, None, None, prev)  # every row gets a G
    epoch = [0]

    def ledger_update(r):
        epoch[0] += 1
        return ledger.update_device(order, d, workers, [epoch[0]] * M, lr, merged)

    ng0, _, st0 = ledger_update(0)  # every worker new
    if st0.any() or merged.cpu().numpy()[:L].tobytes() != expect:
        raise RuntimeError("the ledger's first update differs from the pool's")
    t_led, t_pool, t_kd, t_plain = [], [], [], []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def clock(ts, call, keep):
        a.record()
        v = call()
        b.record()
        b.synchronize()
        if keep:
            ts.append(a.elapsed_time(b) * 1e-3)
        return v

    for r in range(reps + 1):  # the measurements alternate
        ng, nd, st = clock(t_led, lambda: ledger_update(r + 1), r)
        if not st.all() or np.isnan(nd).any() or not np.array_equal(ng, ng0):
            raise RuntimeError("the ledger's update of known workers is not a diff + store of every pick")
        clock(t_pool, lambda: pool.update_device(order, d, merged), r)
        bg, _ = clock(t_kd, lambda: codec.update_kardam_device(picked, L, d, hp, lr, merged, None, prev, [True] * M, prev), r)
        clock(t_plain, lambda: codec.update_device(picked, L, d, hp, merged), r)
        if not np.allclose(bg, ng, rtol=1e-12, atol=0):
            raise RuntimeError("the ledger's norms differ from the batch path's")
    if merged.cpu().numpy()[:L].tobytes() != expect:
        raise RuntimeError("a device-resident result differs from the pool's host form")
    # (d) the M-th arrival on the host to merged bytes and norms on the host
    last = order[-1]
    last_row = rows[last].tobytes()
    post_l, post_p = [], []
    for r in range(reps + 1):
        epoch[0] += 1
        t0 = time.perf_counter()
        pool.put(last, last_row)
        m = ledger.update(order, d, workers, [epoch[0]] * M, lr)[0]
        t1 = time.perf_counter()
        pool.put(last, last_row)
        m2 = pool.update(order, d)
        t2 = time.perf_counter()
        if m != expect or m2 != expect:
            raise RuntimeError("a host result differs")
        if r:
            post_l.append(t1 - t0)
            post_p.append(t2 - t1)
    ledger.close()
    pool.close()
    launches = (M + F.ACC_BURST - 1) // F.ACC_BURST
    out["device"] = {
        "ledger_update_device_diff_store": spread(t_led), "pool_update_device": spread(t_pool),
        "batch_update_kardam_device_prev_in_place": spread(t_kd), "batch_update_device": spread(t_plain),
        "ledger_over_pool": min(t_led) / min(t_pool), "batch_kardam_over_batch_plain": min(t_kd) / min(t_plain),
        "ledger_over_batch_kardam": min(t_led) / min(t_kd)}
    out["post_arrival"] = {"pool_put_plus_ledger_update": spread(post_l), "pool_put_plus_pool_update": spread(post_p),
                           "ledger_over_pool": min(post_l) / min(post_p)}
    # per update, from the shapes: the pool's bytes (pool_latency.py) plus 12 bytes of prev and 12 of G per (pick, group)
    out["algorithmic_bytes"] = {"pool_update_of_M_picks": groups * (16 * M + 24 * (launches - 1) + 16),
                                "ledger_update_of_M_picks": groups * (16 * M + 24 * (launches - 1) + 16 + 24 * M)}
    out["resident_device_bytes"] = {"ledger_slab_of_2M_rows": 2 * M * ((12 * groups + 15) // 16 * 16)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="synth1m_256,mnist64")
    ap.add_argument("--reps", type=int, default=0, help="0: 7 for the large workload, 30 for the small")
    ap.add_argument("--pool-only", action="store_true", help="Pool.update_device alone (also for a library without the ledger)")
    ap.add_argument("--out", default=None,
                    help="default: profiles/pool_kardam/pool_kardam_latency.json (none with --pool-only); '' writes no file")
    a = ap.parse_args()
    if a.out is None:
        a.out = "" if a.pool_only else os.path.join(ROOT, "profiles", "pool_kardam", "pool_kardam_latency.json")
    import torch
    import fleet_amd as F
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device paths only")
    codec = F.Codec(0)
    results = [measure(torch, codec, name, a.reps or (7 if name.startswith("synth") else 30), a.pool_only)
               for name in a.workloads.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("FLEET_CODEC_LIB", "") or "this tree's",
           "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
