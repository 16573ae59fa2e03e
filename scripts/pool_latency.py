#!/usr/bin/env python3
"""The upload pool (fleet_pool) against the batch host path and the accumulator, on one GPU.

In one process, alternating the paths on the same uploads (bench.py's synthetic workloads,
the rows page-locked with fleet_host_register), per workload:

  post_arrival   time from the M-th upload being available on the host to the merged bytes
                 on the host:
                 (a) pool = the M-th fleet_pool_put + fleet_pool_update of all M slots (M - 1
                     uploads put before the clock, as they would have been while the server
                     waited for the M-th);
                 (b) batch = fleet_update_rows on the registered rows;
                 (c) accumulator = the M-th fleet_acc_push + fleet_acc_finish (M - 1 folded
                     before the clock).
  device_fold    (d) fleet_pool_update_device of K = M picks, by device events, beside the
                 accumulator's device fold in bursts of fleet_acc_burst() rows
                 (push_many_device, the last through push_finish_device) in the same loop.
  total          (e) all M puts + the update against that same batch call.
  resident       device bytes each path holds (from the shapes).

(b), (c) and the accumulator's fold are the baselines: code the pool does not change,
measured here beside it. Host clocks around the synchronous calls; the C entry points are
called on the rows in place. Every figure is the minimum of `reps` with the median and the
maximum beside it. The picks are a fixed scrambled order of the slots, the same for every
path (the batch and accumulator paths get the rows in that order). No fallback: without a
GPU the script fails.

  python scripts/pool_latency.py [--workloads synth1m_256,mnist64] [--out FILE.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
      python scripts/pool_latency.py --workloads synth1m_256 --trace-only   # a run of its own
  python scripts/pool_latency.py --kernel-stats synth1m_256=DIR/.../run_kernel_stats.csv --out FILE.json
      # adds k_pool_fold's average time and achieved TB/s (algorithmic bytes from the shapes)
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from acc_latency import HBM_PEAK, host_rows, spread  # noqa: E402


def measure(torch, codec, name, reps, trace_only=False):
    import fleet_amd as F
    layout, M, L, rows, d = host_rows(torch, codec, name)
    lib, groups = codec._L, (F.b64_count(L) + 2) // 3
    B = F.ACC_BURST
    # the pick order: a fixed scramble of the slots; upload c lives in slot c
    order = [int(s) for s in np.random.default_rng(M).permutation(M)]
    picked = np.ascontiguousarray(rows[order])  # the same uploads in pick order, for the batch and accumulator paths
    ptr = [rows[c].ctypes.data for c in range(M)]
    pptr = [picked[k].ctypes.data for k in range(M)]
    out = np.empty(L + 16, np.uint8)
    n = C.c_size_t(0)
    picks = np.ascontiguousarray(order, np.int32)
    dd = np.ascontiguousarray(d, np.float64)
    picks_at, dd_at, out_at = picks.ctypes.data, dd.ctypes.data, out.ctypes.data
    pool = codec.pool(L, layout.header_positions(), M)
    acc = codec.accumulator(L, layout.header_positions())

    def put(c):
        codec._check(lib.fleet_pool_put(pool._h, c, ptr[c], L))

    def update():
        codec._check(lib.fleet_pool_update(pool._h, picks_at, M, dd_at, out_at, len(out), C.byref(n), None))
        return out[:L].tobytes()

    def push(k):
        codec._check(lib.fleet_acc_push(acc._h, pptr[k], L, d[k]))

    def finish():
        codec._check(lib.fleet_acc_finish(acc._h, out_at, len(out), C.byref(n), None))
        return out[:L].tobytes()

    last = order[-1]  # the M-th arrival is the last pick for every path
    codec.register_host(picked)
    try:
        expect = codec.update_rows(picked, L, d)  # warm-up of the batch path (staging, allocations)
        for c in range(M):
            put(c)
        if update() != expect:
            raise RuntimeError("the pool's result differs from fleet_update_rows")
        for k in range(M):
            push(k)
        if finish() != expect:
            raise RuntimeError("the accumulator's result differs from fleet_update_rows")
        if trace_only:
            for _ in range(3):
                update()
            pool.close()
            acc.close()
            return None
        post_p, post_b, post_s, tot_p, tot_b = [], [], [], [], []
        for _ in range(reps):  # the paths alternate
            t0 = time.perf_counter()
            put(last)
            update()
            post_p.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            codec.update_rows(picked, L, d)
            post_b.append(time.perf_counter() - t0)
            for k in range(M - 1):
                push(k)
            t0 = time.perf_counter()
            push(M - 1)
            finish()
            post_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for c in range(M):
                put(c)
            update()
            tot_p.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            codec.update_rows(picked, L, d)
            tot_b.append(time.perf_counter() - t0)
    finally:
        codec.unregister_host(picked)
    # the device-resident forms, by device events: the pool's update of K = M picks over its
    # resident rows, and the accumulator's fold of the same rows in bursts of B
    pitch = 16 * groups
    dev = torch.zeros((M, pitch), dtype=torch.uint8, device="cuda")
    dev[:, :L] = torch.from_numpy(picked).cuda()
    merged = torch.zeros(pitch, dtype=torch.uint8, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_pool, dev_acc = [], []
    got = {}
    for r in range(reps + 1):
        a.record()
        pool.update_device(order, d, merged)
        b.record()
        b.synchronize()
        if r:
            dev_pool.append(a.elapsed_time(b) * 1e-3)
        else:
            got["pool"] = merged.cpu().numpy()[:L].tobytes()
            merged.zero_()
        a.record()
        i = 0
        while M - i > B:
            acc.push_many_device(dev[i: i + B], d[i: i + B])
            i += B
        acc.push_finish_device(dev[i:], d[i:], merged)
        b.record()
        b.synchronize()
        if r:
            dev_acc.append(a.elapsed_time(b) * 1e-3)
        else:
            got["acc"] = merged.cpu().numpy()[:L].tobytes()
            merged.zero_()
    if got["pool"] != expect or got["acc"] != expect:
        raise RuntimeError("a device-resident result differs from fleet_update_rows")
    pool.close()
    acc.close()
    launches = (M + B - 1) // B
    res_pool = (M + 1) * (16 * groups + 64) + 12 * groups + 64 + 4 * M
    res_acc = 2 * 12 * groups + 2 * 16 * groups
    res_batch = M * 16 * groups + 16 * groups + 8 * M
    return {
        "workload": name, "M": M, "upload_bytes": L, "groups": groups, "picks_per_launch": B,
        "post_arrival": {"pool_put_plus_update": spread(post_p), "batch_update_rows_registered": spread(post_b),
                         "accumulator_push_plus_finish": spread(post_s),
                         "pool_over_batch": min(post_p) / min(post_b), "pool_over_accumulator": min(post_p) / min(post_s)},
        "total": {"pool_M_puts_plus_update": spread(tot_p), "batch_update_rows_registered": spread(tot_b),
                  "pool_over_batch": min(tot_p) / min(tot_b)},
        "device_fold": {"pool_update_device_K_eq_M": spread(dev_pool),
                        "accumulator_device_fold_in_bursts_of_B": spread(dev_acc),
                        "pool_over_accumulator": min(dev_pool) / min(dev_acc)},
        "resident_device_bytes": {"pool_of_M_slots": res_pool, "accumulator": res_acc, "batch": res_batch},
        # per launch of B picks: 16 B row bytes, the 12-byte state read (not by an update's first launch) and
        # written (the finish form writes the 16-byte merged group instead); k_pool_fold: the mean over an
        # update's launches before the last
        "algorithmic_bytes": {"k_pool_fold": groups * (16 * B + 12 + (12 * (launches - 2) / (launches - 1)
                                                                      if launches > 1 else 0)),
                              "k_pool_fold_finish_form": groups * (16 * min(B, M - B * (launches - 1)) + (
                                  12 if launches > 1 else 0) + 16),
                              "update_of_M_picks": groups * (16 * M + 24 * (launches - 1) + 16)},
    }


def kernel_rates(stats_csv):
    """k_pool_fold's two forms from a rocprofv3 --kernel-trace --stats run of --trace-only over ONE workload."""
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            rows[r["Name"].split("(")[0]] = r
    names = {"k_pool_fold": lambda s: "k_pool_fold<false>" in s or "k_pool_foldILb0" in s,
             "k_pool_fold_finish_form": lambda s: "k_pool_fold<true>" in s or "k_pool_foldILb1" in s}
    out = {}
    for k, match in names.items():
        hit = next((v for s, v in rows.items() if match(s)), None)
        if hit is None and k == "k_pool_fold":
            continue  # an update of at most one launch's picks runs the finish form alone
        if hit is None:
            raise RuntimeError(f"{k} is not in {stats_csv}: the native kernel did not run")
        out[k] = {"calls": int(hit["Calls"]), "avg_us": float(hit["AverageNs"]) / 1e3, "min_us": float(hit["MinNs"]) / 1e3,
                  "max_us": float(hit["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="synth1m_256,mnist64")
    ap.add_argument("--reps", type=int, default=0, help="0: 5 for the large workload, 20 for the small")
    ap.add_argument("--trace-only", action="store_true", help="run the pool's update a few times and exit (under rocprofv3)")
    ap.add_argument("--kernel-stats", default="", help="WORKLOAD=CSV[,WORKLOAD=CSV]: rocprofv3 kernel stats of --trace-only runs")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import fleet_amd as F
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device paths only")
    codec = F.Codec(0)
    results = []
    for name in a.workloads.split(","):
        r = measure(torch, codec, name, a.reps or (5 if name.startswith("synth") else 20), a.trace_only)
        if r:
            results.append(r)
    if a.trace_only:
        print("trace-only run done")
        return
    stats = dict(p.split("=", 1) for p in a.kernel_stats.split(",") if p)
    for r in results:
        if r["workload"] in stats:
            k = kernel_rates(stats[r["workload"]])
            for kk, v in k.items():
                v["tb_s"] = r["algorithmic_bytes"][kk] / (v["avg_us"] * 1e-6) / 1e12
                v["fraction_of_8_tb_s"] = v["tb_s"] * 1e12 / HBM_PEAK
            r["kernels"] = k
    doc = {"device": torch.cuda.get_device_name(0), "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
