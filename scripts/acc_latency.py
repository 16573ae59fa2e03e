#!/usr/bin/env python3
"""Streaming aggregation (fleet_acc) against the batch host path, on one GPU.

In one process, alternating the two paths on the same uploads (bench.py's synthetic
workloads, the rows page-locked with fleet_host_register), per workload:

  post_arrival   time from the M-th upload being available on the host to the merged
                 bytes on the host: streaming = the M-th fleet_acc_push + fleet_acc_finish
                 (M - 1 uploads folded before the clock, as they would have been while
                 the server waited for the M-th); batch = fleet_update_rows on the
                 registered rows, the best host path without an accumulator.
  total          all M pushes + the finish against that same batch call: what streaming
                 costs in throughput.
  resident       device bytes each path holds (from the shapes; the accumulator's two
                 states and two rows against the batch call's M rows and outputs).

Host clocks around the synchronous calls; the device-resident fold (push_device /
finish_device) is timed with device events beside them. The C entry points are called
on the rows in place (no Python copy of an upload inside the clock). Every figure is
the minimum of `reps` with the median and maximum beside it (the spread of repeating
the identical call). No fallback: without a GPU the script fails.

  python scripts/acc_latency.py [--workloads synth1m_256,mnist64] [--out FILE.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
      python scripts/acc_latency.py --trace-only       # per-kernel times, a run of its own
  python scripts/acc_latency.py --kernel-stats DIR/.../run_kernel_stats.csv --out FILE.json
      # adds k_acc_push / k_acc_finish achieved TB/s (algorithmic bytes from the shapes)
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def spread(ts):
    return {"min_ms": min(ts) * 1e3, "median_ms": statistics.median(ts) * 1e3, "max_ms": max(ts) * 1e3, "reps": len(ts)}


def algorithmic_bytes(groups: int, M: int):
    """Per launch, from the shapes: a push reads the 16-byte group and (but for the first
    of a batch) the 12-byte state and writes 12; a finish reads 16 + 12 and writes the
    16-byte group (and, when asked, the 12 bytes of merged_f32: not in this tool's runs)."""
    return {"k_acc_push_first": groups * (16 + 12), "k_acc_push": groups * (16 + 12 + 12),
            "k_acc_push_mean_of_M": groups * (16 + 12 + 12) - groups * 12 / M, "k_acc_finish": groups * (16 + 12 + 16),
            "k_acc_finish_with_f32": groups * (16 + 12 + 16 + 12)}


def host_rows(torch, codec, name):
    import bench
    from fleet_amd.layouts import LAYOUTS
    lay_name, M, _ = bench.WORKLOADS[name]
    layout = LAYOUTS[lay_name]
    sh = bench.Shard(codec, torch, layout, M, 0, 1)
    sh.encode()
    torch.cuda.synchronize()
    L = sh.L
    rows = np.ascontiguousarray(sh.text.cpu().numpy()[:, :L])
    del sh
    torch.cuda.empty_cache()
    return layout, M, L, rows, bench.dampen_policy(M)


def measure(torch, codec, name, reps, trace_only=False):
    import fleet_amd as F
    layout, M, L, rows, d = host_rows(torch, codec, name)
    lib, groups = codec._L, (F.b64_count(L) + 2) // 3
    ptr = [rows[c].ctypes.data for c in range(M)]
    out = np.empty(L + 16, np.uint8)
    n = C.c_size_t(0)
    acc = codec.accumulator(L, layout.header_positions())

    def push(c):
        codec._check(lib.fleet_acc_push(acc._h, ptr[c], L, d[c]))

    def finish():
        codec._check(lib.fleet_acc_finish(acc._h, out.ctypes.data, len(out), C.byref(n), None))
        return out[:L].tobytes()

    codec.register_host(rows)
    try:
        expect = codec.update_rows(rows, L, d)  # warm-up of the batch path (staging, allocations)
        for c in range(M):  # and of the streaming one, checked against it
            push(c)
        if finish() != expect:
            raise RuntimeError("streaming result differs from fleet_update_rows")
        if trace_only:
            for _ in range(3):
                for c in range(M):
                    push(c)
                finish()
            return None
        post_s, post_b, tot_s, tot_b = [], [], [], []
        for _ in range(reps):  # the two paths alternate
            for c in range(M - 1):
                push(c)
            t0 = time.perf_counter()
            push(M - 1)
            finish()
            post_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            codec.update_rows(rows, L, d)
            post_b.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for c in range(M):
                push(c)
            finish()
            tot_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            codec.update_rows(rows, L, d)
            tot_b.append(time.perf_counter() - t0)
    finally:
        codec.unregister_host(rows)
    # the device-resident fold, by device events: M push_device + finish_device on rows in HBM
    pitch = 16 * groups
    dev = torch.zeros((M, pitch), dtype=torch.uint8, device="cuda")
    dev[:, :L] = torch.from_numpy(rows).cuda()
    merged = torch.zeros(pitch, dtype=torch.uint8, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms = []
    for r in range(reps + 1):
        a.record()
        for c in range(M):
            acc.push_device(dev[c], d[c])
        acc.finish_device(merged)
        b.record()
        b.synchronize()
        if r:
            dev_ms.append(a.elapsed_time(b) * 1e-3)
    if merged.cpu().numpy()[:L].tobytes() != expect:
        raise RuntimeError("device-resident streaming result differs from fleet_update_rows")
    acc.close()
    res_stream = 2 * 12 * groups + 2 * 16 * groups
    res_batch = M * 16 * groups + 16 * groups + 8 * M
    return {
        "workload": name, "M": M, "upload_bytes": L, "groups": groups,
        "post_arrival": {"streaming_push_plus_finish": spread(post_s), "batch_update_rows_registered": spread(post_b),
                         "streaming_over_batch": min(post_s) / min(post_b)},
        "total": {"streaming_M_pushes_plus_finish": spread(tot_s), "batch_update_rows_registered": spread(tot_b),
                  "streaming_over_batch": min(tot_s) / min(tot_b)},
        "device_resident_fold_M_pushes_plus_finish": spread(dev_ms),
        "resident_device_bytes": {"streaming": res_stream, "batch": res_batch, "batch_over_streaming": res_batch / res_stream},
        "algorithmic_bytes": algorithmic_bytes(groups, M),
    }


def kernel_rates(stats_csv, results):
    """Achieved TB/s of the two kernels from a rocprofv3 --kernel-trace --stats run of
    --trace-only (every workload's launches pooled by rocprofv3: meaningful for a run
    over ONE workload) and the algorithmic bytes of that workload."""
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            rows[r["Name"].split("(")[0]] = r
    out = {}
    for k in ("k_acc_push", "k_acc_finish"):
        hit = next((v for n, v in rows.items() if k in n), None)
        if hit is None:
            raise RuntimeError(f"{k} is not in {stats_csv}: the native kernels did not run")
        out[k] = {"calls": int(hit["Calls"]), "avg_us": float(hit["AverageNs"]) / 1e3, "min_us": float(hit["MinNs"]) / 1e3,
                  "max_us": float(hit["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="synth1m_256,mnist64")
    ap.add_argument("--reps", type=int, default=0, help="0: 5 for the large workload, 20 for the small")
    ap.add_argument("--trace-only", action="store_true", help="run the two paths a few times and exit (under rocprofv3)")
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
        M_big = name.startswith("synth")
        r = measure(torch, codec, name, a.reps or (5 if M_big else 20), a.trace_only)
        if r:
            results.append(r)
    if a.trace_only:
        print("trace-only run done")
        return
    stats = dict(p.split("=", 1) for p in a.kernel_stats.split(",") if p)
    for r in results:
        if r["workload"] in stats:
            k = kernel_rates(stats[r["workload"]], results)
            ab = r["algorithmic_bytes"]
            k["k_acc_push"]["tb_s"] = ab["k_acc_push_mean_of_M"] / (k["k_acc_push"]["avg_us"] * 1e-6) / 1e12
            k["k_acc_finish"]["tb_s"] = ab["k_acc_finish"] / (k["k_acc_finish"]["avg_us"] * 1e-6) / 1e12
            for v in k.values():
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
