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
  burst          beside those, alternating with them in the same repetitions: the batch
                 folded in bursts of K in {4, 16, 64, M} (fleet_acc_push_many, the last burst
                 through fleet_acc_push_finish), the post-arrival time of push_finish with
                 K = 1, and the device-resident fold in bursts of fleet_acc_burst() uploads
                 (push_many_device, the last through push_finish_device) against M
                 push_device calls. Compare them with the single-push lines of the same run.
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
      # adds k_acc_push / k_acc_finish / k_acc_push_many achieved TB/s (algorithmic bytes from
      # the shapes; the trace's bursts are launches of fleet_acc_burst() uploads each)
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

    # bursts: the C entry points on slices of one pointer / length / factor array
    B = F.ACC_BURST
    P = (C.c_void_p * M)(*ptr)
    lens = np.full(M, L, np.uint64)
    dd = np.ascontiguousarray(d, np.float64)
    # (addresses taken once: numpy's .ctypes costs microseconds, which a 60 us call would show)
    p_at, lens_at, dd_at, out_at = C.addressof(P), lens.ctypes.data, dd.ctypes.data, out.ctypes.data

    def push_many(i, k):
        codec._check(lib.fleet_acc_push_many(acc._h, p_at + 8 * i, lens_at + 8 * i, k, dd_at + 8 * i))

    def push_finish(i, k):
        codec._check(lib.fleet_acc_push_finish(acc._h, p_at + 8 * i, lens_at + 8 * i, k, dd_at + 8 * i, out_at, len(out),
                                               C.byref(n), None))
        return out[:L].tobytes()

    def in_bursts(K):
        """The whole batch in bursts of K, the last one through push_finish."""
        i = 0
        while M - i > K:
            push_many(i, K)
            i += K
        return push_finish(i, M - i)

    burst_ks = sorted({k for k in (4, 16, 64, M) if k <= M})

    codec.register_host(rows)
    try:
        expect = codec.update_rows(rows, L, d)  # warm-up of the batch path (staging, allocations)
        for c in range(M):  # and of the streaming one, checked against it
            push(c)
        if finish() != expect:
            raise RuntimeError("streaming result differs from fleet_update_rows")
        for K in ([B] if trace_only else burst_ks + [1]):  # (a trace holds launches of B uploads alone)
            if in_bursts(K) != expect:
                raise RuntimeError(f"bursts of {K} differ from fleet_update_rows")
        if trace_only:
            for _ in range(3):
                for c in range(M):
                    push(c)
                finish()
                in_bursts(B)  # launches of B uploads each (M a multiple of B) for the kernel's bytes
            return None
        post_s, post_b, tot_s, tot_b = [], [], [], []
        post_f, tot_k = [], {K: [] for K in burst_ks}
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
            # the M-th arrival through the fused call (M - 1 uploads folded before the clock)
            if M > 1:
                push_many(0, M - 1)
            t0 = time.perf_counter()
            push_finish(M - 1, 1)
            post_f.append(time.perf_counter() - t0)
            for K in burst_ks:
                t0 = time.perf_counter()
                in_bursts(K)
                tot_k[K].append(time.perf_counter() - t0)
    finally:
        codec.unregister_host(rows)
    # the device-resident fold, by device events: M push_device + finish_device on rows in HBM
    pitch = 16 * groups
    dev = torch.zeros((M, pitch), dtype=torch.uint8, device="cuda")
    dev[:, :L] = torch.from_numpy(rows).cuda()
    merged = torch.zeros(pitch, dtype=torch.uint8, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms, dev_burst_ms = [], []
    for r in range(reps + 1):  # single device pushes and bursts of B alternate
        a.record()
        for c in range(M):
            acc.push_device(dev[c], d[c])
        acc.finish_device(merged)
        b.record()
        b.synchronize()
        if r:
            dev_ms.append(a.elapsed_time(b) * 1e-3)
        else:
            single = merged.cpu().numpy()[:L].tobytes()
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
            dev_burst_ms.append(a.elapsed_time(b) * 1e-3)
    if single != expect or merged.cpu().numpy()[:L].tobytes() != expect:
        raise RuntimeError("device-resident streaming result differs from fleet_update_rows")
    acc.close()
    res_stream = 2 * 12 * groups + 2 * 16 * groups
    launches = (M + B - 1) // B
    res_batch = M * 16 * groups + 16 * groups + 8 * M
    return {
        "workload": name, "M": M, "upload_bytes": L, "groups": groups,
        "post_arrival": {"streaming_push_plus_finish": spread(post_s), "batch_update_rows_registered": spread(post_b),
                         "streaming_over_batch": min(post_s) / min(post_b)},
        "total": {"streaming_M_pushes_plus_finish": spread(tot_s), "batch_update_rows_registered": spread(tot_b),
                  "streaming_over_batch": min(tot_s) / min(tot_b)},
        "device_resident_fold_M_pushes_plus_finish": spread(dev_ms),
        "burst": {
            "uploads_per_launch": B,
            "total_in_bursts_of_K_last_through_push_finish": {str(K): spread(ts) for K, ts in tot_k.items()},
            "bursts_of_16_over_single_pushes": min(tot_k[16]) / min(tot_s) if 16 in tot_k else None,
            "post_arrival_push_finish_K1": spread(post_f),
            "post_arrival_push_finish_over_push_plus_finish": min(post_f) / min(post_s),
            "device_resident_fold_in_bursts_of_B": spread(dev_burst_ms),
            "device_burst_fold_over_single_fold": min(dev_burst_ms) / min(dev_ms),
            # staging of a host burst: min(K - 1, B) window rows in HBM (and as many pinned on the host)
            "resident_device_bytes_with_staging": {str(K): res_stream + min(K - 1, B) * 16 * groups for K in burst_ks},
            # per launch of K = B uploads: 16 K row bytes, the 12-byte state read (not by a batch's first launch)
            # and written (the finish form writes the 16-byte merged group instead)
            "algorithmic_bytes": {"k_acc_push_many_K": B, "k_acc_push_many": groups * (16 * B + 12 + 12),
                                  "k_acc_push_many_mean_of_batch": groups * (16 * B + 12 + 12) - (
                                      groups * 12 / (launches - 1) if launches > 1 else 0),
                                  "k_acc_push_many_finish_form": groups * (16 * B + (12 if launches > 1 else 0) + 16)},
        },
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
    names = {"k_acc_push": lambda n: "k_acc_push" in n and "k_acc_push_many" not in n,
             "k_acc_finish": lambda n: "k_acc_finish" in n,
             "k_acc_push_many": lambda n: "k_acc_push_many<false>" in n or "k_acc_push_manyILb0" in n,
             "k_acc_push_many_finish_form": lambda n: "k_acc_push_many<true>" in n or "k_acc_push_manyILb1" in n}
    for k, match in names.items():
        hit = next((v for n, v in rows.items() if match(n)), None)
        if hit is None and k.startswith("k_acc_push_many"):
            continue  # a trace of a batch of at most one launch's uploads holds the finish form alone
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
            bb = r["burst"]["algorithmic_bytes"]
            for kk, key in (("k_acc_push_many", "k_acc_push_many_mean_of_batch"),
                            ("k_acc_push_many_finish_form", "k_acc_push_many_finish_form")):
                if kk in k:
                    k[kk]["tb_s"] = bb[key] / (k[kk]["avg_us"] * 1e-6) / 1e12
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
