#!/usr/bin/env python3
"""The Kardam model ledger (fleet_mledger) against the per-pick host path of kardam.setModel,
on one GPU.

Per size (a model's weights, use_bias() biases and layer-graph edges; K picks of K workers),
with `stale_size` distinct versions and every worker known at another version than the one it
picks, so that every pick is a setModel that subtracts, takes the norm and stores. In one
process, alternating within each repetition:

  (a) host_per_pick       what FleetUpdater(kardam_model=...) does per pick: the picked
                          version's getModelParametersNative text (fleet_model_params: an encode
                          launch and the text copied to the host) and Kardam.set_model on it
                          (subtractNative + getNorm over two texts from the host), K times;
  (b) ledger              what FleetUpdater(kardam_models=...) does per update: the distinct
                          versions made resident under new ids (fleet_mledger_stage from host
                          vectors, as fleet_mledger_stage_model does) and one
                          ModelLedger.update of the K picks;
  (c) ledger_update_alone the ModelLedger.update of (b)'s shape with its versions resident, by
                          device events around the call (the call synchronises).

(a) and (b) are host clocks around work that ends in a device synchronise. Every figure is the
minimum of `reps` with the median and the maximum beside it; the first repetition is not
recorded. The norms of (a) and (b) are compared in every repetition (1e-12 relative: one
getNorm summed in two orders). The models are seeded N(0, 0.1) vectors, the versions small
steps from one another as sgd leaves them. No fallback: without a GPU the script fails.

  python scripts/model_ledger_latency.py [--sizes mnist64,cifar10_256] [--out FILE.json]
      # writes profiles/model_ledger/model_ledger_latency.json unless told otherwise
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
from acc_latency import spread  # noqa: E402

# name: (non-null W floats, use_bias() biases, layer-graph edges, picks): the MNIST network of
# fleet_amd/layouts.py (conv 8, 16, 48 maps and the softmax's 10 biases over 6 edges) and the
# CIFAR-10 one (conv 16, 64, fully connected 384, 192, 10 over 7 edges)
SIZES = {"mnist64": (200 + 128 + 19200 + 1920, 8 + 16 + 48 + 10, 6, 64),
         "cifar10_256": (432 + 9216 + 221184 + 73728 + 1920, 16 + 64 + 384 + 192 + 10, 7, 256)}


def measure(torch, codec, name, reps, stale_size):
    from fleet_amd.updater import Kardam
    n_w, n_b, edges, K = SIZES[name]
    S = stale_size
    rng = np.random.default_rng(K)
    w0, b0 = rng.normal(0, 0.1, n_w).astype(np.float32), rng.normal(0, 0.1, n_b).astype(np.float32)
    vers = [((w0 - np.float32(0.01 * j) * rng.normal(0, 0.1, n_w).astype(np.float32)).astype(np.float32),
             (b0 - np.float32(0.01 * j) * rng.normal(0, 0.1, n_b).astype(np.float32)).astype(np.float32)) for j in range(S)]
    workers = list(range(K))

    def picked(r):  # repetition r: worker k picks version (k + r) % S, and holds (k + r - 1) % S from the one before
        return [(k + r) % S for k in range(K)]

    # the state before repetition 0: worker k at version (k - 1) % S, on both paths
    kardam = Kardam(codec, K)
    texts = [codec.getModelParametersNative(w, b, edges) for w, b in vers]
    for k, j in enumerate(picked(-1)):
        kardam.models[k] = texts[j]
    led = codec.model_ledger(n_w, n_b, edges, K, max_versions=S)
    alone = codec.model_ledger(n_w, n_b, edges, K, max_versions=S)
    for j, (w, b) in enumerate(vers):
        led.stage(-1 - j, w, b)
        alone.stage(j, w, b)
    _, _, st = led.update([-1 - j for j in picked(-1)], workers)
    _, _, st2 = alone.update(picked(-1), workers)
    if not (st == 1).all() or not (st2 == 1).all():
        raise RuntimeError("the first models were not stored")
    t_host, t_led, t_alone = [], [], []
    a, b_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 1):
        pk = picked(r)
        # (a) per pick: the text, then setModel on it
        t0 = time.perf_counter()
        for k, j in enumerate(pk):
            w, b = vers[j]
            kardam.set_model(k, codec.getModelParametersNative(w, b, edges))
        t1 = time.perf_counter()
        # (b) per update: the distinct versions resident under this repetition's ids, one update
        ids = {}
        for j in pk:
            if j not in ids:
                ids[j] = r * S + j
                led.stage(ids[j], *vers[j])
        _, nd, st = led.update([ids[j] for j in pk], workers)
        t2 = time.perf_counter()
        # (c) the update alone
        a.record()
        _, nd2, st2 = alone.update(pk, workers)
        b_ev.record()
        b_ev.synchronize()
        if not (st == 3).all() or not (st2 == 3).all() or not np.array_equal(nd, nd2):
            raise RuntimeError("the ledger's update of known workers is not a set of every pick")
        host = np.array([kardam.model_diff_norm[k] for k in workers])
        if not np.allclose(nd, host, rtol=1e-12, atol=0):
            raise RuntimeError("the ledger's norms differ from the host path's")
        if r:
            t_host.append(t1 - t0)
            t_led.append(t2 - t1)
            t_alone.append(a.elapsed_time(b_ev) * 1e-3)
    out = {"size": name, "n_weights": n_w, "n_biases": n_b, "graph_edges": edges, "values": led.n, "picks": K,
           "workers": K, "stale_size": S, "distinct_versions_per_update": len(set(picked(0))),
           "host_per_pick_text_plus_set_model": spread(t_host), "ledger_stage_versions_plus_update": spread(t_led),
           "ledger_update_alone_device_events": spread(t_alone),
           "ledger_over_host": min(t_led) / min(t_host),
           "resident_device_bytes": {"rows_of_workers_plus_stale_size": led.resident_bytes}}
    led.close()
    alone.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="mnist64,cifar10_256")
    ap.add_argument("--reps", type=int, default=0, help="0: 20 for mnist64, 8 for cifar10_256")
    ap.add_argument("--stale-size", type=int, default=4)
    ap.add_argument("--out", default=None,
                    help="default: profiles/model_ledger/model_ledger_latency.json; '' writes no file")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "model_ledger", "model_ledger_latency.json")
    import torch
    import fleet_amd as F
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device paths only")
    codec = F.Codec(0)
    results = [measure(torch, codec, name, a.reps or (20 if name.startswith("mnist") else 8), a.stale_size)
               for name in a.sizes.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
