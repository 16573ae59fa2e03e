#!/usr/bin/env python3
"""The model resident in HBM (fleet_amd.ResidentModel) against the unchanged host model
(fleet_amd.Model), on one GPU, in one process, alternating within each repetition.

Per model (the MNIST network of tests/golden/session_mnist.npz; a CIFAR-10-size network of
306,480 weights with a synthetic text) and per DISTILLATION_MODE (1 and 0):

  (a) step_and_stage   from a merged gradient resident in HBM (its text and decodeFloat of it,
                       as update_device leaves them) to the new version resident and staged in
                       a Kardam model ledger. Resident: descent_device + stage_model (device to
                       device). Host: the merged text copied to the host, descentNative(text),
                       stage_model (host vectors to the device).
  (b) get_params       getParametersNative(newest) to the host.
  (c) get_model_params getModelParametersNative(newest) to the host.
  (d) resident bytes   the resident model's rows and its workspace.

All host clocks around work that ends in a device synchronise. Medians of `reps` with the
minimum and maximum beside them; the first repetition is not recorded. Both models take the
same steps, and every text of (b) and (c) is compared in every repetition. No fallback:
without a GPU the script fails.

  python scripts/resident_model_latency.py [--models mnist,cifar10] [--out FILE.json]
      # writes profiles/resident_model/resident_model_latency.json unless told otherwise
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from acc_latency import spread  # noqa: E402
from model_nets import header, lines  # noqa: E402  (the getParams text builders the tests use)

# the CIFAR-10 network of fleet_amd/layouts.py as a getParams header (the activation names are
# not read by the model state)
CIFAR10_LAYERS = [("I1", "input 32 32 3 identity"), ("C1", "convolution 3 16 1 elu"), ("P1", "max_pool 3 2"),
                  ("C2", "convolution 3 64 1 elu"), ("P2", "max_pool 4 4"), ("FC1", "fully_connected 384 elu"),
                  ("FC2", "fully_connected 192 elu"), ("FC3", "fully_connected 10 softmax")]
CIFAR10_DIMS = [(3, 3, 48), (3, 3, 1024), (576, 384, 1), (384, 192, 1), (192, 10, 1)]
CIFAR10_BIAS = [16, 64, 384, 192, 10]


def cifar10_texts(codec):
    rng = np.random.default_rng(10)
    sizes = [c * r * k for c, r, k in CIFAR10_DIMS]
    w = rng.normal(0, 0.05, sum(sizes)).astype(np.float32)
    b = rng.normal(0, 0.05, sum(CIFAR10_BIAS)).astype(np.float32)
    top = header(CIFAR10_LAYERS) + lines(b, CIFAR10_BIAS)
    dims = np.array(CIFAR10_DIMS, np.int32).reshape(-1)
    return {0: top + lines(w, sizes), 1: top + codec.model_weights_text(w, dims)}


def mnist_texts(codec):
    import fleet_amd as F
    s = np.load(os.path.join(ROOT, "tests", "golden", "session_mnist.npz"))
    init = bytes(s["init"])
    m = F.Model(codec, init, 1)
    w, b = m.export(-1)
    m.close()
    cut = init.index(b" \n%d\n" % len(w)) + 2
    top = init[:cut]
    return {0: top + lines(w, [200, 128, 19200, 1920]), 1: init}


def measure(torch, codec, oracle, name, layout, text, mode, reps, stale):
    import fleet_amd as F
    hm, rm = F.Model(codec, text, mode), F.ResidentModel(codec, text, mode, max_versions=stale)
    lrates = [1e-4]
    hm.initUpdater(lrates)
    rm.initUpdater(lrates)
    lh, lr = hm.kardam_ledger(4, stale), rm.kardam_ledger(4, stale)
    # the merged gradients in HBM: text rows and decodeFloat of them
    ups = [oracle.encode_floats(oracle.synth_upload(77 + i, i, list(layout.w_sizes), list(layout.b_sizes)))
           for i in range(2)]
    length = len(ups[0])
    n = F.b64_count(length)
    pitch = (length + 15) // 16 * 16 + 16
    d_text = torch.zeros((2, pitch), dtype=torch.uint8, device="cuda")
    for i, u in enumerate(ups):
        d_text[i, :length] = torch.from_numpy(np.frombuffer(u, np.uint8).copy()).cuda()
    d_f32 = torch.zeros((2, n + 3), dtype=torch.float32, device="cuda")
    codec.decode_device(d_text, length, d_f32)
    codec.check()
    t = {k: [] for k in ("step_r", "step_h", "params_r", "params_h", "a20_r", "a20_h")}
    clock = time.perf_counter
    for r in range(reps + 1):
        i = r % 2
        torch.cuda.synchronize()
        t0 = clock()
        rm.descent_device(d_f32[i], stale, n_values=n)
        lr.stage_model(rm, rm.modelsSize() - 1)
        t1 = clock()
        merged = d_text[i, :length].cpu().numpy().tobytes()
        hm.descentNative(merged, 8, stale)
        lh.stage_model(hm, hm.modelsSize() - 1)
        t2 = clock()
        v = rm.modelsSize() - 1
        pr = rm.getParametersNative(v)
        t3 = clock()
        ph = hm.getParametersNative(v)
        t4 = clock()
        ar = rm.getModelParametersNative(v)
        t5 = clock()
        ah = hm.getModelParametersNative(v)
        t6 = clock()
        if pr != ph or ar != ah or rm.version_id(v) != hm.version_id(v):
            raise RuntimeError("the resident model's texts differ from the host model's")
        if r:
            for k, d in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t6 - t5)):
                t[k].append(d)
    st = rm.stats()
    nw, nb, ge, _ = rm.shape()
    out = {"model": name, "distillation_mode": mode, "n_weights": nw, "n_biases": nb, "graph_edges": ge,
           "gradient_values": n, "stale_size": stale, "params_text_bytes": len(pr), "reps": reps,
           "step_and_stage": {"resident": spread(t["step_r"]), "host": spread(t["step_h"])},
           "get_params": {"resident": spread(t["params_r"]), "host": spread(t["params_h"])},
           "get_model_params": {"resident": spread(t["a20_r"]), "host": spread(t["a20_h"])},
           "resident_over_host_median": {
               "step_and_stage": float(np.median(t["step_r"]) / np.median(t["step_h"])),
               "get_params": float(np.median(t["params_r"]) / np.median(t["params_h"])),
               "get_model_params": float(np.median(t["a20_r"]) / np.median(t["a20_h"]))},
           "resident_device_bytes": {"rows": st["resident_bytes"], "workspace": st["workspace_bytes"]},
           "device_allocs": st["device_allocs"]}
    for x in (lh, lr, hm, rm):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="mnist,cifar10")
    ap.add_argument("--reps", type=int, default=0, help="0: 20 for mnist, 8 for cifar10")
    ap.add_argument("--stale-size", type=int, default=2)
    ap.add_argument("--out", default=None,
                    help="default: profiles/resident_model/resident_model_latency.json; '' writes no file")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "resident_model", "resident_model_latency.json")
    import torch
    import fleet_amd as F
    import pyoracle
    from fleet_amd.layouts import CIFAR10, MNIST
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device paths only")
    codec = F.Codec(0)
    oracle = pyoracle.Oracle()
    results = []
    for name in a.models.split(","):
        texts = mnist_texts(codec) if name == "mnist" else cifar10_texts(codec)
        layout = MNIST if name == "mnist" else CIFAR10
        for mode in (1, 0):
            results.append(measure(torch, codec, oracle, name, layout, texts[mode], mode,
                                   a.reps or (20 if name == "mnist" else 8), a.stale_size))
    doc = {"device": torch.cuda.get_device_name(0), "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
