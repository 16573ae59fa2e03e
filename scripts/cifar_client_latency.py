#!/usr/bin/env python3
"""The client's gradients on the CIFAR-10 network on the device
(fleet_amd.cifar_client.resident_client_gradients_device: k_rgb_sample, k_rgb_sum, k_rgb_fc_sum)
for 64 clients of 100 samples on a resident model, by device events:

  rows          the fp32 rows alone
  rows+upload   the rows and their Base64 upload rows
  host mirror   tests/native/check_cifar_backward.cpp --mirror (cifar_backward.h in plain loops) on
                one core over ONE client, scaled to 64 and marked so, and compared in bits

Medians of --reps calls after two warm-up calls; the two sets alternate in one process, so the
spread between them is visible. No number here is a gate.

  python scripts/cifar_client_latency.py [--reps N] [--out FILE.json]
      # writes profiles/cifar_client/cifar_client_latency.json unless told otherwise
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

N, C, B, CLASSES = 2000, 64, 100, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="default: profiles/cifar_client/cifar_client_latency.json; '' writes no file")
    a = ap.parse_args()
    import torch
    import fleet_amd as F
    from fleet_amd import cifar_client as K
    from fleet_amd.client import client_shifts
    import cifar_grad_ref as G
    import cifar_ref as R
    import model_nets as M
    from client_grad_latency import median_ms
    from test_gpu_cifar import LAYERS
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device path only")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "cifar_client", "cifar_client_latency.json")
    codec = F.Codec(0)
    r = np.random.RandomState(1234)
    x = r.uniform(-1, 1, (N, 3072)).astype(np.float32)
    lab = r.randint(0, CLASSES, N).astype(np.int32)
    idx = r.randint(0, N, (C, B)).astype(np.int32)
    sh = client_shifts(1, C, B)
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    di, ds = torch.from_numpy(idx).cuda(), torch.from_numpy(sh).cuda()
    w, b = G.model(5, CLASSES)
    rm = F.ResidentModel(codec, M.mode0_text(LAYERS(CLASSES), R.B_SIZES[CLASSES], R.W_SIZES[CLASSES], w, b), 0,
                         max_versions=2)
    rm.initUpdater([0.05, 0.02])
    n = K.grad_len(CLASSES)
    grads = torch.empty(C, n, dtype=torch.float32, device="cuda")
    ups = torch.empty(C, 16 * ((n + 2) // 3), dtype=torch.uint8, device="cuda")

    def rows():
        K.resident_client_gradients_device(rm, CLASSES, None, dx, dl, idx=di, shifts=ds, grads=grads)

    def rows_uploads():
        K.resident_client_gradients_device(rm, CLASSES, None, dx, dl, idx=di, shifts=ds, grads=grads, uploads=ups)

    sets = {}
    for tag in ("a", "b"):
        sets[tag] = {"rows": median_ms(rows, a.reps), "rows+upload": median_ms(rows_uploads, a.reps)}
    codec.check()
    med = lambda t, k: sets[t][k]["median_ms"]  # noqa: E731
    doc = {"device": torch.cuda.get_device_name(0), "classes": CLASSES, "clients": C, "samples_per_client": B, "images": N,
           "what": "device events around one call, median; sets a and b alternate in one process", "sets": sets,
           "summary": {"device_ms": {k: med(k, "rows") for k in sets},
                       "device_with_uploads_ms": {k: med(k, "rows+upload") for k in sets},
                       "repeat_spread_ms": abs(med("a", "rows") - med("b", "rows")),
                       "device_us_per_sample": {k: med(k, "rows") * 1e3 / (C * B) for k in sets}}}
    d = tempfile.mkdtemp(prefix="cifar_client_latency_")
    exe = G.build_checker(d)
    if exe is not None:
        wv, bv = rm.export(0)
        t0 = time.perf_counter()
        (vec, _), = G.mirror(exe, d, [(CLASSES, wv, bv, x[idx[0]], lab[idx[0]], sh[0], 2.0)])
        ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(vec.view(np.uint32), grads[0].cpu().numpy().view(np.uint32)))
        doc["host_mirror_one_core"] = {"clients_run": 1, "ms_per_client": ms, "scaled_to_64_clients_ms": ms * C,
                                       "scaled": True, "build": "-O1 -g, as the tests build it",
                                       "clock": "host, process start and file I/O included",
                                       "bit_equal_to_the_device_row": same}
        doc["summary"]["host_mirror_scaled_over_device"] = {k: ms * C / med(k, "rows") for k in sets}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
