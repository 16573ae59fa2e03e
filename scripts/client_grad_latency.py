#!/usr/bin/env python3
"""The client's gradients on the device (fleet_amd.client.resident_client_gradients_device:
getGradients for a fleet of clients) against the host mirror of the same source on one core.

C = 64 clients of B = 100 samples (the reference client's mini-batch) over 10,000 seeded images
resident in HBM, every client on the seeded MNIST model's newest version, shifts drawn. Measured,
each the median of `reps` calls between device events after a warm-up:
  client_gradients_device        the fp32 rows alone
  client_gradients_device+upload the rows and their Base64 upload rows
  host mirror on one core        tests/native/check_client_grad.cpp --mirror (client_backward.h in
                                 plain loops, the reference's order of operations, -O2) over 2
                                 clients of 100 samples on a host clock, scaled to 64 and marked
                                 as scaled
The device set is taken twice in one process, the measurements alternating (set "a", set "b"),
so that the spread of a repeat stands beside every figure. No figure is fixed in advance and no
speed is promised. No fallback: without a GPU the script fails.

  python scripts/client_grad_latency.py [--reps N] [--out FILE.json]
      # writes profiles/client_grad/client_grad_latency.json unless told otherwise
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, C, B = 10000, 64, 100


def median_ms(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "reps": reps}


def host_mirror_ms(w, b, x, lab, idx, sh, clients=2):
    """the mirror program over `clients` clients: (ms per client, its vectors)"""
    clang = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"))
                  if c and os.path.exists(c)), None)
    if clang is None:
        return None, None
    d = tempfile.mkdtemp(prefix="client_grad_latency_")
    try:
        exe = os.path.join(d, "mirror")
        subprocess.check_call([clang, "-std=c++17", "-O2", "-mfma", "-ffp-contract=off",
                               os.path.join(ROOT, "tests", "native", "check_client_grad.cpp"), "-o", exe])
        pick = idx[:clients].reshape(-1)
        with open(os.path.join(d, "jobs.bin"), "wb") as fh:
            fh.write(np.int32(1).tobytes() + w.tobytes() + b.tobytes() + np.array([clients, B], np.int32).tobytes() +
                     np.float32(2.0).tobytes() + np.ascontiguousarray(x[pick]).tobytes() + lab[pick].tobytes() +
                     np.ascontiguousarray(sh[:clients]).tobytes())
        t0 = time.perf_counter()
        subprocess.check_call([exe, "--mirror", os.path.join(d, "jobs.bin"), os.path.join(d, "vec.out")])
        ms = (time.perf_counter() - t0) * 1e3
        return ms / clients, np.fromfile(os.path.join(d, "vec.out"), np.float32).reshape(clients, -1)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="default: profiles/client_grad/client_grad_latency.json; '' writes no file")
    a = ap.parse_args()
    import torch
    import fleet_amd as F
    from fleet_amd import client as K
    import eval_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device path only")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "client_grad", "client_grad_latency.json")
    codec = F.Codec(0)
    r = np.random.RandomState(1234)
    x = r.uniform(-1, 1, (N, 784)).astype(np.float32)
    lab = r.randint(0, 10, N).astype(np.int32)
    idx = r.randint(0, N, (C, B)).astype(np.int32)
    sh = K.client_shifts(1, C, B)
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    di, ds = torch.from_numpy(idx).cuda(), torch.from_numpy(sh).cuda()
    rm = F.ResidentModel(codec, R.seeded_text(), 1, max_versions=2)
    rm.initUpdater([0.1])
    grads = torch.empty(C, K.client_grad_len(), dtype=torch.float32, device="cuda")
    ups = torch.empty(C, 16 * ((K.client_grad_len() + 2) // 3), dtype=torch.uint8, device="cuda")

    def rows():
        K.resident_client_gradients_device(rm, None, dx, dl, idx=di, shifts=ds, grads=grads)

    def rows_uploads():
        K.resident_client_gradients_device(rm, None, dx, dl, idx=di, shifts=ds, grads=grads, uploads=ups)

    sets = {}
    for tag in ("a", "b"):
        sets[tag] = {"client_gradients_device": median_ms(rows, a.reps),
                     "client_gradients_device+upload": median_ms(rows_uploads, a.reps)}
    codec.check()
    doc = {"device": torch.cuda.get_device_name(0), "clients": C, "samples_per_client": B, "images": N,
           "what": "device events around one call, median; sets a and b alternate in one process",
           "sets": sets}
    w, b = rm.export(0)
    per_client, vec = host_mirror_ms(w, b, x, lab, idx, sh)
    med = lambda t, k: sets[t][k]["median_ms"]  # noqa: E731
    summary = {"device_ms": {k: med(k, "client_gradients_device") for k in sets},
               "device_with_uploads_ms": {k: med(k, "client_gradients_device+upload") for k in sets},
               "repeat_spread_ms": abs(med("a", "client_gradients_device") - med("b", "client_gradients_device")),
               "device_us_per_sample": {k: med(k, "client_gradients_device") * 1e3 / (C * B) for k in sets}}
    if per_client is not None:
        same = bool(np.array_equal(vec.view(np.uint32), grads[:len(vec)].cpu().numpy().view(np.uint32)))
        doc["host_mirror_one_core"] = {"clients_run": len(vec), "ms_per_client": per_client,
                                       "scaled_to_64_clients_ms": per_client * C, "scaled": True,
                                       "clock": "host, process start and file I/O included",
                                       "bit_equal_to_the_device_rows": same}
        summary["host_mirror_scaled_over_device"] = {k: per_client * C / med(k, "client_gradients_device") for k in sets}
    doc["summary"] = summary
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
