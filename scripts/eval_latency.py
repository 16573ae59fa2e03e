#!/usr/bin/env python3
"""The evaluation (fleet_amd.ResidentModel.evaluate_device: the Driver's test() on the device)
against the launch it is judged by: Codec.teacher_forward_device over the same images from the
same weights -- one image per block, the same forward cost, code this change does not touch.

10,000 seeded images of 784 floats, resident in HBM, and the seeded MNIST model's newest
version. Measured, each the median of `reps` launches between device events after a warm-up:
  evaluate_device        B = 10,000 and B = 100 (where launch latency ends)
  teacher_forward_device B = 10,000 and B = 100
  Model.evaluate         B = 10,000, the host model, uploads included (a host clock)
  mojo on one core       where oracle/_ref is present: the reference's own forward over 200 of
                         the images (ReferenceModel.teacher_forward, the same arithmetic cost
                         per image), scaled to 10,000 and marked as scaled
The whole set is taken twice in one process, the measurements alternating (set "a", set "b"),
so that the spread of a repeat stands beside every ratio. No figure is fixed in advance.
No fallback: without a GPU the script fails.

  python scripts/eval_latency.py [--reps N] [--out FILE.json]
      # writes profiles/eval/eval_latency.json unless told otherwise
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 10000


def images(n, seed=1234):
    r = np.random.RandomState(seed)
    x = r.uniform(-1, 1, (n, 784)).astype(np.float32)
    return x, r.randint(0, 10, n).astype(np.int32)


def median_ms(fn, reps, warm=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="default: profiles/eval/eval_latency.json; '' writes no file")
    a = ap.parse_args()
    import torch
    import fleet_amd as F
    import eval_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device path only")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "eval", "eval_latency.json")
    codec = F.Codec(0)
    x, lab = images(N)
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    text = R.seeded_text()
    rm = F.ResidentModel(codec, text, 1, max_versions=2)
    hm = F.Model(codec, text, 1)
    for m in (rm, hm):
        m.initUpdater([0.1])
    dw, db = rm.version_tensors(0)
    probs = torch.empty(N, 10, dtype=torch.float32, device="cuda")
    outs = {B: rm.evaluate_device(dx[:B], dl[:B]) for B in (N, 100)}  # written again by every launch

    def ev(B):
        return lambda: rm.evaluate_device(dx[:B], dl[:B], out=outs[B])

    def teacher(B):
        return lambda: codec.teacher_forward_device(dw, db, dx[:B], probs[:B], temperature=1.0)

    sets = {}
    for tag in ("a", "b"):
        s = {}
        for B in (N, 100):
            s[f"evaluate_device/B{B}"] = median_ms(ev(B), a.reps)
            s[f"teacher_forward_device/B{B}"] = median_ms(teacher(B), a.reps)
        ts = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hm.evaluate(x, lab)
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        s[f"Model.evaluate/B{N}"] = {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)),
                                     "max_ms": float(np.max(ts)), "reps": len(ts), "clock": "host, uploads included"}
        sets[tag] = s
    codec.check()
    doc = {"device": torch.cuda.get_device_name(0), "images": N, "block_images": F.evaluate_block_images(),
           "what": "device events around one call, median; sets a and b alternate in one process", "sets": sets}
    import pyoracle
    if os.path.exists(pyoracle.REF_MODEL_SO):
        ref = pyoracle.ReferenceModel()
        w, b = hm.export(0)
        t0 = time.perf_counter()
        ref.teacher_forward(w, b, x[:200])
        per = (time.perf_counter() - t0) / 200
        doc["mojo_one_core"] = {"images_run": 200, "ms_per_image": per * 1e3, "scaled_to_10000_ms": per * N * 1e3,
                                "scaled": True}
    med = lambda t, k: sets[t][k]["median_ms"]  # noqa: E731
    rows = {}
    for B in (N, 100):
        e, t = f"evaluate_device/B{B}", f"teacher_forward_device/B{B}"
        rows[f"B{B}"] = {
            "evaluate_ms": {k: med(k, e) for k in sets}, "teacher_ms": {k: med(k, t) for k in sets},
            "teacher_over_evaluate": {k: med(k, t) / med(k, e) for k in sets},
            "repeat_spread_ms": {"evaluate": abs(med("a", e) - med("b", e)), "teacher": abs(med("a", t) - med("b", t))}}
    rows["host_model_over_resident_B10000"] = {k: med(k, f"Model.evaluate/B{N}") / med(k, f"evaluate_device/B{N}")
                                               for k in sets}
    if "mojo_one_core" in doc:
        rows["mojo_scaled_over_resident_B10000"] = {k: doc["mojo_one_core"]["scaled_to_10000_ms"] / med(k, f"evaluate_device/B{N}")
                                                    for k in sets}
    doc["summary"] = rows
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
