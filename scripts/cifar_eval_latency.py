#!/usr/bin/env python3
"""The CIFAR evaluation (fleet_amd.cifar.resident_evaluate_device: the Driver's test() on the
reference's CIFAR network, on the device) beside the two ways a user had before it.

10,000 seeded images of 3072 floats, resident in HBM, and a seeded mode-0 model, for the 10-class
and the 100-class head. Measured, each the median of `reps` launches between device events after
a warm-up:
  resident_evaluate_device  B = 10,000 and B = 100 (where launch latency ends)
  model_evaluate            B = 10,000, the host model: weights, images and labels uploaded by
                            the call (a host clock)
The whole set is taken twice in one process, the measurements alternating (set "a", set "b"), so
that the spread of a repeat stands beside every ratio. No figure is fixed in advance and none
gates anything. No fallback: without a GPU the script fails.

  python scripts/cifar_eval_latency.py [--reps N] [--out FILE.json]
      # writes profiles/cifar_eval/cifar_eval_latency.json unless told otherwise

mojo's own forward on one core needs the reference's sources, which a GPU machine need not hold:

  python scripts/cifar_eval_latency.py --mojo DIR [--mojo-images N] [--out FILE.json]
      # no GPU used: compiles tests/native/ref_cifar_driver.cpp against DIR/commonLib/cppNN into a
      # temporary directory with the reference's flags (-O0), times it over N images (default 300)
      # per head, scales to 10,000 and writes profiles/cifar_eval/mojo_one_core.json
"""
import argparse
import json
import os
import platform
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

N = 10000
LAYERS = lambda n: (("I1", "input 32 32 3 identity"), ("C1", "convolution 3 16 1 elu"), ("P1", "max_pool 3 2"),  # noqa: E731
                    ("C2", "convolution 3 64 1 elu"), ("P2", "max_pool 4 4"), ("local4", "fully_connected 384 relu"),
                    ("local5", "fully_connected 192 relu"), ("FC2", f"fully_connected {n} softmax"))


def images(n, classes, seed=1234):
    r = np.random.RandomState(seed)
    x = r.uniform(-1, 1, (n, 3072)).astype(np.float32)
    return x, r.randint(0, classes, n).astype(np.int32)


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


def mojo(reference, n_images, out):
    import cifar_ref as R
    import make_cifar_golden as M
    tmp = tempfile.mkdtemp(prefix="cifar_latency_")
    doc = {"host": platform.processor() or platform.machine(), "flags": "-std=c++11 -O0 -DDISTILLATION_MODE=1",
           "what": "the reference's network class, predict_class per image on one core; process start and file "
                   "reading included", "heads": {}}
    try:
        exe = M.build_driver(reference, tmp)
        for classes in (10, 100):
            w, b = R.model(classes, 10 + classes)
            x, lab = images(n_images, classes)
            t0 = time.perf_counter()
            M.run(exe, tmp, classes, w, b, x, lab, keep_probs=0)
            per = (time.perf_counter() - t0) / n_images
            doc["heads"][str(classes)] = {"images_run": n_images, "ms_per_image": per * 1e3,
                                          "scaled_to_10000_ms": per * N * 1e3, "scaled": True}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    write(doc, out)


def write(doc, out):
    text = json.dumps(doc, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="default: under profiles/cifar_eval/; '' writes no file")
    ap.add_argument("--mojo", default=None, metavar="DIR", help="time the reference's own forward instead (no GPU)")
    ap.add_argument("--mojo-images", type=int, default=300)
    a = ap.parse_args()
    here = os.path.join(ROOT, "profiles", "cifar_eval")
    if a.mojo:
        return mojo(a.mojo, a.mojo_images, os.path.join(here, "mojo_one_core.json") if a.out is None else a.out)
    import torch
    import fleet_amd as F
    from fleet_amd import cifar
    import cifar_ref as R
    import model_nets as NETS
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device path only")
    codec = F.Codec(0)
    heads = {}
    for classes in (10, 100):
        x, lab = images(N, classes)
        dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
        w, b = R.model(classes, 10 + classes)
        text = NETS.mode0_text(LAYERS(classes), R.B_SIZES[classes], R.W_SIZES[classes], w, b)
        rm = F.ResidentModel(codec, text, 0, max_versions=2)
        hm = F.Model(codec, text, 0)
        for m in (rm, hm):
            m.initUpdater([0.1])
        outs = {B: cifar.resident_evaluate_device(rm, dx[:B], dl[:B]) for B in (N, 100)}  # written again by every launch
        sets = {}
        for tag in ("a", "b"):
            s = {}
            for B in (N, 100):
                s[f"resident_evaluate_device/B{B}"] = median_ms(
                    lambda B=B: cifar.resident_evaluate_device(rm, dx[:B], dl[:B], out=outs[B]), a.reps)
            ts = []
            for i in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cifar.model_evaluate(hm, x, lab)
                if i:
                    ts.append((time.perf_counter() - t0) * 1e3)
            s[f"model_evaluate/B{N}"] = {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)),
                                         "max_ms": float(np.max(ts)), "reps": len(ts), "clock": "host, uploads included"}
            sets[tag] = s
        codec.check()
        med = lambda t, k: sets[t][k]["median_ms"]  # noqa: E731
        key = f"resident_evaluate_device/B{N}"
        heads[str(classes)] = {"sets": sets, "summary": {
            "images_per_s_B10000": {k: N / med(k, key) * 1e3 for k in sets},
            "repeat_spread_ms_B10000": abs(med("a", key) - med("b", key)),
            "host_model_over_resident_B10000": {k: med(k, f"model_evaluate/B{N}") / med(k, key) for k in sets}}}
        rm.close()
        hm.close()
    write({"device": torch.cuda.get_device_name(0), "images": N, "block_images": cifar.block_images(),
           "what": "device events around one call, median; sets a and b alternate in one process", "heads": heads},
          os.path.join(here, "cifar_eval_latency.json") if a.out is None else a.out)


if __name__ == "__main__":
    main()
