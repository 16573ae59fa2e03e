#!/usr/bin/env python3
"""DPgradients on the CIFAR network beside the plain call
(fleet_amd.cifar_client.resident_client_gradients_device), on the workload of
cifar_client_latency.py: C = 64 clients of B = 100 samples over 2,000 seeded images resident in
HBM, every client on a resident CIFAR-10 model, shifts drawn.

Measured, each the median of `reps` calls between device events after a warm-up:
  plain  no clip / sigma: k_rgb_sample, k_rgb_sum, k_rgb_fc_sum
  dp     sigma > 0 for every client: k_rgb_sample, k_rgb_clip, k_rgb_sum_dp, k_rgb_fc_sum_dp
The set is taken twice in one process, the measurements alternating (set "a", set "b"), so that
the spread of a repeat stands beside every figure. --parent-lib names a library built from the
parent commit: a child process loads it (FLEET_CODEC_LIB) and measures the plain call the same
way, twice, before this process touches the GPU. What DP adds over the plain call (dp - plain)
is k_rgb_clip plus the difference of the sum kernels (the noise); divided by the C * (B - 1)
clipped samples it bounds k_rgb_clip's time per clipped sample from above. No figure is fixed
in advance and no speed is promised. No fallback: without a GPU the script fails.

  python scripts/cifar_dp_latency.py [--reps N] [--parent-lib LIB.so] [--out FILE.json]
      # writes profiles/cifar_dp/cifar_dp_latency.json unless told otherwise
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

N, C, B, CLASSES = 2000, 64, 100, 10
CLIP, SIGMA = 1.0, 1.0 / 128  # (the walk's length does not depend on them)


def measure(reps, plain_only):
    import torch
    import fleet_amd as F
    from fleet_amd import cifar_client as K
    from fleet_amd.client import client_shifts
    import cifar_grad_ref as G
    import cifar_ref as R
    import model_nets as M
    from client_dp_latency import median_ms
    from test_gpu_cifar import LAYERS
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device path only")
    codec = F.Codec(0)
    r = np.random.RandomState(1234)
    x = r.uniform(-1, 1, (N, 3072)).astype(np.float32)
    lab = r.randint(0, CLASSES, N).astype(np.int32)
    idx = r.randint(0, N, (C, B)).astype(np.int32)
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    di, ds = torch.from_numpy(idx).cuda(), torch.from_numpy(client_shifts(1, C, B)).cuda()
    w, b = G.model(5, CLASSES)
    rm = F.ResidentModel(codec, M.mode0_text(LAYERS(CLASSES), R.B_SIZES[CLASSES], R.W_SIZES[CLASSES], w, b), 0,
                         max_versions=2)
    rm.initUpdater([0.05, 0.02])
    grads = torch.empty(C, K.grad_len(CLASSES), dtype=torch.float32, device="cuda")

    def plain():
        K.resident_client_gradients_device(rm, CLASSES, None, dx, dl, idx=di, shifts=ds, grads=grads)

    def dp():
        K.resident_client_gradients_device(rm, CLASSES, None, dx, dl, idx=di, shifts=ds, grads=grads, clip=CLIP,
                                           sigma=SIGMA)

    configs = {"plain": plain} if plain_only else {"plain": plain, "dp": dp}
    sets = {tag: {name: median_ms(fn, reps) for name, fn in configs.items()} for tag in ("a", "b")}
    codec.check()
    return {"device": torch.cuda.get_device_name(0), "sets": sets}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libfleetcodec.so built from the parent commit")
    ap.add_argument("--plain-only", action="store_true", help="the plain call alone, JSON on stdout (the child's mode)")
    ap.add_argument("--out", default=None, help="default: profiles/cifar_dp/cifar_dp_latency.json; '' writes no file")
    a = ap.parse_args()
    if a.plain_only:
        print("RESULT " + json.dumps(measure(a.reps, True)))
        return
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "cifar_dp", "cifar_dp_latency.json")
    parent = None
    if a.parent_lib:  # a fresh process, before this one opens the GPU
        env = dict(os.environ, FLEET_CODEC_LIB=os.path.abspath(a.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--reps", str(a.reps)], env=env,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("the parent library's run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        parent = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")][-1][7:])
    got = measure(a.reps, False)
    sets = got["sets"]
    med = lambda t, k: sets[t][k]["median_ms"]  # noqa: E731
    spread = {k: abs(med("a", k) - med("b", k)) for k in sets["a"]}
    doc = {"device": got["device"], "classes": CLASSES, "clients": C, "samples_per_client": B, "images": N, "clip": CLIP,
           "sigma": SIGMA, "what": "device events around one call, median; sets a and b alternate in one process",
           "sets": sets}
    summary = {"ms": {k: {t: med(t, k) for t in sets} for k in sets["a"]}, "repeat_spread_ms": spread,
               "dp_minus_plain_ms": {t: med(t, "dp") - med(t, "plain") for t in sets},
               "dp_minus_plain_us_per_clipped_sample": {t: (med(t, "dp") - med(t, "plain")) * 1e3 / (C * (B - 1))
                                                        for t in sets}}
    if parent is not None:
        pm = {t: parent["sets"][t]["plain"]["median_ms"] for t in parent["sets"]}
        doc["parent_commit_plain"] = {"what": "the parent commit's library in a process of its own, the same call",
                                      "sets": parent["sets"]}
        summary["parent_plain_ms"] = pm
        summary["plain_minus_parent_ms"] = float(np.mean([med(t, "plain") for t in sets]) - np.mean(list(pm.values())))
    doc["summary"] = summary
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
