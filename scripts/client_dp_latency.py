#!/usr/bin/env python3
"""The client's gradients with DPgradients and with the distillation cost beside the plain call
(fleet_amd.client.resident_client_gradients_device), on the workload of client_grad_latency.py:
C = 64 clients of B = 100 samples over 10,000 seeded images resident in HBM, every client on the
seeded MNIST model's newest version, shifts drawn.

Measured, each the median of `reps` calls between device events after a warm-up:
  plain         cost cross_entropy, no clip / sigma: k_client_sample, k_client_sum
  dp            sigma > 0 for every client: k_client_sample, k_client_clip, k_client_sum_dp
  distillation  cost distillation, no DP: k_client_sample_distill, k_client_sum
The set is taken twice in one process, the measurements alternating (set "a", set "b"), so that
the spread of a repeat stands beside every figure. --parent-lib names a library built from the
parent commit: a child process loads it (FLEET_CODEC_LIB) and measures the plain call the same
way, twice, before this process touches the GPU. What DP adds over the plain call (dp - plain)
is k_client_clip, its serial binary32 add included, plus the difference of the two sum kernels;
--trace-only runs the dp call alone a few times for `rocprofv3 --kernel-trace --stats`, which
tells the kernels apart. No figure is fixed in advance and no speed is promised. No fallback:
without a GPU the script fails.

  python scripts/client_dp_latency.py [--reps N] [--parent-lib LIB.so] [--out FILE.json]
      # writes profiles/client_dp/client_dp_latency.json unless told otherwise
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

N, C, B = 10000, 64, 100
CLIP, SIGMA = 35.0, 1.0 / 128  # the clip lies inside the range of per-sample norms this model gives


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


def measure(reps, plain_only, trace_only):
    import torch
    import fleet_amd as F
    from fleet_amd import client as K
    import eval_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device path only")
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

    def plain():
        K.resident_client_gradients_device(rm, None, dx, dl, idx=di, shifts=ds, grads=grads)

    def dp():
        K.resident_client_gradients_device(rm, None, dx, dl, idx=di, shifts=ds, grads=grads, clip=CLIP, sigma=SIGMA)

    def distillation():
        K.resident_client_gradients_device(rm, None, dx, dl, idx=di, shifts=ds, grads=grads, cost="distillation")

    if trace_only:
        for _ in range(5):
            dp()
        torch.cuda.synchronize()
        codec.check()
        return None
    configs = {"plain": plain} if plain_only else {"plain": plain, "dp": dp, "distillation": distillation}
    sets = {tag: {name: median_ms(fn, reps) for name, fn in configs.items()} for tag in ("a", "b")}
    codec.check()
    return {"device": torch.cuda.get_device_name(0), "sets": sets}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None, help="libfleetcodec.so built from the parent commit")
    ap.add_argument("--plain-only", action="store_true", help="the plain call alone, JSON on stdout (the child's mode)")
    ap.add_argument("--trace-only", action="store_true", help="five dp calls and nothing else, for a kernel trace")
    ap.add_argument("--out", default=None, help="default: profiles/client_dp/client_dp_latency.json; '' writes no file")
    a = ap.parse_args()
    if a.plain_only or a.trace_only:
        got = measure(a.reps, True, a.trace_only)
        if got is not None:
            print("RESULT " + json.dumps(got))
        return
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "client_dp", "client_dp_latency.json")
    parent = None
    if a.parent_lib:  # a fresh process, before this one opens the GPU
        env = dict(os.environ, FLEET_CODEC_LIB=os.path.abspath(a.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--reps", str(a.reps)], env=env,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("the parent library's run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        parent = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")][-1][7:])
    got = measure(a.reps, False, False)
    sets = got["sets"]
    med = lambda t, k: sets[t][k]["median_ms"]  # noqa: E731
    spread = {k: abs(med("a", k) - med("b", k)) for k in sets["a"]}
    doc = {"device": got["device"], "clients": C, "samples_per_client": B, "images": N, "clip": CLIP, "sigma": SIGMA,
           "what": "device events around one call, median; sets a and b alternate in one process",
           "sets": sets}
    summary = {"ms": {k: {t: med(t, k) for t in sets} for k in sets["a"]}, "repeat_spread_ms": spread,
               "dp_minus_plain_ms": {t: med(t, "dp") - med(t, "plain") for t in sets},
               "dp_minus_plain_us_per_clipped_sample": {t: (med(t, "dp") - med(t, "plain")) * 1e3 / (C * (B - 1))
                                                        for t in sets},
               "distillation_minus_plain_ms": {t: med(t, "distillation") - med(t, "plain") for t in sets}}
    if parent is not None:
        pm = {t: parent["sets"][t]["plain"]["median_ms"] for t in parent["sets"]}
        doc["parent_commit_plain"] = {"what": "the parent commit's library in a process of its own, the same call",
                                      "sets": parent["sets"]}
        lo, hi = min(pm.values()), max(pm.values())
        this = [med(t, "plain") for t in sets]
        summary["parent_plain_ms"] = pm
        summary["plain_minus_parent_ms"] = float(np.mean(this) - np.mean(list(pm.values())))
        summary["plain_within_the_spread_of_the_parent_sets"] = bool(
            min(this) <= hi + spread["plain"] and max(this) >= lo - spread["plain"])
    doc["summary"] = summary
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
