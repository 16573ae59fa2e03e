#!/usr/bin/env python3
"""The resident model's step (fleet_amd.ResidentModel.descent_device) under each solver: from a
merged gradient in HBM to the new version staged in its row, the call's closing synchronise
included (a host clock around it).

Per model (the MNIST network; a CIFAR-10-size network of 306,480 weights; the texts of
scripts/resident_model_latency.py), per DISTILLATION_MODE (0 and 1) and per solver (sgd,
adagrad, rmsprop, adam): the median of `reps` steps, the solvers alternating within each
repetition, the first repetition not recorded. Every figure is taken twice, in two identical
runs (run "a" and run "b", each a process of its own), so that the spread of a repeat stands
beside every difference. With --parent-lib (a libfleetcodec.so built from the parent commit,
loaded through FLEET_CODEC_LIB) the sgd step of that build is measured in the same session,
in runs of sgd alone, alternating with like runs of this build (a run that alternates four
models is no like-for-like partner of one that steps a single model): parent a, this-sgd a,
this a, parent b, this-sgd b, this b.

No figure is fixed in advance. The file records: the sgd step of this build against the
parent's, with the spread of the identical runs; what each solver costs over sgd.
No fallback: without a GPU the script fails.

  python scripts/solver_step_latency.py [--parent-lib PATH] [--models mnist,cifar10] [--out FILE.json]
      # writes profiles/solvers/solver_step_latency.json unless told otherwise
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SOLVERS = ("sgd", "adagrad", "rmsprop", "adam")


def worker(models, reps_arg, solvers):
    """One run: prints {"<model>/mode<m>/<solver>": spread} as one JSON line."""
    import torch
    import fleet_amd as F
    import pyoracle
    from acc_latency import spread
    from fleet_amd.layouts import CIFAR10, MNIST
    from resident_model_latency import cifar10_texts, mnist_texts
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device path only")
    codec = F.Codec(0)
    oracle = pyoracle.Oracle()
    out = {"device": torch.cuda.get_device_name(0)}
    clock = time.perf_counter
    for name in models:
        texts = mnist_texts(codec) if name == "mnist" else cifar10_texts(codec)
        layout = MNIST if name == "mnist" else CIFAR10
        reps = reps_arg or (200 if name == "mnist" else 60)
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
        for mode in (0, 1):
            ms = {}
            for s in solvers:
                ms[s] = F.ResidentModel(codec, texts[mode], mode, max_versions=2)
                if s != "sgd":
                    ms[s].set_solver(s)
                ms[s].initUpdater([1e-4])
            t = {s: [] for s in solvers}
            for r in range(reps + 1):
                for s in solvers:
                    torch.cuda.synchronize()
                    t0 = clock()
                    ms[s].descent_device(d_f32[r % 2], 2, n_values=n)
                    t1 = clock()
                    if r:
                        t[s].append(t1 - t0)
            for s in solvers:
                out[f"{name}/mode{mode}/{s}"] = spread(t[s])
                ms[s].close()
    print("RESULT " + json.dumps(out))


def run(lib, models, reps, solvers):
    env = dict(os.environ)
    if lib:
        env["FLEET_CODEC_LIB"] = lib
    else:
        env.pop("FLEET_CODEC_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--models", ",".join(models), "--reps",
                        str(reps), "--solvers", ",".join(solvers)], env=env, capture_output=True, text=True, timeout=900)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit("worker failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="mnist,cifar10")
    ap.add_argument("--reps", type=int, default=0, help="0: 200 for mnist, 60 for cifar10")
    ap.add_argument("--solvers", default=",".join(SOLVERS))
    ap.add_argument("--parent-lib", default=None, help="libfleetcodec.so of the parent commit (sgd only)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="default: profiles/solvers/solver_step_latency.json; '' writes no file")
    a = ap.parse_args()
    models, solvers = a.models.split(","), a.solvers.split(",")
    if a.worker:
        return worker(models, a.reps, solvers)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "solvers", "solver_step_latency.json")
    runs = {}
    for tag in ("a", "b"):
        if a.parent_lib:
            runs[f"parent_{tag}"] = run(os.path.abspath(a.parent_lib), models, a.reps, ["sgd"])
            runs[f"this_sgd_{tag}"] = run(None, models, a.reps, ["sgd"])
        runs[f"this_{tag}"] = run(None, models, a.reps, solvers)
    device = runs["this_a"].pop("device")
    for v in runs.values():
        v.pop("device", None)
    rows = []
    for key in sorted(k for k in runs["this_a"] if k.endswith("/sgd")):
        base = key[: -len("/sgd")]
        med = lambda r, k: runs[r][k]["median_ms"]  # noqa: E731
        row = {"config": base,
               "sgd_median_ms": {"this_a": med("this_a", key), "this_b": med("this_b", key)},
               "repeat_spread_ms": abs(med("this_a", key) - med("this_b", key))}
        if a.parent_lib:
            row["sgd_alone_median_ms"] = {r: med(r, key) for r in ("parent_a", "parent_b", "this_sgd_a", "this_sgd_b")}
            row["sgd_alone_repeat_spread_ms"] = max(abs(med("parent_a", key) - med("parent_b", key)),
                                                    abs(med("this_sgd_a", key) - med("this_sgd_b", key)))
            row["sgd_alone_this_minus_parent_ms"] = ((med("this_sgd_a", key) + med("this_sgd_b", key))
                                                     - (med("parent_a", key) + med("parent_b", key))) / 2
        row["solver_over_sgd_ms"] = {
            s: {t: med(f"this_{t}", f"{base}/{s}") - med(f"this_{t}", key) for t in ("a", "b")}
            for s in solvers if s != "sgd"}
        rows.append(row)
    doc = {"device": device, "what": "ResidentModel.descent_device, host clock around the synchronous call",
           "summary": rows, "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
