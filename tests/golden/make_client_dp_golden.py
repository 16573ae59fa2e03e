"""Records tests/golden/client_dp_ref.npz from the reference's own network class.

    python tests/golden/make_client_dp_golden.py [OUT.npz] [--reference DIR] [--probe]

tests/native/ref_client_dp_driver.cpp is compiled into a temporary directory outside the tree
with the flags make_client_grad_golden.py uses (-std=c++11 -O0 -DDISTILLATION_MODE=1
-I<reference>/commonLib/cppNN -w -fno-access-control), run on the seeded inputs of
tests/client_dp_ref.py (whose docstring lists the cases and the recorded fields), and its
outputs are stored. Before anything is written the reference's numbers alone must show that the
fixture can tell DPgradients and the distillation cost from their nearest wrong neighbours
(conditions()). --probe prints the recorded norms of every case and writes nothing: CLIP_C of
client_dp_ref.py is chosen from them. Only recorded values are committed."""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import client_dp_ref as R  # noqa: E402

DEFAULT_REFERENCE = "/root/reference"
f = np.float32


def build_driver(reference: str, tmp: str) -> str:
    exe = os.path.join(tmp, "ref_client_dp_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O0", "-DDISTILLATION_MODE=1", "-fno-access-control",
                           f"-I{os.path.join(reference, 'commonLib', 'cppNN')}", "-w",
                           os.path.join(ROOT, "tests", "native", "ref_client_dp_driver.cpp"), "-o", exe])
    return exe


def run(exe, tmp, cases):
    """(draws [22961] float64, [{E, node_FC2, delta_FC2, sqsum, sqsum_layout, norm, scale, grad}] per case)"""
    w, b = R.model()
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(w.tobytes() + b.tobytes() + np.int32(len(cases)).tobytes())
        for name, B, cost, clip, sigma, x, lab, sh in cases:
            fh.write(np.array([B, cost], np.int32).tobytes() + np.array([clip, sigma], f).tobytes())
            for a, t in ((x, f), (lab, np.int32), (sh, np.int32)):
                fh.write(np.ascontiguousarray(a, dtype=t).tobytes())
    subprocess.check_call([exe, fin, fout], stdout=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    n = int(np.frombuffer(raw, np.int32, 1, 0)[0])
    assert n == R.N_UP
    draws = np.frombuffer(raw, np.float64, n, 4).copy()
    o = 4 + 8 * n

    def take(count):
        nonlocal o
        a = np.frombuffer(raw, f, count, o).copy()
        o += 4 * count
        return a
    outs = []
    for name, B, *_ in cases:
        per = np.stack([take(21) for _ in range(B)])
        stats = np.stack([take(4) for _ in range(B)])
        outs.append({"E": per[:, 0].copy(), "node_FC2": per[:, 1:11].copy(), "delta_FC2": per[:, 11:21].copy(),
                     "sqsum": stats[:, 0].copy(), "sqsum_layout": stats[:, 1].copy(), "norm": stats[:, 2].copy(),
                     "scale": stats[:, 3].copy(), "grad": take(R.N_UP)})
    assert o == len(raw), (o, len(raw))
    return draws, outs


def blocks_differ(u, v):
    return [bool((R.bits(u[s:s + n]) != R.bits(v[s:s + n])).any()) for s, n in R.BLOCKS]


def conditions(out, helpers):
    """What the reference's numbers must show before the fixture is written."""
    c, d = out["c"], out["d"]
    # c: an ordered sqsum differs in bits from the same squares added in layout order
    assert (R.bits(c["sqsum"][1:]) != R.bits(c["sqsum_layout"][1:])).any(), "the walk's order does not show"
    # c: samples 1-3 on both sides of the clip, sample 0 above it; d: the clip above every norm
    assert (c["norm"][1:] > R.CLIP_C).any() and (c["norm"][1:] < R.CLIP_C).any() and c["norm"][0] > R.CLIP_C, c["norm"]
    assert (c["scale"][1:] < 1).any() and (c["scale"][1:] == 1).any()
    assert (d["norm"] < R.CLIP_D).all() and (d["scale"] == 1).all()
    assert f(R.CLIP_C) * f(R.SIGMA_C) == f(R.CLIP_D) * f(R.SIGMA_D)
    # c's vector differs from d's in a bias block; whether in a dW block is recorded as a fact
    diff = blocks_differ(c["grad"], d["grad"])
    n_dw = sum(1 for s, n in R.BLOCKS if s < R.BIAS_START)
    assert any(diff[n_dw:]), "clipping does not show in any bias block"
    dw_differ = any(diff[:n_dw])
    # every value block of a differs from the noise-free vector
    assert all(blocks_differ(out["a"]["grad"], helpers["a_plain"]["grad"]))
    # the distillation delta differs from the cross-entropy delta
    assert (R.bits(out["e1"]["delta_FC2"]) != R.bits(helpers["e1_ce"]["delta_FC2"])).any()
    assert (R.bits(out["e1"]["node_FC2"]) == R.bits(helpers["e1_ce"]["node_FC2"])).all()
    # every out * (1 - out) of the distillation cases is non-zero, every E finite
    for name in ("e1", "e3", "f"):
        node = out[name]["node_FC2"].astype(f)
        assert ((node * (f(1) - node)).astype(f) != 0).all(), name
    for name, o in out.items():
        assert np.isfinite(o["E"]).all(), name
        assert np.isfinite(o["grad"]).all(), name
    return dw_differ


def record(out_path: str, reference: str = DEFAULT_REFERENCE, probe: bool = False) -> None:
    tmp = tempfile.mkdtemp(prefix="client_dp_golden_")
    try:
        exe = build_driver(reference, tmp)
        cases, extra = R.cases(), R.helper_cases()
        draws, outs = run(exe, tmp, cases + extra)
        out = {name: o for (name, *_), o in zip(cases, outs)}
        helpers = {name: o for (name, *_), o in zip(extra, outs[len(cases):])}
        if probe:
            for name, o in out.items():
                print(name, "norm", o["norm"], "scale", o["scale"])
            return
        z = {"digest": np.frombuffer(R.input_digest().encode(), np.uint8),
             "z_sha256": np.frombuffer(hashlib.sha256(draws.tobytes()).hexdigest().encode(), np.uint8),
             "z_head": draws[:32].copy(), "z_tail": draws[-32:].copy()}
        for name, o in out.items():
            for k in ("E", "node_FC2", "delta_FC2", "sqsum", "sqsum_layout", "norm", "scale"):
                z[f"{name}_{k}"] = o[k]
            z[f"{name}_grad_sha256"] = np.frombuffer(R.sha(o["grad"]).encode(), np.uint8)
            z[f"{name}_grad_i1"], z[f"{name}_grad_fc2"] = o["grad"][R.G_I1], o["grad"][R.G_FC2]
            if name in R.FULL:
                z[f"{name}_grad"] = o["grad"]
        z["c_d_dw_differ"] = np.array(conditions(out, helpers))
        z = {k: np.ascontiguousarray(v) for k, v in z.items()}
        np.savez_compressed(out_path, **z)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    ref = DEFAULT_REFERENCE
    if "--reference" in args:
        i = args.index("--reference")
        ref = args[i + 1]
        del args[i:i + 2]
    probe = "--probe" in args
    args = [a for a in args if a != "--probe"]
    out = args[0] if args else os.path.join(HERE, "client_dp_ref.npz")
    record(out, ref, probe)
    if not probe:
        print(out, os.path.getsize(out), "bytes")
