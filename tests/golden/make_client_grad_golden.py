"""Records tests/golden/client_grad_ref.npz from the reference's own network class.

    python tests/golden/make_client_grad_golden.py [OUT.npz] [--reference DIR]

tests/native/ref_client_grad_driver.cpp is compiled into a temporary directory outside the tree
with the flags make_eval_golden.py uses (-std=c++11 -O0 -DDISTILLATION_MODE=1
-I<reference>/commonLib/cppNN -w -fno-access-control), run on the seeded inputs of
tests/client_grad_ref.py (whose docstring lists the cases and the recorded fields), and its
outputs are stored. Before anything is written the reference's numbers alone must show that
the fixture can tell the gradient from its nearest wrong neighbours (conditions(), re-asserted
from the fixture by tests/test_client_grad_inputs.py). Only recorded values are committed."""
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

import client_grad_ref as R  # noqa: E402

DEFAULT_REFERENCE = "/root/reference"
f = np.float32


def build_driver(reference: str, tmp: str) -> str:
    exe = os.path.join(tmp, "ref_client_grad_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O0", "-DDISTILLATION_MODE=1", "-fno-access-control",
                           f"-I{os.path.join(reference, 'commonLib', 'cppNN')}", "-w",
                           os.path.join(ROOT, "tests", "native", "ref_client_grad_driver.cpp"), "-o", exe])
    return exe


def run(exe, tmp, cases):
    """[{input, E, node_<L>, pmap_P1, pmap_P2, delta_<L> (per sample, stacked), grad}] per case"""
    w, b = R.model()
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(w.tobytes() + b.tobytes() + np.int32(len(cases)).tobytes())
        for name, B, teacher, mode, seed, x, lab, sh in cases:
            fh.write(np.array([B, teacher, mode, seed], np.int32).tobytes())
            for a, t in ((x, f), (lab, np.int32), (sh, np.int32)):
                fh.write(np.ascontiguousarray(a, dtype=t).tobytes())
    subprocess.check_call([exe, fin, fout], stdout=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    o = 0

    def take(n, t):
        nonlocal o
        a = np.frombuffer(raw, t, n, o).copy()
        o += 4 * n
        return a
    outs = []
    for name, B, *_ in cases:
        per = []
        for k in range(B):
            d = {"input": take(784, f), "E": take(1, f)[0]}
            for L, n in zip(R.LAYERS, R.SIZES):
                d[f"node_{L}"] = take(n, f)
            d["pmap_P1"], d["pmap_P2"] = take(512, np.int32), take(192, np.int32)
            for L, n in zip(R.LAYERS, R.SIZES):
                d[f"delta_{L}"] = take(n, f)
            per.append(d)
        out = {k: np.stack([d[k] for d in per]) for k in per[0]}
        out["grad"] = take(R.N_UP, f)
        outs.append(out)
    assert o == len(raw), (o, len(raw))
    return outs


def second_picks(node_top, pmap, pool, size):
    """per window: True where the picked element is not the window's largest"""
    top = np.asarray(node_top, f).reshape(-1, size, size)
    out = []
    n = size // pool
    for o, idx in enumerate(pmap):
        k, j, i = o // (n * n), (o // n) % n, o % n
        win = top[k, pool * j:pool * j + pool, pool * i:pool * i + pool]
        out.append(top.reshape(-1)[idx] < win.max())
    return np.array(out)


def ordered_sum(vectors):
    """sync_mini_batch's per-element binary32 sum over these gradients() vectors in the order
    given (the header values are sizes and are not summed)"""
    from fleet_amd.layouts import MNIST
    acc = vectors[0].copy()
    for v in vectors[1:]:
        acc = (acc + v).astype(f)
    acc[MNIST.header_positions()] = MNIST.header_values()
    return acc


def conditions(z):
    """What the reference's numbers must show (the issue's six conditions)."""
    # 1. in one sample both pools take the second candidate somewhere and the first elsewhere
    ok = False
    for name in R.FULL:
        s1 = second_picks(z[f"{name}_node_C1"][0], z[f"{name}_pmap_P1"][0], 3, 24)
        s2 = second_picks(z[f"{name}_node_C2"][0], z[f"{name}_pmap_P2"][0], 2, 4)
        ok |= bool(s1.any() and (~s1).any() and s2.any() and (~s2).any())
    assert ok, "no sample has both picks in both pools"
    # 2. both elu df branches occur in C1, C2i and C2, where a delta arrives
    for L in ("C1", "C2i", "C2"):
        node, delta = z[f"z_node_{L}"][0], z[f"z_delta_{L}"][0]
        live = delta != 0
        assert (node[live] > 0).any() and (node[live] <= 0).any(), L
    # 3. the B = 5 vector differs in bits from the same samples summed in reverse order
    assert (R.bits(z["b5_grad"]) != R.bits(z["b5_reverse"])).any(), "the sum's order does not show"
    # 4. temperature 1 and 2 differ
    assert (R.bits(z["t1_grad"]) != R.bits(z["z_grad"])).any()
    # 5. each shifted case's input differs from the unshifted one
    for dx, dy in R.SHIFTS8:
        assert (R.bits(z[f"{R.shift_name(dx, dy)}_input"]) != R.bits(z["z_input"])).any(), (dx, dy)
    # 6. every E is finite
    for name, *_ in R.cases():
        assert np.isfinite(z[f"{name}_E"]).all(), name


def record(out_path: str, reference: str = DEFAULT_REFERENCE) -> None:
    tmp = tempfile.mkdtemp(prefix="client_grad_golden_")
    try:
        exe = build_driver(reference, tmp)
        cases = R.cases()
        outs = run(exe, tmp, cases)
        z = {"digest": np.frombuffer(R.input_digest().encode(), np.uint8)}
        for (name, B, *_), out in zip(cases, outs):
            z[f"{name}_input"], z[f"{name}_E"] = out["input"], out["E"]
            if name in R.FULL:
                for k, v in out.items():
                    z[f"{name}_{k}"] = v
            elif name.startswith("s_"):
                z[f"{name}_node_FC2"] = out["node_FC2"]
                z[f"{name}_grad_c1"], z[f"{name}_grad_i1"] = out["grad"][R.G_C1], out["grad"][R.G_I1]
                z[f"{name}_grad_sha256"] = np.frombuffer(R.sha(out["grad"]).encode(), np.uint8)
            else:
                z[f"{name}_grad"] = out["grad"]
        # b5's samples one by one under the shifts the reference drew, for condition 3 (the
        # vectors themselves are not stored, only their reverse-order sum)
        name, B, teacher, mode, seed, x, lab, sh = cases[-1]
        assert name == "b5"
        shifts = R.recorded_shifts(z, "b5", x)
        singles = run(exe, tmp, [(f"b5_{k}", 1, teacher, 0, 0, x[k:k + 1], lab[k:k + 1], shifts[k:k + 1])
                                 for k in range(B)])
        vs = [s["grad"] for s in singles]
        assert (R.bits(ordered_sum(vs)) == R.bits(z["b5_grad"])).all(), "b5 is not its samples' ordered sum"
        z["b5_reverse"] = ordered_sum(vs[::-1])
        z = {k: np.ascontiguousarray(v) for k, v in z.items()}
        conditions(z)
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
    out = args[0] if args else os.path.join(HERE, "client_grad_ref.npz")
    record(out, ref)
    print(out, os.path.getsize(out), "bytes")
