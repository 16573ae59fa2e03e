"""Records tests/golden/solver_ref.npz from the reference's own solver and network classes.

    python tests/golden/make_solver_golden.py [OUT.npz] [--reference DIR]

tests/native/ref_solver_driver.cpp is compiled into a temporary directory outside the tree
with the reference's flags (oracle/Makefile: -std=c++11 -O0 -DDISTILLATION_MODE=1
-I<reference>/commonLib/cppNN -w) plus -fno-access-control (the solvers keep their state
private), run on the seeded inputs of tests/solver_ref.py, and its outputs are stored:

  (a) class level, new_solver(name)->increment_w on one matrix, three steps:
        a_{solver}_{w,g1}[3][N], a_adam_g2[3][N]        inputs: solver_ref.class_inputs()
      and a session continued from state in the denormal range:
        c_{solver}_{w,g1}[3][N], c_adam_g2[3][N]        inputs: solver_ref.continued_inputs()
  (b) network level, mojo::network(name) reading model_mnist_seeded.npz's text, one
      train_class, then three set_learning_rate / descent(vector) with distinct gradients
      (solver_ref.network_gradients(MNIST, oracle): decodeFloat of seeded merged texts;
      rates solver_ref.NET_LRS):
        b_w0, b_b0                          the weights and biases as read
        b_{solver}_w_last                   every weight after the last step
        b_{solver}_w_sub[3][...]            every NET_STRIDE-th weight after each step
        b_{solver}_b[3][n_b]                the use_bias() layers' biases after each step
Only these recorded values are committed, never the driver's binary."""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import solver_ref as R  # noqa: E402
from fleet_amd.layouts import MNIST  # noqa: E402

DEFAULT_REFERENCE = "/root/reference"


def build_driver(reference: str, tmp: str) -> str:
    exe = os.path.join(tmp, "ref_solver_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O0", "-DDISTILLATION_MODE=1", "-fno-access-control",
                           f"-I{os.path.join(reference, 'commonLib', 'cppNN')}", "-w",
                           os.path.join(ROOT, "tests", "native", "ref_solver_driver.cpp"), "-o", exe])
    return exe


def run_class(exe, tmp, solver, L, w0, g1_0, g2_0, d):
    steps, n = d.shape
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<iiif", R.SOLVERS.index(solver), n, steps, float(L)))
        for a in (w0, g1_0, g2_0, d):
            fh.write(np.ascontiguousarray(a, np.float32).tobytes())
    subprocess.check_call([exe, "class", fin, fout])
    out = np.fromfile(fout, np.float32).reshape(steps, 3, n)
    return out[:, 0], out[:, 1], out[:, 2]


def run_net(exe, tmp, solver, text, lrs, grads):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<iiii", R.SOLVERS.index(solver), len(text), len(grads[0]), len(grads)))
        fh.write(text)
        for lr, g in zip(lrs, grads):
            fh.write(struct.pack("<f", float(np.float32(lr))))
            fh.write(np.ascontiguousarray(g, np.float32).tobytes())
    subprocess.check_call([exe, "net", fin, fout])
    raw = open(fout, "rb").read()
    n_w, n_b = struct.unpack("<ii", raw[:8])
    v = np.frombuffer(raw[8:], np.float32).reshape(len(grads) + 1, n_w + n_b)
    return v[:, :n_w], v[:, n_w:]


def record(out_path: str, reference: str = DEFAULT_REFERENCE) -> None:
    tmp = tempfile.mkdtemp(prefix="solver_golden_")
    try:
        exe = build_driver(reference, tmp)
        z = {}
        w0, d = R.class_inputs()
        zero = np.zeros_like(w0)
        cw0, cg1, cg2, cd = R.continued_inputs()
        for s in R.SOLVERS[1:]:
            w, g1, g2 = run_class(exe, tmp, s, R.CLASS_L, w0, zero, zero, d)
            z[f"a_{s}_w"], z[f"a_{s}_g1"] = w, g1
            if s == "adam":
                z["a_adam_g2"] = g2
            s1, s2 = R.continued_state(s, cg1, cg2)
            w, g1, g2 = run_class(exe, tmp, s, R.CONT_L, cw0, s1, s2, cd)
            z[f"c_{s}_w"], z[f"c_{s}_g1"] = w, g1
            if s == "adam":
                z["c_adam_g2"] = g2
        text = bytes(np.load(os.path.join(HERE, "model_mnist_seeded.npz"))["text"])
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import pyoracle
        pyoracle.build()
        grads = [g for _, g in R.network_gradients(MNIST, pyoracle.Oracle())]
        for s in R.SOLVERS[1:]:
            w, b = run_net(exe, tmp, s, text, R.NET_LRS, grads)
            if "b_w0" in z:
                assert np.array_equal(R.bits(z["b_w0"]), R.bits(w[0]))
            z["b_w0"], z["b_b0"] = w[0], b[0]
            z[f"b_{s}_w_last"] = w[-1]
            z[f"b_{s}_w_sub"] = w[1:, ::R.NET_STRIDE]
            z[f"b_{s}_b"] = b[1:]
        np.savez_compressed(out_path, **{k: np.ascontiguousarray(v) for k, v in z.items()})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    ref = DEFAULT_REFERENCE
    if "--reference" in args:
        i = args.index("--reference")
        ref = args[i + 1]
        del args[i:i + 2]
    out = args[0] if args else os.path.join(HERE, "solver_ref.npz")
    record(out, ref)
    print(out, os.path.getsize(out), "bytes")
