"""Records tests/golden/cifar_ref.npz from the reference's own network class.

    python tests/golden/make_cifar_golden.py [OUT.npz] [--reference DIR]

tests/native/ref_cifar_driver.cpp is compiled into a temporary directory outside the tree
with the reference's flags (oracle/Makefile: -std=c++11 -O0 -DDISTILLATION_MODE=1
-I<reference>/commonLib/cppNN -w) plus -fno-access-control, run on the seeded inputs of
tests/cifar_ref.py (whose docstring lists the cases), and its outputs are stored. Before
anything is written the reference's numbers alone must show that the fixture can tell the
forward from its nearest wrong neighbours (conditions(), re-asserted from the fixture by
tests/test_cifar_inputs.py). Only recorded values are committed, never the driver's binary."""
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

import cifar_ref as R  # noqa: E402

DEFAULT_REFERENCE = "/root/reference"


def build_driver(reference: str, tmp: str) -> str:
    exe = os.path.join(tmp, "ref_cifar_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O0", "-DDISTILLATION_MODE=1", "-fno-access-control",
                           f"-I{os.path.join(reference, 'commonLib', 'cppNN')}", "-w",
                           os.path.join(ROOT, "tests", "native", "ref_cifar_driver.cpp"), "-o", exe])
    return exe


def run(exe, tmp, classes, w, b, x, labels, perm=None, keep_probs=None, n_layers=0):
    B = len(labels)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<iiii", classes, B, 0 if perm is None else B, n_layers))
        for a, t in ((w, np.float32), (b, np.float32), (x, np.float32), (labels, np.int32)):
            fh.write(np.ascontiguousarray(a, t).tobytes())
        if perm is not None:
            fh.write(np.ascontiguousarray(perm, np.int32).tobytes())
    subprocess.check_call([exe, fin, fout], stdout=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    o = 0

    def take(n, t):
        nonlocal o
        a = np.frombuffer(raw, t, n, o).copy()
        o += 4 * n
        return a
    nw, nb, stride = (int(v) for v in take(3, np.int32))
    assert nw == R.n_w(classes) and nb == R.n_b(classes), (nw, nb)
    out = {"c1_chan_stride": stride, "pred": take(B, np.int32), "p": take(B, np.float32), "cost": take(B, np.float32),
           "probs": take(classes * B, np.float32).reshape(B, classes)[:B if keep_probs is None else keep_probs],
           "error": take(B, np.float32), "accuracy": take(B, np.float32), "correct": take(B, np.int32)}
    layers = {name: [] for name, _ in R.LAYERS}
    for _ in range(n_layers):
        for name, shape in R.LAYERS:
            layers[name].append(take(int(np.prod(shape)), np.float32).reshape(shape))
    out["layers"] = {k: np.stack(v) for k, v in layers.items() if v}
    if perm is not None:
        e, a, c = struct.unpack("<ffi", raw[o:o + 12])
        o += 12
        out["perm"] = (np.float32(e), np.float32(a), np.int32(c))
    assert o == len(raw)
    return out


def windows(top, size, stride):
    """[..., rows, cols, size*size]: every pool window of the maps top [..., h, w], row-major"""
    h = (top.shape[-2] - size) // stride + 1
    w = (top.shape[-1] - size) // stride + 1
    return np.stack([top[..., dy:dy + stride * h:stride, dx:dx + stride * w:stride]
                     for dy in range(size) for dx in range(size)], axis=-1)


def conditions(z):
    """What the reference's numbers must show, from the recorded arrays alone."""
    bits = R.bits
    for name, least in (("a10", 5), ("a100", 8)):
        a = R.case(z, name)
        B = len(a["pred"])
        assert len(np.unique(a["pred"])) >= least, (name, np.unique(a["pred"]))
        assert 0 < int(a["correct"][-1]) < B, (name, int(a["correct"][-1]))
    # the ordered binary32 sum differs from the pairwise sum, the float64 sum and the permuted order
    a = R.case(z, "a10")
    B = len(a["pred"])
    e = bits(a["error"][-1])
    pairwise = np.float32(np.sum(a["cost"], dtype=np.float32) / np.float32(B))
    wide = np.float32(np.float32(np.sum(a["cost"].astype(np.float64))) / np.float32(B))
    assert e != bits(pairwise) and e != bits(wide), "error does not tell the summation order"
    assert bits(z["a10_perm_error"]) != e, "the permutation's error equals the identity's"
    # the recorded layers
    c1 = z["a10_c1"].reshape(-1, 16, 30, 30)
    p1 = z["a10_p1"].reshape(-1, 16, 14, 14)
    c2 = z["a10_c2"].reshape(-1, 64, 12, 12)
    p2 = z["a10_p2"].reshape(-1, 64, 3, 3)
    for name, node in (("C1", c1), ("C2", c2)):
        assert (node < 0).any() and (node > 0).any(), f"{name}: one elu side only"
    ties = 0
    for name, top, node, size, stride in (("P1", c1, p1, 3, 2), ("P2", c2, p2, 4, 4)):
        win = windows(top, size, stride)
        assert np.array_equal(bits(win.max(axis=-1)), bits(node)), f"{name} is not its windows' maximum"
        assert (win.argmax(axis=-1) != 0).any(), f"{name}: every maximum is in first place"
        ties += int(((win == node[..., None]).sum(axis=-1) >= 2).sum())
    assert ties > 0, "no pool window with a tie for its maximum"
    for name in ("local4", "local5"):
        node = z[f"a10_{name}"]
        assert (node == 0).any() and (node > 0).any(), f"{name}: one relu side only"
    # a mirror that reads C1's maps 900 apart from the reference's node would mis-index
    stride = int(np.asarray(z["c1_chan_stride"]).reshape(-1)[0])
    assert stride == 904 and 1 * stride + 0 != 1 * 900 + 0  # where map 1 begins, in the node and in the mirror


def record(out_path: str, reference: str = DEFAULT_REFERENCE) -> None:
    tmp = tempfile.mkdtemp(prefix="cifar_golden_")
    try:
        exe = build_driver(reference, tmp)
        z = {"digest": np.frombuffer(R.input_digest().encode(), np.uint8)}

        def store(name, out):
            for k in R.FIELDS:
                z[f"{name}_{k}"] = out[k]
        for classes in (10, 100):
            w, b, x, labels = R.main_case(classes)
            first = classes == 10
            out = run(exe, tmp, classes, w, b, x, labels, R.PERM if first else None, R.N_PROBS,
                      R.N_LAYERS if first else 0)
            store(f"a{classes}", out)
            if first:
                z["a10_perm_error"], z["a10_perm_accuracy"], z["a10_perm_correct"] = out["perm"]
                z["c1_chan_stride"] = np.int32(out["c1_chan_stride"])
                for k, v in out["layers"].items():
                    z[f"a10_{k}"] = v
        for name, contract, w, b, x, labels in R.edge_cases():
            store(name, run(exe, tmp, 10, w, b, x, labels))
        z = {k: np.ascontiguousarray(v) for k, v in z.items()}
        if os.environ.get("CIFAR_GOLDEN_REPORT"):
            for n in ("a10", "a100"):
                print(n, "pred", np.unique(z[f"{n}_pred"], return_counts=True), "correct", z[f"{n}_correct"][-1])
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
    out = args[0] if args else os.path.join(HERE, "cifar_ref.npz")
    record(out, ref)
    print(out, os.path.getsize(out), "bytes")
