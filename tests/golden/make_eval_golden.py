"""Records tests/golden/eval_ref.npz from the reference's own network class.

    python tests/golden/make_eval_golden.py [OUT.npz] [--reference DIR]

tests/native/ref_eval_driver.cpp is compiled into a temporary directory outside the tree
with the reference's flags (oracle/Makefile: -std=c++11 -O0 -DDISTILLATION_MODE=1
-I<reference>/commonLib/cppNN -w) plus -fno-access-control, run on the seeded inputs of
tests/eval_ref.py (whose docstring lists the cases), and its outputs are stored. Before
anything is written the reference's numbers alone must show that the fixture can tell the
evaluation from its nearest wrong neighbours (conditions(), re-asserted from the fixture by
tests/test_eval_inputs.py). Only recorded values are committed, never the driver's binary."""
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

import eval_ref as R  # noqa: E402

DEFAULT_REFERENCE = "/root/reference"


def build_driver(reference: str, tmp: str) -> str:
    exe = os.path.join(tmp, "ref_eval_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O0", "-DDISTILLATION_MODE=1", "-fno-access-control",
                           f"-I{os.path.join(reference, 'commonLib', 'cppNN')}", "-w",
                           os.path.join(ROOT, "tests", "native", "ref_eval_driver.cpp"), "-o", exe])
    return exe


def parse(raw, B, keep_probs):
    o = 0

    def take(n, t):
        nonlocal o
        a = np.frombuffer(raw, t, n, o).copy()
        o += 4 * n
        return a
    out = {"pred": take(B, np.int32), "p": take(B, np.float32), "cost": take(B, np.float32),
           "probs": take(10 * B, np.float32).reshape(B, 10)[:keep_probs],
           "error": take(B, np.float32), "accuracy": take(B, np.float32), "correct": take(B, np.int32)}
    return out, raw[o:]


def run_class(exe, tmp, w, b, x, labels, perm=None, keep_probs=None):
    B = len(labels)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<ii", B, 0 if perm is None else B))
        for a, t in ((w, np.float32), (b, np.float32), (x, np.float32), (labels, np.int32)):
            fh.write(np.ascontiguousarray(a, t).tobytes())
        if perm is not None:
            fh.write(np.ascontiguousarray(perm, np.int32).tobytes())
    subprocess.check_call([exe, "class", fin, fout], stdout=subprocess.DEVNULL)
    out, rest = parse(open(fout, "rb").read(), B, B if keep_probs is None else keep_probs)
    if perm is not None:
        e, a, c = struct.unpack("<ffi", rest[:12])
        out["perm"] = (np.float32(e), np.float32(a), np.int32(c))
    return out


def run_text(exe, tmp, text, chain, x, labels, keep_probs):
    B = len(labels)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<iii", B, chain, len(text)))
        fh.write(text)
        fh.write(np.ascontiguousarray(x, np.float32).tobytes())
        fh.write(np.ascontiguousarray(labels, np.int32).tobytes())
    subprocess.check_call([exe, "text", fin, fout], stdout=subprocess.DEVNULL)
    out, rest = parse(open(fout, "rb").read(), B, keep_probs)
    wb = np.frombuffer(rest, np.float32)
    assert len(wb) == R.N_W + R.N_B
    out["w"], out["b"] = wb[:R.N_W].copy(), wb[R.N_W:].copy()
    return out


def conditions(z, teacher_probs):
    """What the reference's numbers must show (the issue's three conditions). teacher_probs:
    oracle.teacher_forward(w, b, x, temperature=1.0) of case a's inputs, the train-mode forward."""
    a = R.case(z, "a")
    B = len(a["pred"])
    # 1. the train-mode pools give other bits, and another prediction, for some image
    tp = np.asarray(teacher_probs, np.float32)
    t_pred = np.array([R_argmax(row) for row in tp])
    t_p = tp[np.arange(B), t_pred]
    assert (R.bits(t_p) != R.bits(a["p"])).any(), "train-mode pools give the same p everywhere"
    assert (t_pred != a["pred"]).any(), "train-mode pools give the same predictions everywhere"
    # 2. the ordered binary32 sum differs from the pairwise and the float64 sums
    e = R.bits(a["error"][-1])
    pairwise = np.float32(np.sum(a["cost"], dtype=np.float32) / np.float32(B))
    wide = np.float32(np.float32(np.sum(a["cost"].astype(np.float64))) / np.float32(B))
    assert e != R.bits(pairwise) and e != R.bits(wide), "error does not tell the summation order"
    assert R.bits(z["a_perm_error"]) != e, "the permutation's error equals the identity's"
    # 3. at least five classes predicted, right and wrong answers both
    assert len(np.unique(a["pred"])) >= 5, np.unique(a["pred"])
    assert 0 < int(a["correct"][-1]) < B


def R_argmax(out):
    """network.h:146-153 arg_max"""
    m = 0
    for j in range(len(out)):
        if out[m] < out[j]:
            m = j
    return m


def teacher_probs_a():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    pyoracle.build()
    w, b = R.model_a()
    return pyoracle.Oracle().teacher_forward(w, b, R.images_a(), temperature=1.0)


def record(out_path: str, reference: str = DEFAULT_REFERENCE) -> None:
    tmp = tempfile.mkdtemp(prefix="eval_golden_")
    try:
        exe = build_driver(reference, tmp)
        z = {"digest": np.frombuffer(R.input_digest().encode(), np.uint8)}
        x, labels = R.images_a(), R.labels_a()
        w, b = R.model_a()

        def store(name, out):
            for k in R.FIELDS:
                z[f"{name}_{k}"] = out[k]
        out = run_class(exe, tmp, w, b, x, labels, R.PERM, R.N_PROBS)
        store("a", out)
        z["a_perm_error"], z["a_perm_accuracy"], z["a_perm_correct"] = out["perm"]
        text = R.seeded_text()
        for chain, name in enumerate(("b_text", "b_copy", "b_bcast")):
            out = run_text(exe, tmp, text, chain, x, labels, R.N_PROBS)
            store(name, out)
            z[f"{name}_w"], z[f"{name}_b"] = out["w"], out["b"]
        for name, contract, w, b, x, labels in R.edge_cases():
            store(name, run_class(exe, tmp, w, b, x, labels))
        z = {k: np.ascontiguousarray(v) for k, v in z.items()}
        conditions(z, teacher_probs_a())
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
    out = args[0] if args else os.path.join(HERE, "eval_ref.npz")
    record(out, ref)
    print(out, os.path.getsize(out), "bytes")
