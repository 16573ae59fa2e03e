"""tests/golden/teacher_edges.npz: the teacher's edge cases (tests/test_teacher.py,
tests/native/check_teacher.cpp), recorded from the reference's own mojo network by
tests/golden/make_golden.py teacher_edges.

The file holds data only. To stay small it stores base weight / bias vectors and
image sets once, and per case: the base and image set it uses, one scale per layer
(C1, C2i, C2, FC2) for weights and for biases, sparse overrides (index, binary32
bit pattern -- NaN payloads survive) of weights, biases and pixels, the contract
(1: no NaN among the inputs, bitwise; 2: NaN inputs, see compare()) and the
recorded probabilities. expand() rebuilds the full inputs; the multiplications are
single binary32 roundings, so every machine rebuilds the same bits.
"""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "teacher_edges.npz")

W_SPLITS = (0, 200, 328, 19528, 21448)  # C1, C2i, C2, FC2 in the teacher's weight vector
B_SPLITS = (0, 8, 24, 72, 82)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def _scaled(base, scale, splits):
    out = base.astype(np.float32, copy=True)
    for k in range(4):
        out[splits[k]:splits[k + 1]] = base[splits[k]:splits[k + 1]] * np.float32(scale[k])
    return out


def build_inputs(base_w, base_b, images, wscale, bscale, wo, bo, xo, rows):
    """(w, b, x) of one case. wo / bo / xo: (indices, bit patterns); xo indexes the
    flattened [rows, 784] image block."""
    w = _scaled(base_w, wscale, W_SPLITS)
    b = _scaled(base_b, bscale, B_SPLITS)
    x = images[:rows].astype(np.float32, copy=True)
    for arr, (idx, val) in ((w, wo), (b, bo), (x.reshape(-1), xo)):
        arr.view(np.uint32)[np.asarray(idx, np.int64)] = np.asarray(val, np.uint32)
    return w, b, x


def load(path=PATH):
    """[(name, contract, w, b, x, probs)] of every case."""
    z = np.load(path)
    out = []
    for i, name in enumerate(z["names"]):
        def seg(key):
            lo, hi = z[key + "_off"][i], z[key + "_off"][i + 1]
            return z[key + "_idx"][lo:hi], z[key + "_bits"][lo:hi]
        rows = int(z["rows"][i])
        w, b, x = build_inputs(z["base_w"][z["wbase"][i]], z["base_b"][z["wbase"][i]], z["images"][z["xset"][i]],
                               z["wscale"][i], z["bscale"][i], seg("wo"), seg("bo"), seg("xo"), rows)
        p = z["probs"][z["p_off"][i]:z["p_off"][i] + rows]
        out.append((str(name), int(z["contract"][i]), w, b, x, p))
    return out


def mismatch(contract, got, want):
    """'' when `got` meets the contract against the recorded `want`, else what differs.
    Contract 1: every bit equal. Contract 2: NaN at the same positions, every other
    value bitwise equal (the NaN bit patterns are not pinned)."""
    g, r = bits(got), bits(want)
    if g.shape != r.shape:
        return f"shape {g.shape} != {r.shape}"
    if contract == 1:
        bad = g != r
    else:
        gn, rn = np.isnan(got), np.isnan(want)
        bad = (gn != rn) | (~rn & (g != r))
    if not bad.any():
        return ""
    k = np.argwhere(bad)[0]
    return (f"{int(bad.sum())} of {bad.size} values differ; first at {tuple(int(v) for v in k)}: "
            f"got 0x{int(g[tuple(k)]):08X}, recorded 0x{int(r[tuple(k)]):08X}")


def write_flat(path, cases):
    """The cases as one flat little-endian file for tests/native/check_teacher.cpp:
    int32 n, then per case int32 name length, the name, int32 contract, int32 rows,
    w[21448], b[82], x[rows*784], probs[rows*10] as binary32."""
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for name, contract, w, b, x, p in cases:
            nb = name.encode()
            f.write(np.int32(len(nb)).tobytes() + nb)
            f.write(np.array([contract, x.shape[0]], np.int32).tobytes())
            for a in (w, b, x, p):
                f.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
