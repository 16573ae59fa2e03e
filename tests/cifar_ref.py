"""tests/golden/cifar_ref.npz: the Driver's test() (Driver/src/main/c++/cppNN_backend.cpp:53-75)
on the reference's CIFAR network (:128-138), recorded from the reference's own network class by
tests/golden/make_cifar_golden.py, and the seeded inputs it was recorded from. The fixture
holds recorded results only; images, labels and weights are regenerated here from seeds
(RandomState streams and single binary32 operations, the same bits on every machine), and the
fixture's `digest` catches a generator that drifts.

Cases, each with pred[B], p[B], cost[B], probs[n][N] (the first N_PROBS images of a main case,
every image of an edge) and, per prefix length k + 1, error[k], accuracy[k], correct[k]:
  a10      N = 10, B = 160; also a10_perm_error / _accuracy / _correct (test() over
           images[PERM]) and, for the first N_LAYERS images, every layer's node: a10_c1
           [n][16][900] (the reference's padding of four floats per map dropped), a10_p1,
           a10_c2, a10_p2, a10_local4, a10_local5, a10_fc2
  a100     N = 100, B = 64
  c_*      edges at N = 10 (edge_cases()), contract 1 (no NaN among the inputs: bitwise) or 2
           (NaN inputs: NaN at the same positions, every other value bitwise)
c1_chan_stride: the distance of C1's maps in the reference's own node (904).
"""
import hashlib
import os
import subprocess

import numpy as np

f = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PATH = os.path.join(HERE, "golden", "cifar_ref.npz")

PIX = 3072
W_SIZES = {10: (432, 9216, 221184, 73728, 1920), 100: (432, 9216, 221184, 73728, 19200)}  # C1, C2, local4, local5, FC2
B_SIZES = {10: (16, 64, 384, 192, 10), 100: (16, 64, 384, 192, 100)}
FANS = (27, 144, 576, 384, 192)
B_MAIN = {10: 160, 100: 64}
N_PROBS = 4
N_LAYERS = 2
FIELDS = ("pred", "p", "cost", "probs", "error", "accuracy", "correct")
LAYERS = (("c1", (16, 900)), ("p1", (16, 196)), ("c2", (64, 144)), ("p2", (64, 9)), ("local4", (384,)),
          ("local5", (192,)), ("fc2", (10,)))
LAYER_FLOATS = sum(int(np.prod(s)) for _, s in LAYERS)


def n_w(classes):
    return sum(W_SIZES[classes])


def n_b(classes):
    return sum(B_SIZES[classes])


def w_splits(classes):
    return np.concatenate([[0], np.cumsum(W_SIZES[classes])])


def b_splits(classes):
    return np.concatenate([[0], np.cumsum(B_SIZES[classes])])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def images(n, seed):
    """n images of 3 x 32 x 32 in [-1, 1], planar as cifar_parser.h delivers them (pixel / 255 * 2
    - 1): per channel a level of its own, a few blobs of either sign, a gradient in some, and
    noise inside one rectangle only, so that flat ground (equal convolution outputs: ties in the
    pool windows) and busy ground both occur and the answer changes from image to image. Every
    image also carries one 10 x 10 patch of a single level per channel."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:32, 0:32].astype(np.float64)
    out = np.empty((n, PIX), f)
    for k in range(n):
        img = np.empty((3, 32, 32))
        style = r.randint(0, 4)
        fy, fx = r.randint(0, 22, 2)
        for c in range(3):
            ch = np.full((32, 32), r.uniform(0.05, 0.95))
            for _ in range(r.randint(1, 5)):
                cy, cx = r.uniform(2, 30, 2)
                sy, sx = r.uniform(1.0, 7.0, 2)
                ch += r.uniform(-1.0, 1.0) * np.exp(-((yy - cy) / sy) ** 2 - ((xx - cx) / sx) ** 2)
            if style == 1:
                ch += r.uniform(-0.5, 0.5) * (xx / 31.0) + r.uniform(-0.5, 0.5) * (yy / 31.0)
            if style == 2:
                ch += r.uniform(0.1, 0.4) * np.sign(np.sin(xx * r.uniform(0.3, 1.5) + yy * r.uniform(0.3, 1.5)))
            y0, x0 = r.randint(0, 16, 2)
            ch[y0:y0 + 14, x0:x0 + 14] += r.normal(0, 0.08, (14, 14))
            ch[fy:fy + 10, fx:fx + 10] = r.uniform(0.1, 0.9)
            img[c] = ch
        img = np.clip(img, 0.0, 1.0)
        out[k] = (np.round(img * 255.0) / 255.0 * 2.0 - 1.0).astype(f).reshape(-1)
    return out


GAINS = {10: (1.6, 1.6, 1.6, 1.6, 2.5), 100: (1.6, 1.6, 1.6, 1.6, 2.5)}


def model(classes, seed):
    """(w, b): normal weights scaled per layer by its fan-in; the convolutions' biases lean
    negative (elu's negative side, windows without a positive value), the fc layers' biases
    straddle zero (both relu sides)"""
    r = np.random.RandomState(seed)
    ws, bs = w_splits(classes), b_splits(classes)
    w = np.empty(n_w(classes), f)
    b = np.empty(n_b(classes), f)
    for k in range(5):
        w[ws[k]:ws[k + 1]] = (r.normal(0, 1, ws[k + 1] - ws[k]) * GAINS[classes][k] / np.sqrt(FANS[k])).astype(f)
        b[bs[k]:bs[k + 1]] = r.normal(-0.25 if k < 2 else -0.1, 0.25, bs[k + 1] - bs[k]).astype(f)
    return w, b


# N = 100: uniform labels would be right about once in 64 images; these are drawn from a pool
# of classes the seeded model predicts (20, 33, 56, 99) and some it does not
LABEL_POOL = {10: None, 100: (20, 33, 56, 99, 7, 12, 61, 85)}


def main_case(classes):
    """(w, b, images, labels) of a10 / a100"""
    B = B_MAIN[classes]
    w, b = model(classes, 10 + classes)
    x = images(B, 20251021 + classes)
    r = np.random.RandomState(100 + classes)
    pool = LABEL_POOL[classes]
    labels = (r.randint(0, classes, B) if pool is None else np.asarray(pool)[r.randint(0, len(pool), B)]).astype(np.int32)
    return w, b, x, labels


PERM = np.random.RandomState(7).permutation(B_MAIN[10]).astype(np.int32)


def edge_cases():
    """[(name, contract, w, b, images, labels)], N = 10"""
    w0, b0 = model(10, 20)
    ws, bs = w_splits(10), b_splits(10)
    x0 = images(6, 31337)
    lab = np.array([0, 3, 7, 9, 1, 5], np.int32)
    out = []
    # all-zero weights and biases: ten equal probabilities, argm 0; every pool window a tie
    out.append(("c_zero", 1, np.zeros(n_w(10), f), np.zeros(n_b(10), f), x0[:4], np.array([0, 1, 0, 9], np.int32)))
    # two classes with the same FC2 row: their probabilities tie; the other rows are zero
    w = w0.copy()
    fc = w[ws[4]:].reshape(10, 192)
    row = np.abs(fc[3])
    fc[:] = 0
    fc[3] = fc[7] = row
    out.append(("c_tie", 1, w, b0.copy(), x0, np.array([3, 7, 0, 3, 7, 0], np.int32)))
    # strongly negative convolution biases: elu's negative side, pool windows all negative
    b = b0.copy()
    b[:bs[2]] = (b[:bs[2]] - f(1.5)).astype(f)
    out.append(("c_neg_bias", 1, w0.copy(), b, x0, lab))
    # biases that silence local4: relu all zero, local5 sees its bias alone
    b = b0.copy()
    b[bs[2]:bs[3]] = f(-1.0e6)
    out.append(("c_relu_silent", 1, w0.copy(), b, x0[:4], lab[:4]))
    # +-inf pixels
    x = x0.copy()
    x[0, 100] = np.inf
    x[1, 1024 + 400] = -np.inf
    x[2, 5] = np.inf
    x[2, 2048 + 700] = -np.inf
    x[3, 3071] = np.inf
    out.append(("c_inf_pixels", 1, w0.copy(), b0.copy(), x, lab))
    # one NaN weight (C2, one map's tap of one channel): the NaN rule
    w = w0.copy()
    w[ws[1] + 9 * (11 + 3 * 64) + 4] = np.nan
    out.append(("c_nan_weight", 2, w, b0.copy(), x0, lab))
    # one NaN pixel at (4, 4) of channel 0: C1 is NaN at rows and columns 2..4, so the P1
    # window of row 1, column 1 has the NaN in its first place (it stays) and the window of
    # row 0, column 0 has it in its last (it never wins)
    x = x0.copy()
    x[:, 4 * 32 + 4] = np.nan
    out.append(("c_nan_pixel", 2, w0.copy(), b0.copy(), x[:4], lab[:4]))
    # labels outside 0..9, some beyond binary32's integers
    out.append(("c_labels", 1, w0.copy(), b0.copy(), x0,
                np.array([-3, 10, 1000000, 2 ** 31 - 1, -2 ** 31, 16777217], np.int32)))
    return out


def input_digest():
    """sha256 over every generated input, in a fixed order"""
    h = hashlib.sha256()
    for classes in (10, 100):
        for a in main_case(classes):
            h.update(np.ascontiguousarray(a).tobytes())
    h.update(PERM.tobytes())
    for name, contract, w, b, x, lab in edge_cases():
        h.update(name.encode() + bytes([contract]))
        for a in (w, b, x, lab):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load(path=PATH):
    return np.load(path)


def case(z, name):
    """the recorded fields of one case as a dict"""
    return {k: z[f"{name}_{k}"] for k in FIELDS}


def ordered_error(cost):
    """test()'s error over these costs: added in binary32 in order from 0.f, divided by (float)B"""
    s = f(0.0)
    with np.errstate(all="ignore"):
        for c in np.asarray(cost, f):
            s = f(s + c)
        return f(s / f(len(cost)))


def accuracy_of(correct, B):
    return f(f(f(correct) / f(B)) * f(100.0))


def mismatch(contract, got, want):
    """'' when `got` meets the contract against the recorded `want`, else what differs"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    if got.dtype.kind != "f":
        bad = got != want
    else:
        g, r = bits(got), bits(want)
        if contract == 1:
            bad = g != r
        else:
            gn, rn = np.isnan(got), np.isnan(want)
            bad = (gn != rn) | (~rn & (g != r))
    if not bad.any():
        return ""
    k = tuple(int(v) for v in np.argwhere(bad)[0])
    return f"{int(bad.sum())} of {bad.size} values differ; first at {k}: got {got[k]!r}, recorded {want[k]!r}"


def all_cases():
    """[(name, contract, classes, w, b, images, labels)]: the main cases, then the edges"""
    out = [(f"a{n}", 1, n) + main_case(n) for n in (10, 100)]
    return out + [(name, contract, 10, w, b, x, lab) for name, contract, w, b, x, lab in edge_cases()]


def write_flat(path, z):
    """Every case as one flat little-endian file for tests/native/check_cifar_forward.cpp: int32 n,
    then per case int32 name length, the name, int32 contract, N, B, n_probs, has_perm, n_layers;
    w, b, x[B*3072], labels[B], pred[B], p[B], cost[B], probs[n_probs*N], error[B], accuracy[B],
    correct[B]; per image of the first n_layers the nodes in LAYERS order; with a permutation
    perm[B], error, accuracy, correct."""
    with open(path, "wb") as fh:
        cases = all_cases()
        fh.write(np.int32(len(cases)).tobytes())
        for name, contract, classes, w, b, x, lab in cases:
            c = case(z, name)
            nb = name.encode()
            perm = name == "a10"
            n_layers = N_LAYERS if name == "a10" else 0
            fh.write(np.int32(len(nb)).tobytes() + nb)
            fh.write(np.array([contract, classes, len(lab), len(c["probs"]), int(perm), n_layers], np.int32).tobytes())
            for a, t in ((w, f), (b, f), (x, f), (lab, np.int32), (c["pred"], np.int32), (c["p"], f), (c["cost"], f),
                         (c["probs"], f), (c["error"], f), (c["accuracy"], f), (c["correct"], np.int32)):
                fh.write(np.ascontiguousarray(a, dtype=t).tobytes())
            for k in range(n_layers):
                for lname, _ in LAYERS:
                    fh.write(np.ascontiguousarray(z[f"{name}_{lname}"][k], f).tobytes())
            if perm:
                fh.write(PERM.tobytes())
                fh.write(np.float32(z["a10_perm_error"]).tobytes() + np.float32(z["a10_perm_accuracy"]).tobytes() +
                         np.int32(z["a10_perm_correct"]).tobytes())


# ------------------------------------------------------------------ the host mirror, for other shapes

def build_checker(out_dir, flags=()):
    """tests/native/check_cifar_forward.cpp compiled into out_dir; None without a clang++"""
    from test_native_math import _clang
    clang = _clang()
    if clang is None:
        return None
    exe = os.path.join(str(out_dir), "check_cifar_forward")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "native", "check_cifar_forward.cpp"), "-o", exe])
    return exe


def mirror(exe, work_dir, jobs):
    """cifar_forward.h's host form over jobs [(classes, w, b, images[n, 3072], labels[n], idx or None)]:
    per job a dict of pred, p, cost, probs [B, N], error, accuracy, correct (check_cifar_forward
    --mirror; B = len(idx), or n without indices)."""
    fin, fout = os.path.join(str(work_dir), "mirror_in.bin"), os.path.join(str(work_dir), "mirror_out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.int32(len(jobs)).tobytes())
        for classes, w, b, x, lab, idx in jobs:
            x = np.ascontiguousarray(x, f).reshape(len(lab), PIX)
            B = len(lab) if idx is None else len(idx)
            fh.write(np.array([classes, B, len(lab), int(idx is not None)], np.int32).tobytes())
            for a, t in ((w, f), (b, f), (x, f), (lab, np.int32)):
                fh.write(np.ascontiguousarray(a, dtype=t).tobytes())
            if idx is not None:
                fh.write(np.ascontiguousarray(idx, np.int32).tobytes())
    subprocess.check_call([exe, "--mirror", fin, fout], stdout=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    out, o = [], 0
    for classes, w, b, x, lab, idx in jobs:
        B = len(lab) if idx is None else len(idx)

        def take(n, t):
            nonlocal o
            a = np.frombuffer(raw, t, n, o).copy()
            o += 4 * n
            return a
        out.append({"pred": take(B, np.int32), "p": take(B, f), "cost": take(B, f),
                    "probs": take(B * classes, f).reshape(B, classes), "error": take(1, f)[0],
                    "accuracy": take(1, f)[0], "correct": int(take(1, np.int32)[0])})
    assert o == len(raw)
    return out
