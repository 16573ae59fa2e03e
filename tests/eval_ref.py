"""tests/golden/eval_ref.npz: the Driver's test() (Driver/src/main/c++/cppNN_backend.cpp:53-75)
recorded from the reference's own network class by tests/golden/make_eval_golden.py, and the
seeded inputs it was recorded from. The fixture holds recorded results only; images, labels
and weights are regenerated here from seeds (RandomState streams and single binary32
operations, the same bits on every machine), and the fixture's `digest` catches a generator
that drifts.

Cases, each with pred[B], p[B], cost[B], probs[B][10] and, per prefix length k + 1,
error[k], accuracy[k], correct[k] (what test(..., sample = k + 1) returns):
  a        class level: the network of :109-115 built by push_back, model_a() set; also
           a_perm_error / _accuracy / _correct: test() over images[PERM]
  b_text   text level: cnn.read of model_mnist_seeded.npz's text
  b_copy   the server's version copy of that text (initUpdater's models[0])
  b_bcast  the mode-1 broadcast text of that copy (getParametersNative), read again
  c_*      edges (edge_cases()), contract 1 (no NaN among the inputs: bitwise) or 2 (NaN
           inputs: NaN at the same positions, every other value bitwise)
"""
import hashlib
import os

import numpy as np

f = np.float32
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_ref.npz")
SEEDED_MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_mnist_seeded.npz")

N_W, N_B, PIX = 21448, 82, 784
W_SPLITS = (0, 200, 328, 19528, 21448)  # C1, C2i, C2, FC2 in the weight vector
B_SPLITS = (0, 8, 24, 72, 82)
B_A = 600       # images of the main cases
N_PROBS = 8     # images whose ten probabilities the fixture keeps for the main cases
FIELDS = ("pred", "p", "cost", "probs", "error", "accuracy", "correct")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def images_a(n=B_A, seed=20250117):
    """n images of 784 pixels in [-1, 1] like mnist_parser's, each a few soft strokes of its
    own on a dark ground, so that the network's answer changes from image to image."""
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:28, 0:28].astype(np.float64)
    out = np.empty((n, PIX), f)
    for k in range(n):
        img = np.zeros((28, 28))
        for _ in range(r.randint(1, 5)):
            cy, cx = r.uniform(4, 24, 2)
            sy, sx = r.uniform(1.0, 6.0, 2)
            img += r.uniform(0.5, 1.5) * np.exp(-((yy - cy) / sy) ** 2 - ((xx - cx) / sx) ** 2)
        img = np.clip(img + r.normal(0, 0.05, (28, 28)), 0.0, 1.0)
        out[k] = (np.round(img * 255.0) / 255.0 * 2.0 - 1.0).astype(f).reshape(-1)
    return out


def labels_a(n=B_A, seed=99):
    return np.random.RandomState(seed).randint(0, 10, n).astype(np.int32)


def model_a(seed=2):
    """(w, b): normal weights scaled per layer by its fan-in; the convolutions' biases lean
    negative, so that elu's negative side and pool windows without a positive value are common"""
    r = np.random.RandomState(seed)
    w = np.empty(N_W, f)
    b = np.empty(N_B, f)
    for k, (fan, gain) in enumerate(((25, 1.5), (8, 1.5), (400, 1.5), (192, 6.0))):
        lo, hi = W_SPLITS[k], W_SPLITS[k + 1]
        w[lo:hi] = (r.normal(0, 1, hi - lo) * gain / np.sqrt(fan)).astype(f)
        b[B_SPLITS[k]:B_SPLITS[k + 1]] = r.normal(-0.3 if k < 3 else 0.0, 0.2, B_SPLITS[k + 1] - B_SPLITS[k]).astype(f)
    return w, b


PERM = np.random.RandomState(7).permutation(B_A).astype(np.int32)


def seeded_text():
    return bytes(np.load(SEEDED_MODEL)["text"])


def edge_cases():
    """[(name, contract, w, b, images, labels)]"""
    w0, b0 = model_a()
    x0 = images_a(6, seed=31337)
    lab = np.array([0, 3, 7, 9, 1, 5], np.int32)
    out = []
    # all-zero weights and biases: ten equal probabilities, argm 0; every pool window 0 + 0
    out.append(("c_zero", 1, np.zeros(N_W, f), np.zeros(N_B, f), x0[:4], np.array([0, 1, 0, 9], np.int32)))
    # two classes with the same FC2 row: their probabilities tie; the other rows are zero
    w = w0.copy()
    fc = w[W_SPLITS[3]:].reshape(10, 192)
    row = fc[3].copy()
    fc[:] = 0
    fc[3] = fc[7] = row
    out.append(("c_tie", 1, w, b0.copy(), x0, np.array([3, 7, 0, 3, 7, 0], np.int32)))
    # C1 silent on half its maps (zero weights, zero bias: windows with max + max2 == 0), the rest as seeded
    w = w0.copy()
    b = b0.copy()
    w[:100] = 0
    b[:4] = 0
    out.append(("c_denom_zero", 1, w, b, x0, lab))
    # strongly negative biases: elu's negative side, pool windows of mixed sign and all negative
    w = w0.copy()
    b = b0.copy()
    b[:72] = (b[:72] - f(0.6)).astype(f)
    w[:328] = (w[:328] * f(2.0)).astype(f)
    out.append(("c_mixed_sign", 1, w, b, x0, lab))
    # +-inf pixels
    x = x0.copy()
    x[0, 100] = np.inf
    x[1, 400] = -np.inf
    x[2, 5] = np.inf
    x[2, 700] = -np.inf
    x[3, 783] = np.inf
    out.append(("c_inf_pixels", 1, w0.copy(), b0.copy(), x, lab))
    # one NaN weight (C2, one map's tap): the NaN rule
    w = w0.copy()
    w[W_SPLITS[2] + 25 * (3 * 48 + 11) + 7] = np.nan
    out.append(("c_nan_weight", 2, w, b0.copy(), x0, lab))
    # labels outside 0..9, some beyond binary32's integers
    out.append(("c_labels", 1, w0.copy(), b0.copy(), x0,
                np.array([-3, 10, 1000000, 2 ** 31 - 1, -2 ** 31, 16777217], np.int32)))
    return out


def input_digest():
    """sha256 over every generated input, in a fixed order"""
    h = hashlib.sha256()
    w, b = model_a()
    for a in (images_a(), labels_a(), w, b, PERM):
        h.update(np.ascontiguousarray(a).tobytes())
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
    """test()'s error over these costs: added in binary32 in order from 0.f, divided by (float)B
    (single IEEE operations; tests/test_eval_inputs.py proves it equal to every recorded prefix)"""
    s = f(0.0)
    with np.errstate(all="ignore"):
        for c in np.asarray(cost, f):
            s = f(s + c)
        return f(s / f(len(cost)))


def accuracy_of(correct, B):
    return f(f(f(correct) / f(B)) * f(100.0))


def mismatch(contract, got, want):
    """'' when `got` meets the contract against the recorded `want`, else what differs
    (tests/teacher_edges.py's contract: 1 bitwise, 2 NaN positions and every other value)"""
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


def write_flat(path, z):
    """Every case as one flat little-endian file for tests/native/check_eval_forward.cpp: int32 n,
    then per case int32 name length, the name, int32 contract, B, n_probs, has_perm; w[21448],
    b[82], x[B*784], labels[B], pred[B], p[B], cost[B], probs[n_probs*10], error[B], accuracy[B],
    correct[B]; with a permutation perm[B], error, accuracy, correct."""
    w, b = model_a()
    cases = [("a", 1, w, b, images_a(), labels_a())]
    if "b_text_w" in z:
        for name in ("b_text", "b_copy", "b_bcast"):
            cases.append((name, 1, z[f"{name}_w"], z[f"{name}_b"], images_a(), labels_a()))
    cases += edge_cases()
    with open(path, "wb") as fh:
        fh.write(np.int32(len(cases)).tobytes())
        for name, contract, w, b, x, lab in cases:
            c = case(z, name)
            nb = name.encode()
            perm = name == "a"
            fh.write(np.int32(len(nb)).tobytes() + nb)
            fh.write(np.array([contract, len(lab), len(c["probs"]), int(perm)], np.int32).tobytes())
            for a, t in ((w, f), (b, f), (x, f), (lab, np.int32), (c["pred"], np.int32), (c["p"], f), (c["cost"], f),
                         (c["probs"], f), (c["error"], f), (c["accuracy"], f), (c["correct"], np.int32)):
                fh.write(np.ascontiguousarray(a, dtype=t).tobytes())
            if perm:
                fh.write(np.ascontiguousarray(PERM, np.int32).tobytes())
                fh.write(np.float32(z["a_perm_error"]).tobytes() + np.float32(z["a_perm_accuracy"]).tobytes() +
                         np.int32(z["a_perm_correct"]).tobytes())
