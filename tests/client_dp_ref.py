"""tests/golden/client_dp_ref.npz: the client's getGradients with sigma > 0 (cnn.DPgradients(C,
sigma), commonLib/cppNN/network.h:1092-1181) and under start_epoch("distillation")
(Client/app/src/main/cpp/cppNN-lib.cpp:218-221, 251-252), recorded from the reference's own
network class by tests/golden/make_client_dp_golden.py, and the seeded inputs it was recorded
from. The fixture holds recorded values only; images, labels, shifts and weights are regenerated
here (client_grad_ref.py's generators), and `digest` catches drift.

Cases (CASES): name, B, cost (0 cross_entropy, 1 distillation), clip, sigma, images. Every
forward runs at TEMPERATURE 2 (the client passes a teacher_prob), shifts are given.
  a   B = 1, sigma > 0: noise, and no clip loop
  b   B = 2
  c   B = 4, clip between the recorded norms of samples 1-3 and below sample 0's
  d   B = 4, c's samples, clip above every norm; clip * sigma is c's, so the draws are c's
  e1  distillation, B = 1, sigma = 0
  e3  distillation, B = 3, sigma = 0
  f   distillation with c's clip and sigma, c's samples

Recorded per case (fields of `<name>_...`):
  E[B], node_FC2[B][10], delta_FC2[B][10]   after train_class
  sqsum[B], sqsum_layout[B], norm[B], scale[B]   scale_gradients' walk per batch slot, restated
      by the recorder over the reference's own dW_sets (sqsum_layout: the same squares added in
      the gradients() order; slot 0 is recorded though the reference never clips it)
  grad_sha256, grad_i1[784], grad_fc2[10]   the vector's digest and its first and last bias block
  grad[22961]   the whole vector, for the cases of FULL
and once: z_sha256 over the bytes of the first 22961 draws of std::normal_distribution<double>(0,
1) on a default-constructed std::default_random_engine, z_head[32], z_tail[32]; c_d_dw_differ: whether
c's and d's vectors differ in any dW block (a recorded fact).
"""
import hashlib
import os

import numpy as np

import client_grad_ref as G

f = np.float32
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "client_dp_ref.npz")
N_UP = G.N_UP
TEMPERATURE = 2.0
FULL = ("a", "c", "e3")
# chosen from the norms the reference recorded for c's samples (make_client_dp_golden.py asserts
# that samples 1-3 fall on both sides of CLIP_C and that sample 0 lies above it)
CLIP_C, SIGMA_C = 35.0, 1.0 / 128
CLIP_D, SIGMA_D = CLIP_C * 64, SIGMA_C / 64  # the same float product
PICK_C = [5, 4, 6, 7]  # the images of c, d and f: the one of the largest norm takes slot 0
G_I1 = G.G_I1
G_FC2 = slice(N_UP - 10, N_UP)
# the 13 value blocks of gradients(): (start, length), dW then dbias, empty ones left out
BLOCKS = ((2, 200), (204, 128), (333, 19200), (19535, 1920), (21457, 784), (22243, 512), (22758, 192), (22951, 10))
BIAS_START = 21455


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def model():
    return G.model()


def shifts8():
    return np.random.RandomState(33).randint(-1, 2, (8, 2)).astype(np.int32)


def cases():
    """[(name, B, cost, clip, sigma, images[B][784], labels[B], shifts[B][2])]"""
    x, lab, sh = G.images(), G.labels(), shifts8()

    def case(name, cost, clip, sigma, pick):
        return (name, len(pick), cost, clip, sigma, x[pick], lab[pick], sh[pick])
    return [case("a", 0, 1.0, 0.5, [0]), case("b", 0, CLIP_C, 1.0 / 64, [1, 2]), case("c", 0, CLIP_C, SIGMA_C, PICK_C),
            case("d", 0, CLIP_D, SIGMA_D, PICK_C), case("e1", 1, 0.0, 0.0, [0]), case("e3", 1, 0.0, 0.0, [1, 2, 3]),
            case("f", 1, CLIP_C, SIGMA_C, PICK_C)]


def helper_cases():
    """what the recorder compares against and does not store: a without noise, e1 under
    cross_entropy"""
    c = {n: rest for n, *rest in cases()}
    B, cost, clip, sigma, x, lab, sh = c["a"]
    out = [("a_plain", B, 0, 0.0, 0.0, x, lab, sh)]
    B, cost, clip, sigma, x, lab, sh = c["e1"]
    out.append(("e1_ce", B, 0, 0.0, 0.0, x, lab, sh))
    return out


def input_digest():
    h = hashlib.sha256()
    w, b = model()
    h.update(w.tobytes() + b.tobytes())
    for name, B, cost, clip, sigma, x, lab, sh in cases():
        h.update(name.encode() + bytes([B, cost]) + f(clip).tobytes() + f(sigma).tobytes())
        for a in (x, lab, sh):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load(path=PATH):
    return np.load(path)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, f).tobytes()).hexdigest()


def sha_of(z, key):
    return bytes(z[key]).decode()


def write_flat(path, z):
    """Every case as one flat little-endian file for tests/native/check_client_dp.cpp:
    w[21448], b[82], int32 n; per case int32 name length, the
    name, int32 B, cost, full, float clip, sigma, images[B][784], labels[B], shifts[B][2], E[B],
    node_FC2[B][10], delta_FC2[B][10], sqsum[B], norm[B], scale[B], grad_i1[784], grad_fc2[10],
    and grad[22961] where full. (The checker writes the vectors it computed to a second file,
    whose digests the caller compares.)"""
    w, b = model()
    cs = cases()
    with open(path, "wb") as fh:
        fh.write(w.tobytes() + b.tobytes() + np.int32(len(cs)).tobytes())
        for name, B, cost, clip, sigma, x, lab, sh in cs:
            nb = name.encode()
            fh.write(np.int32(len(nb)).tobytes() + nb + np.array([B, cost, name in FULL], np.int32).tobytes())
            fh.write(np.array([clip, sigma], f).tobytes())
            for a, t in ((x, f), (lab, np.int32), (sh, np.int32)):
                fh.write(np.ascontiguousarray(a, dtype=t).tobytes())
            for k in ("E", "node_FC2", "delta_FC2", "sqsum", "norm", "scale", "grad_i1", "grad_fc2"):
                fh.write(np.ascontiguousarray(z[f"{name}_{k}"], f).tobytes())
            if name in FULL:
                fh.write(np.ascontiguousarray(z[f"{name}_grad"], f).tobytes())
