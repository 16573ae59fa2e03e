"""tests/golden/client_grad_ref.npz: the client's getGradients (Client/app/src/main/cpp/
cppNN-lib.cpp:101-113, 218-234: B train_class calls, then cnn.gradients()) recorded from the
reference's own network class by tests/golden/make_client_grad_golden.py, and the seeded inputs
it was recorded from. The fixture holds recorded values only; images, labels and weights are
regenerated here (eval_ref.py's generators and weight scales), and `digest` catches drift.

Cases (CASES): name, B, teacher (1: the forward runs at TEMPERATURE 2, as the client's call
does; 0: temperature 1), mode (0: the shifts are given, 1: train_class draws them from rand()
after srand(seed)), seed, first image, labels, shifts.
  z          B = 1, zero shift, temperature 2
  s_<dx><dy> B = 1, z's sample under each of the eight other shifts
  blank      B = 1, every pixel -1 (an empty MNIST image)
  badlabel   B = 1, label 10: the target is all zeros
  t1         z's sample at temperature 1
  b2, b5     B = 2 and B = 5, shifts drawn by the reference's rand() (mode 1)

Recorded per case (fields of `<name>_...`):
  input[B][784]   the shifted input layer of every sample
  E[B]            train_class's E
  grad[22961]     cnn.gradients()
  FULL cases (z, blank, badlabel, t1) also hold every layer's node and delta after
  backward_hidden's first pass (node_<L>, delta_<L>) and both pools' p_map (pmap_P1, pmap_P2).
The eight shift cases hold input, E, node_FC2, and of their gradient vector the C1 weight block
and the I1 bias block (grad_c1, grad_i1: the two blocks the input layer enters directly) plus
grad_sha256 over all 22961 values: eight more full vectors would take the fixture past the size of the largest
golden, and a digest still pins every bit.
"""
import hashlib
import os

import numpy as np

import eval_ref as E

f = np.float32
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "client_grad_ref.npz")
N_W, N_B, PIX, N_UP = E.N_W, E.N_B, E.PIX, 22961
LAYERS = ("I1", "C1", "P1", "C2i", "C2", "P2", "FC2")
SIZES = (784, 4608, 512, 1024, 768, 192, 10)
N_NODES = sum(SIZES)  # 7898
SHIFTS8 = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
FULL = ("z", "blank", "badlabel", "t1")
SEED_B2, SEED_B5 = 11, 5
# the C1 weight block and the I1 bias block inside gradients(): [6, 200, C1.., 0, 128, ...]
G_C1 = slice(2, 202)
G_I1 = slice(N_W + 9, N_W + 9 + 784)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def model():
    return E.model_a()


def images(n=8, seed=424242):
    return E.images_a(n, seed=seed)


def labels(n=8, seed=17):
    return np.random.RandomState(seed).randint(0, 10, n).astype(np.int32)


def shift_edge(img, dx, dy):
    """matrix::shift(dx, dy, mojo::edge) (core_math.h:721-731): pad by replication, crop:
    out[y][x] = in[clamp(y - dy)][clamp(x - dx)]"""
    a = np.asarray(img, f).reshape(28, 28)
    yy = np.clip(np.arange(28) - dy, 0, 27)
    xx = np.clip(np.arange(28) - dx, 0, 27)
    return a[np.ix_(yy, xx)].reshape(-1).copy()


def cases():
    """[(name, B, teacher, mode, seed, images[B][784], labels[B], shifts[B][2])]"""
    x, lab = images(), labels()
    zero = np.zeros((1, 2), np.int32)
    out = [("z", 1, 1, 0, 0, x[:1], lab[:1], zero)]
    for dx, dy in SHIFTS8:
        out.append((shift_name(dx, dy), 1, 1, 0, 0, x[:1], lab[:1], np.array([[dx, dy]], np.int32)))
    out.append(("blank", 1, 1, 0, 0, np.full((1, PIX), -1.0, f), np.array([0], np.int32), zero))
    out.append(("badlabel", 1, 1, 0, 0, x[1:2], np.array([10], np.int32), zero))
    out.append(("t1", 1, 0, 0, 0, x[:1], lab[:1], zero))
    out.append(("b2", 2, 1, 1, SEED_B2, x[1:3], lab[1:3], np.zeros((2, 2), np.int32)))
    out.append(("b5", 5, 1, 1, SEED_B5, x[3:8], lab[3:8], np.zeros((5, 2), np.int32)))
    return out


def shift_name(dx, dy):
    return "s_" + "mzp"[dx + 1] + "mzp"[dy + 1]


def temperature_of(teacher):
    return 2.0 if teacher else 1.0


def input_digest():
    h = hashlib.sha256()
    w, b = model()
    h.update(w.tobytes() + b.tobytes())
    for name, B, teacher, mode, seed, x, lab, sh in cases():
        h.update(name.encode() + bytes([B, teacher, mode, seed]))
        for a in (x, lab, sh):
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load(path=PATH):
    return np.load(path)


def recorded_shifts(z, name, x):
    """the (dx, dy) of every sample of a case, read off its recorded input layers"""
    out = []
    for k, rec in enumerate(z[f"{name}_input"]):
        hit = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
               if (bits(shift_edge(x[k], dx, dy)) == bits(rec)).all()]
        assert len(hit) == 1, (name, k, hit)
        out.append(hit[0])
    return np.array(out, np.int32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, f).tobytes()).hexdigest()


def write_flat(path, z):
    """Every case as one flat little-endian file for tests/native/check_client_grad.cpp:
    w[21448], b[82], int32 n; per case int32 name length, the name, int32 B, full, float
    temperature, images[B][784], labels[B], shifts[B][2] (as recorded), input[B][784], E[B];
    full: node[7898], pmap[704], delta[7898], grad[22961]; light (the shift cases):
    node_FC2[10], grad_c1[200], grad_i1[784]; every other case: grad[22961]. (The checker writes
    the vectors it computed to a second file, whose digests the caller compares.)"""
    w, b = model()
    cs = cases()
    with open(path, "wb") as fh:
        fh.write(w.tobytes() + b.tobytes() + np.int32(len(cs)).tobytes())
        for name, B, teacher, mode, seed, x, lab, sh in cs:
            nb = name.encode()
            kind = 1 if name in FULL else (2 if name.startswith("s_") else 0)
            fh.write(np.int32(len(nb)).tobytes() + nb + np.array([B, kind], np.int32).tobytes())
            fh.write(f(temperature_of(teacher)).tobytes())
            shifts = recorded_shifts(z, name, x) if mode else sh
            for a, t in ((x, f), (lab, np.int32), (shifts, np.int32), (z[f"{name}_input"], f), (z[f"{name}_E"], f)):
                fh.write(np.ascontiguousarray(a, dtype=t).tobytes())
            if kind == 1:
                for L in LAYERS:
                    fh.write(np.ascontiguousarray(z[f"{name}_node_{L}"], f).tobytes())
                fh.write(np.ascontiguousarray(z[f"{name}_pmap_P1"], np.int32).tobytes())
                fh.write(np.ascontiguousarray(z[f"{name}_pmap_P2"], np.int32).tobytes())
                for L in LAYERS:
                    fh.write(np.ascontiguousarray(z[f"{name}_delta_{L}"], f).tobytes())
            if kind == 2:
                fh.write(np.ascontiguousarray(z[f"{name}_node_FC2"], f).tobytes())
                fh.write(np.ascontiguousarray(z[f"{name}_grad_c1"], f).tobytes())
                fh.write(np.ascontiguousarray(z[f"{name}_grad_i1"], f).tobytes())
            else:
                fh.write(np.ascontiguousarray(z[f"{name}_grad"], f).tobytes())
