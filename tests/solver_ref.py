"""The reference's adagrad, rmsprop and adam steps (commonLib/cppNN/solver.h:97-195) restated
with NumPy float32, one IEEE rounding per operation in the type the source shows, and
network::descent(vector)'s wiring of them over a gradients() layout (network.h:1185-1202,
1334-1353). tests/test_solver_math.py proves the restatement equal, bit for bit, to
tests/golden/solver_ref.npz (recorded from the reference's own classes by
tests/golden/make_solver_golden.py); it is then the expected value for every shape the
fixture does not hold. Also the seeded inputs the fixture was recorded from.

NaN: without NaN among weights, state and gradient every NaN below is x86's default
0xFFC00000 (NumPy runs the same SSE operations), as in the reference. With NaN inputs only
the positions are meaningful (`same_but_nan_payloads`)."""
import numpy as np

f = np.float32
SOLVERS = ("sgd", "adagrad", "rmsprop", "adam")
EPS, ONE = f(1e-8), f(1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


FRESH = (f(0.9), f(0.999))                      # adam's b1_t, b2_t in a fresh solver
SESSION = (f(0.9) * f(0.9), f(0.999) * f(0.999))  # after fetchParamsNative's one reset(): a server session's


def increment_w(solver, w, d, g1, g2, L, bias_terms=FRESH):
    """One increment_w of `solver` on float32 arrays: returns (w, g1, g2); g2 is passed
    through unless the solver is adam. L = the solver's learning_rate; bias_terms =
    adam's (b1_t, b2_t), which nothing changes between the steps of a session."""
    w, d, L = np.asarray(w, f), np.asarray(d, f), f(L)
    with np.errstate(all="ignore"):
        if solver == "sgd":
            return w - (f(1) * L) * (d + f(0) * w), g1, g2
        g1 = np.asarray(g1, f)
        if solver == "adagrad":
            lr = f(1) * L
            g1 = g1 + d * d
            return w - (lr * d) / (np.sqrt(g1) + EPS), g1, g2
        if solver == "rmsprop":
            mu = f(0.999)
            lr = (f(0.01) * f(1)) * L
            g1 = mu * g1 + ((ONE - mu) * d) * d
            return w - (lr * d) / (np.sqrt(g1) + EPS), g1, g2
        assert solver == "adam"
        g2 = np.asarray(g2, f)
        b1, b2, (b1_t, b2_t) = f(0.9), f(0.999), bias_terms
        lr = (f(0.1) * f(1)) * L
        g1 = b1 * g1 + (ONE - b1) * d
        g2 = b2 * g2 + ((ONE - b2) * d) * d
        den = np.sqrt(g2.astype(np.float64) / (np.float64(1.0) - np.float64(b2_t))).astype(f) + EPS
        return w - (lr * (g1 / (ONE - b1_t))) / den, g1, g2


def descent(solver, layout, w, g1, g2, fc_bias, grad, L, bias_terms=FRESH):
    """network::descent(vector) over `layout` (w_sizes, w_present(), b_sizes, fc_flags()):
    increment_w on every present W block with its own slice of the state, update_bias
    (b -= db * L, the plain rate) on the fully-connected layers' bias blocks."""
    w, fc_bias, grad = np.array(w, f), np.array(fc_bias, f), np.asarray(grad, f)
    g1 = None if g1 is None else np.array(g1, f)
    g2 = None if g2 is None else np.array(g2, f)
    idx, wo, bo = 1, 0, 0
    for size, present in zip(layout.w_sizes, layout.w_present()):
        idx += 1
        if present and size:
            s = slice(wo, wo + size)
            nw, n1, n2 = increment_w(solver, w[s], grad[idx:idx + size], None if g1 is None else g1[s],
                                     None if g2 is None else g2[s], L, bias_terms)
            w[s] = nw
            if solver != "sgd":
                g1[s] = n1
            if solver == "adam":
                g2[s] = n2
        if present:
            wo += size
        idx += size
    idx += 1
    for size, fc in zip(layout.b_sizes, layout.fc_flags()):
        idx += 1
        if fc and size:
            with np.errstate(all="ignore"):
                fc_bias[bo:bo + size] = fc_bias[bo:bo + size] - grad[idx:idx + size] * f(L)
        if fc:
            bo += size
        idx += size
    assert idx == len(grad) and wo == len(w) and bo == len(fc_bias)
    return w, g1, g2, fc_bias


def same_but_nan_payloads(a, b):
    """NaN at the same positions, every other value bitwise equal"""
    a, b = np.asarray(a, f), np.asarray(b, f)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


class GradLayout:
    """A gradients() layout for the stateless step (fleet_amd.layouts.Layout's interface,
    with W blocks that may be absent though sized)."""

    def __init__(self, w_sizes, b_sizes, fc_layers, absent=()):
        self.w_sizes, self.b_sizes = tuple(w_sizes), tuple(b_sizes)
        self.fc_layers, self.absent = tuple(fc_layers), tuple(absent)

    def w_present(self):
        return tuple(s > 0 and i not in self.absent for i, s in enumerate(self.w_sizes))

    def fc_flags(self):
        return tuple(k in self.fc_layers for k in range(len(self.b_sizes)))

    @property
    def n_weights(self):
        return sum(s for s, p in zip(self.w_sizes, self.w_present()) if p)

    @property
    def n_fc_bias(self):
        return sum(self.b_sizes[k] for k in self.fc_layers)

    def gradient(self, values):
        """the merged vector: header slots of the layout around `values` (one per flat slot)"""
        out, o = [f(len(self.w_sizes))], 0
        for s in self.w_sizes:
            out += [f(s)] + list(values[o:o + s])
            o += s
        out.append(f(len(self.b_sizes)))
        for s in self.b_sizes:
            out += [f(s)] + list(values[o:o + s])
            o += s
        assert o == len(values)
        return np.array(out, f)

    @property
    def n_flat(self):
        return sum(self.w_sizes) + sum(self.b_sizes)


# -- the seeded inputs of tests/golden/solver_ref.npz -------------------------------------------

EDGE_GRADS = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-20, -1e-20, np.inf, -np.inf, 3e38, -3e38, 1e-40, -1e-40,
                       1.4e-45, -1.4e-45, 1.1754942e-38, 1.0, -1.0, 1e-9, 1e3], f)
CLASS_N, CLASS_STEPS, CLASS_L = 2048, 3, f(0.05)
CONT_N, CONT_STEPS, CONT_L = 256, 3, f(0.01)
NET_LRS = np.array([0.1, 0.05, 0.025], np.float64)  # a schedule that changes the rate between the steps
NET_STRIDE = 16  # the fixture holds every weight after the last step, every 16th after the others


def class_inputs():
    """(w0, d[steps][N]): magnitudes 1e-9 .. 1e3 with both signs, and in the first slots every
    pair of edge gradients over steps 1 and 2 (0, -0, 1e-30, 1e-20, +-inf, 3e38 whose square
    overflows, denormals), a third step following from whatever state they left; +-inf
    weights among the first. No NaN among the inputs."""
    r = np.random.RandomState(20240521)
    n, e = CLASS_N, len(EDGE_GRADS)
    d = (10.0 ** r.uniform(-9, 3, (CLASS_STEPS, n)) * r.choice([-1.0, 1.0], (CLASS_STEPS, n))).astype(f)
    w0 = r.normal(0, 0.5, n).astype(f)
    assert e * e <= n
    d[0, :e * e] = np.repeat(EDGE_GRADS, e)
    d[1, :e * e] = np.tile(EDGE_GRADS, e)
    d[2, :e * e] = np.roll(np.tile(EDGE_GRADS, e), 7)
    w0[3:e * e:41] = np.inf
    w0[5:e * e:43] = -np.inf
    w0[e * e:e * e + 4] = [0.0, -0.0, 3e38, -3e38]
    return w0, d


def continued_inputs():
    """(w0, g1_0, g2_0, d[steps][N]): a session continued from state that has decayed into the
    denormal range, with gradients small enough (or zero) to keep it there."""
    r = np.random.RandomState(77)
    n = CONT_N
    g1_0 = (10.0 ** r.uniform(-45, -37, n) * r.choice([-1.0, 1.0], n)).astype(f)
    g2_0 = (10.0 ** r.uniform(-45, -37, n)).astype(f)
    g1_0[::17] = 0.0
    g2_0[::19] = 0.0
    d = (10.0 ** r.uniform(-40, -18, (CONT_STEPS, n)) * r.choice([-1.0, 1.0], (CONT_STEPS, n))).astype(f)
    d[:, ::5] = 0.0
    w0 = r.normal(0, 0.5, n).astype(f)
    return w0, g1_0, g2_0, d


def continued_state(solver, g1_0, g2_0):
    """adagrad's and rmsprop's G1 is a sum of squares: they continue from |g1_0|"""
    return (g1_0 if solver == "adam" else np.abs(g1_0)), g2_0


def network_gradients(layout, codec, steps=3):
    """`steps` distinct merged gradients of `layout` (header slots in place) as (text, values):
    values = decodeFloat(text), what descentNative steps with. `codec`: encode_floats /
    decode_floats of the Base64 codec (the oracle's or the library's: they are bit-identical)."""
    r = np.random.RandomState(424242)
    out = []
    for _ in range(steps):
        raw = layout_gradient(layout, (r.normal(0, 1, layout.n_flat) * 10.0 ** r.uniform(-4, -1, layout.n_flat)).astype(f))
        text = bytes(codec.encode_floats(raw))
        out.append((text, np.asarray(codec.decode_floats(text), f)))
    return out


def layout_gradient(layout, values):
    g = GradLayout(layout.w_sizes, layout.b_sizes, getattr(layout, "fc_layers", ()))
    return g.gradient(values)
