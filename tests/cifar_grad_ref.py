"""The client's gradients on the CIFAR network, restated in plain numpy at a chosen precision
(fleet_amd/csrc/cifar_backward.h cites the reference's lines), and the
helpers that drive tests/native/check_cifar_backward.cpp. Vectorised over outputs, with loops over
channels, taps and a fully connected layer's inputs, so that a float32 run rounds after every
term as the reference does (a BLAS product would hide float32's error at these lengths); the
order inside a vectorised step is numpy's, which is what the float64 run is for."""
import os
import subprocess

import numpy as np

from fleet_amd import layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIX = 3072
TAPS = [(r, c) for r in range(3) for c in range(3)]


def model(seed, classes):
    """(w, b) float32: every layer uniform in +-sqrt(3 / fan_in), so that no layer dies"""
    rng = np.random.default_rng(seed)
    fans = [(432, 27), (9216, 144), (221184, 576), (73728, 384), (192 * classes, 192)]
    w = np.concatenate([rng.uniform(-1, 1, n) * np.sqrt(3.0 / fan) for n, fan in fans]).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, 16 + 64 + 384 + 192 + classes).astype(np.float32)
    return w, b


def images(seed, n):
    return np.random.default_rng(seed).uniform(-1, 1, (n, PIX)).astype(np.float32)


def blocks(classes):
    """[(name, start, stop)] of the value blocks of gradients(), headers left out"""
    lay = layouts.CIFAR10 if classes == 10 else layouts.CIFAR100
    names = ["dW C1", "", "dW C2", "", "dW local4", "dW local5", "dW FC2",
             "dbias I1", "", "dbias P1", "", "dbias P2", "dbias local4", "dbias local5", "dbias FC2"]
    pos = lay.header_positions()
    sizes = list(lay.w_sizes) + list(lay.b_sizes)
    starts = pos[1:1 + len(lay.w_sizes)] + pos[2 + len(lay.w_sizes):]
    return [(nm, p + 1, p + 1 + s) for nm, p, s in zip(names, starts, sizes) if s]


def gradients(dt, classes, w, b, x, labels, shifts, temperature):
    """One client: (vector [n_up] in dt, trace). x [B, 3072], labels [B], shifts [B, 2] = (dx, dy).
    trace: per sample the pools' picks and the side of every elu and relu, for the precondition."""
    dt, N = np.dtype(dt), classes
    w, b, T = np.asarray(w, dt), np.asarray(b, dt), dt.type(temperature)
    W1, W2 = w[:432].reshape(3, 16, 3, 3), w[432:9648].reshape(16, 64, 3, 3)  # [channel][map][row][col]
    W4, W5, Wf = w[9648:230832].reshape(384, 576), w[230832:304560].reshape(192, 384), w[304560:].reshape(N, 192)
    b1, b2, b4, b5 = b[:16, None, None], b[16:80, None, None], b[80:464], b[464:656]
    tenth, one = dt.type(0.1), dt.type(1)

    def elu(z):
        return np.where(z < 0, tenth * (np.exp(z) - one), z)

    def elu_df(node):
        return np.where(node > 0, one, tenth * np.exp(node))

    def conv(top, W, n):  # [chans][n+2][n+2] -> [maps][n][n], no bias
        out = np.zeros((W.shape[1], n, n), dt)
        for k in range(W.shape[0]):
            for r, c in TAPS:
                out += top[k, r:r + n, c:c + n][None] * W[k, :, r, c][:, None, None]
        return out

    def conv_back(delta, W, n):  # this layer's delta [maps][n-2][n-2] -> the top's [chans][n][n]
        pad = np.pad(delta, ((0, 0), (2, 2), (2, 2)))
        out = np.zeros((W.shape[0], n, n), dt)
        for m in range(W.shape[1]):
            for r, c in TAPS:
                out += pad[m, r:r + n, c:c + n][None] * W[:, m, 2 - r, 2 - c][:, None, None]
        return out

    def fc(W, top):  # one running sum per neuron, the inputs in order
        out = np.zeros(W.shape[0], dt)
        for i in range(W.shape[1]):
            out += W[:, i] * top[i]
        return out

    def fc_back(W, delta):  # one running sum per input, the neurons in order
        out = np.zeros(W.shape[1], dt)
        for j in range(W.shape[0]):
            out += delta[j] * W[j]
        return out

    def conv_dw(top, delta, n):  # [chans][maps][3][3]
        dW = np.zeros((top.shape[0], delta.shape[0], 3, 3), dt)
        for r, c in TAPS:
            dW[:, :, r, c] = np.einsum("kyx,myx->km", top[:, r:r + n, c:c + n], delta)
        return dW

    total, trace = None, []
    for s in range(len(labels)):
        dx, dy = int(shifts[s][0]), int(shifts[s][1])
        yy, xx = np.clip(np.arange(32) - dy, 0, 31), np.clip(np.arange(32) - dx, 0, 31)
        x0 = np.asarray(x[s], dt).reshape(3, 32, 32)[:, yy][:, :, xx]
        # forward
        z1 = conv(x0, W1, 30) + b1
        c1 = elu(z1)
        win1 = np.stack([c1[:, r:r + 27:2, c:c + 27:2] for r, c in TAPS], -1)  # [16][14][14][9], 3 wide at stride 2
        pk1 = win1.argmax(-1)  # the first maximum, as `max < n` keeps it
        p1 = np.take_along_axis(win1, pk1[..., None], -1)[..., 0]
        z2 = conv(p1, W2, 12) + b2
        c2 = elu(z2)
        quad = [(r, c) for r in range(4) for c in range(4)]
        win2 = np.stack([c2[:, r::4, c::4] for r, c in quad], -1)  # [64][3][3][16]
        pk2 = win2.argmax(-1)
        p2 = np.take_along_axis(win2, pk2[..., None], -1)[..., 0].reshape(576)
        z4 = fc(W4, p2) + b4
        h4 = np.where(z4 < 0, 0, z4).astype(dt)
        z5 = fc(W5, h4) + b5
        h5 = np.where(z5 < 0, 0, z5).astype(dt)
        zf = fc(Wf, h5)
        mx = zf[0]  # softmax::f's maximum, divided only where it is replaced (activation.h:275-278)
        for j in range(1, N):
            if zf[j] > mx:
                mx = zf[j] / T
        e = np.exp(zf / T - mx)
        target = np.zeros(N, dt)
        if 0 <= labels[s] < N:
            target[labels[s]] = 1
        # pass 1
        dfc = e / e.sum() - target
        d5 = fc_back(Wf, dfc) * (h5 > 0)
        d4 = fc_back(W5, d5) * (h4 > 0)
        dp2 = fc_back(W4, d4)
        dwin2 = np.zeros_like(win2)
        np.put_along_axis(dwin2, pk2[..., None], dp2.reshape(64, 3, 3, 1), -1)
        dc2 = np.zeros_like(c2)
        for i, (r, c) in enumerate(quad):
            dc2[:, r::4, c::4] = dwin2[..., i]
        dc2 *= elu_df(c2)
        dp1 = conv_back(dc2, W2, 14)
        dwin1 = np.zeros_like(win1)
        np.put_along_axis(dwin1, pk1[..., None], dp1[..., None], -1)
        dc1 = np.zeros_like(c1)
        fed = np.zeros(c1.shape, np.int32)  # P1 outputs that picked each C1 element
        for i, (r, c) in enumerate(TAPS):
            dc1[:, r:r + 27:2, c:c + 27:2] += dwin1[..., i]
            fed[:, r:r + 27:2, c:c + 27:2] += pk1 == i
        dc1 *= elu_df(c1)
        din = conv_back(dc1, W1, 32)
        # pass 2, in the layout's order
        head = lambda *v: np.array(v, dt)  # noqa: E731
        vec = np.concatenate([
            head(7, 432), conv_dw(x0, dc1, 30).ravel(), head(0, 9216), conv_dw(p1, dc2, 12).ravel(),
            head(0, 221184), np.outer(d4, p2).ravel(), head(73728), np.outer(d5, h4).ravel(),
            head(192 * N), np.outer(dfc, h5).ravel(),
            head(8, 3072), din.ravel(), head(0, 3136), dp1.ravel(), head(0, 576), dp2, head(384), d4, head(192), d5,
            head(N), dfc]).astype(dt)
        total = vec if total is None else total + vec
        trace.append({"pk1": pk1, "pk2": pk2, "fed": fed, "elu C1": z1 < 0, "elu C2": z2 < 0, "relu local4": z4 < 0,
                      "relu local5": z5 < 0, "df": np.concatenate([(a > 0).ravel() for a in (c1, c2, h4, h5)])})
    lay = layouts.CIFAR10 if N == 10 else layouts.CIFAR100
    total[lay.header_positions()] = lay.header_values()
    return total, trace


def build_checker(out_dir, flags=()):
    """tests/native/check_cifar_backward.cpp compiled into out_dir; None without a clang++"""
    from test_native_math import _clang
    clang = _clang()
    if clang is None:
        return None
    exe = os.path.join(str(out_dir), "check_cifar_backward" + ("_san" if flags else ""))
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "native", "check_cifar_backward.cpp"), "-o", exe])
    return exe


def mirror(exe, work_dir, jobs):
    """cifar_backward.h's host form over jobs [(classes, w, b, x [B, 3072], labels [B], shifts [B, 2] or
    None, temperature)], one client each: [(vector float32 [n_up], samples whose E is NaN)]"""
    fin, fout = os.path.join(str(work_dir), "grad_in.bin"), os.path.join(str(work_dir), "grad_out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.int32(len(jobs)).tobytes())
        for classes, w, b, x, lab, sh, temperature in jobs:
            fh.write(np.array([classes, len(lab), int(sh is not None)], np.int32).tobytes())
            fh.write(np.float32(temperature).tobytes())
            for a, t in ((w, np.float32), (b, np.float32), (x, np.float32), (lab, np.int32)):
                fh.write(np.ascontiguousarray(a, dtype=t).tobytes())
            if sh is not None:
                fh.write(np.ascontiguousarray(sh, np.int32).tobytes())
    subprocess.check_call([exe, "--mirror", fin, fout], stdout=subprocess.DEVNULL)
    raw, out, o = open(fout, "rb").read(), [], 0
    for job in jobs:
        n = (layouts.CIFAR10 if job[0] == 10 else layouts.CIFAR100).n_up
        out.append((np.frombuffer(raw, np.float32, n, o).copy(), int(np.frombuffer(raw, np.int32, 1, o + 4 * n)[0])))
        o += 4 * n + 4
    assert o == len(raw)
    return out
