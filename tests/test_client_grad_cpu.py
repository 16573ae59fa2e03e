"""The client gradient's host side without a GPU: the host mirror of the kernels
(tests/native/check_client_grad.cpp over fleet_amd/csrc/client_backward.h) reproduces every
recorded array of tests/golden/client_grad_ref.npz bit for bit, plainly and under the host
sanitizers; the C-ABI declares and exports its entry points, refuses impossible arguments
before anything is launched, and the host-only pieces (the length, the chunk override, the
rand() draw of the shifts) answer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import client_grad_ref as R
import fleet_amd as F
from fleet_amd import client as K
from fleet_amd.layouts import MNIST
from test_native_math import _clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIENT = ["fleet_client_grad_len", "fleet_client_grad_set_chunk", "fleet_client_grads", "fleet_client_grads_device",
          "fleet_rmodel_client_grads_device"]


@pytest.fixture(scope="module")
def z():
    return R.load()


# ------------------------------------------------------------------ the host mirror

def _checker(tmp_path_factory, z, flags):
    clang = _clang()
    if clang is None:
        pytest.skip("no clang++ for the host build of client_backward.h")
    d = tmp_path_factory.mktemp("client_grad_native")
    R.write_flat(str(d / "client_grad_ref.bin"), z)
    exe = d / "check_client_grad"
    cmd = [clang, "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", *flags,
           os.path.join(ROOT, "tests", "native", "check_client_grad.cpp"), "-o", str(exe)]
    return cmd, [str(exe), str(d / "client_grad_ref.bin"), str(d / "vectors.out")]


def _run(run, z):
    r = subprocess.run(run, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "ALL OK" in r.stdout
    cases = R.cases()
    assert r.stdout.count("reproduce ") == len(cases)
    vec = np.fromfile(run[2], np.float32).reshape(len(cases), R.N_UP)
    for (name, *_), v in zip(cases, vec):  # the whole vector of the cases that hold a digest of it
        if name.startswith("s_"):
            assert R.sha(v) == bytes(z[f"{name}_grad_sha256"]).decode(), name
        else:
            assert np.array_equal(R.bits(v), R.bits(z[f"{name}_grad"])), name


def test_host_mirror_reproduces_every_case(tmp_path_factory, z):
    cmd, run = _checker(tmp_path_factory, z, [])
    subprocess.check_call(cmd)
    _run(run, z)


def test_host_mirror_under_sanitizers(tmp_path_factory, z):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
    cmd, run = _checker(tmp_path_factory, z, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitizer" in r.stderr.lower()):
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-4000:]
    _run(run, z)


# ------------------------------------------------------------------ the C-ABI

def test_header_declares_and_library_exports_the_client_call():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in CLIENT:
        assert s in declared, s
        assert hasattr(L, s), s
    assert sorted(s for s in declared if "client_grad" in s) == sorted(CLIENT)


def test_length_is_the_layouts(z):
    assert F.lib().fleet_client_grad_len() == MNIST.n_up == K.client_grad_len() == R.N_UP
    assert np.array_equal(z["z_grad"][MNIST.header_positions()], np.array(MNIST.header_values(), np.float32))


def test_chunk_override_is_restored():
    L = F.lib()
    assert L.fleet_client_grad_set_chunk(0) == 0
    with K.client_chunk_override(3):
        assert L.fleet_client_grad_set_chunk(3) == 3
        with K.client_chunk_override(1):
            assert L.fleet_client_grad_set_chunk(1) == 1
        assert L.fleet_client_grad_set_chunk(3) == 3
    assert L.fleet_client_grad_set_chunk(0) == 0
    assert L.fleet_client_grad_set_chunk(-5) == 0  # a negative chunk is the default
    assert L.fleet_client_grad_set_chunk(0) == 0


def test_refusals_come_before_any_launch():
    """Every refusal of the host form and of the device forms answers without a context that
    could launch: a NULL context, or (for what is checked after the context) none needed."""
    L = F.lib()
    x = np.zeros((2, 784), np.float32)
    lab = np.zeros(2, np.int32)
    w = np.zeros(L.fleet_teacher_weight_count(), np.float32)
    b = np.zeros(L.fleet_teacher_bias_count(), np.float32)
    g = np.zeros((1, R.N_UP), np.float32)
    assert L.fleet_client_grads(None, w.ctypes.data, len(w), b.ctypes.data, len(b), x.ctypes.data, 2, 784,
                                lab.ctypes.data, None, None, 1, 2, 2.0, g.ctypes.data, None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_client_grads_device(None, 1, 21530, 1, None, 1, 2, 784, 1, None, None, 1, 2, 2.0, 1, R.N_UP, None, 0,
                                       None) == F.FLEET_ERR_ARG
    v = np.zeros(1, np.int32)
    assert L.fleet_rmodel_client_grads_device(None, v.ctypes.data, 1, 2, 784, 1, None, None, 1, 2, 2.0, 1, R.N_UP, None,
                                              0, None) == F.FLEET_ERR_ARG


def test_python_refuses_mismatched_inputs():
    with pytest.raises(ValueError):
        K.host_args(np.zeros((3, 784), np.float32), np.zeros(2, np.int32), None, None)
    with pytest.raises(ValueError):
        K.host_args(np.zeros((3, 784), np.float32), np.zeros(3, np.int32), np.zeros((2, 2), np.int32),
                         np.zeros((2, 3, 2), np.int32))
    x, lab, ix, sh, Cn, B = K.host_args(np.zeros((5, 784)), [1, 2, 3, 4, 5], None, None)
    assert (Cn, B) == (1, 5) and ix is None and sh is None and lab.dtype == np.int32
    x, lab, ix, sh, Cn, B = K.host_args(np.zeros((5, 784)), [1, 2, 3, 4, 5], [[0, 1], [4, 4], [2, 2]], None)
    assert (Cn, B) == (3, 2)


def test_client_shifts_against_the_recorded_shifts(z):
    """the rand() draw of the shifts, in the order the reference's g++ build evaluated the two
    arguments: the shifted input layers the recorder stored tell"""
    for name, B, teacher, mode, seed, x, lab, sh in R.cases():
        if mode == 1:
            assert np.array_equal(K.client_shifts(seed, 1, B)[0], R.recorded_shifts(z, name, x)), name
    draws = iter([0, 1, 2, 2, 1, 0, 0, 0])
    got = K.client_shifts(lambda: next(draws), 2, 2)
    assert got.tolist() == [[[0, -1], [1, 1]], [[-1, 0], [-1, -1]]]  # dy is drawn first
