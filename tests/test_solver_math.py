"""CPU checks of the server optimizers (adagrad, rmsprop, adam): solver_math.h's host build
against libm and a plain spelling (tests/native/check_solver.cpp sample) and against the bits
recorded from the reference's own classes (tests/golden/solver_ref.npz); the NumPy restatement
tests/solver_ref.py against both parts of that fixture; the fixture's reproducibility where the
reference is at hand; the new C-ABI entry points' names and argument errors.
`check_solver exhaustive` covers all 2^32 patterns (run during development)."""
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd.layouts import MNIST
from test_native_math import _clang

import solver_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "solver_ref.npz")
MNIST_FC = slice(72, 82)  # FC2's biases among the use_bias() layers' (C1 8, C2i 16, C2 48, FC2 10)


@pytest.fixture(scope="module")
def ref():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def check_solver(tmp_path_factory):
    clang = _clang()
    if clang is None:
        pytest.skip("no clang++ for the host build of solver_math.h")
    exe = tmp_path_factory.mktemp("native") / "check_solver"
    subprocess.check_call([clang, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread",
                           os.path.join(ROOT, "tests", "native", "check_solver.cpp"), "-o", str(exe), "-lm"])
    return str(exe)


def _sessions(z):
    """(solver, L, w0, g1_0, g2_0, d, recorded w, g1, g2) of both class-level blocks"""
    w0, d = R.class_inputs()
    cw0, cg1, cg2, cd = R.continued_inputs()
    for s in R.SOLVERS[1:]:
        zero = np.zeros_like(w0)
        g2 = z["a_adam_g2"] if s == "adam" else np.zeros_like(z[f"a_{s}_w"])
        yield s, R.CLASS_L, w0, zero, zero, d, z[f"a_{s}_w"], z[f"a_{s}_g1"], g2
        s1, s2 = R.continued_state(s, cg1, cg2)
        g2 = z["c_adam_g2"] if s == "adam" else np.zeros_like(z[f"c_{s}_w"])
        yield s, R.CONT_L, cw0, s1, (s2 if s == "adam" else np.zeros_like(s2)), cd, z[f"c_{s}_w"], z[f"c_{s}_g1"], g2


def test_host_math_against_libm_and_plain_spelling(check_solver):
    r = subprocess.run([check_solver, "sample"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout


def test_host_math_against_reference_fixture(check_solver, ref, tmp_path):
    flat = tmp_path / "solver_ref.bin"
    recs = list(_sessions(ref))
    with open(flat, "wb") as fh:
        fh.write(struct.pack("<i", len(recs)))
        for s, L, w0, g1, g2, d, ew, eg1, eg2 in recs:
            fh.write(struct.pack("<iiiif", R.SOLVERS.index(s), len(w0), len(d), 0, float(L)))
            for a in (w0, g1, g2, d):
                fh.write(np.ascontiguousarray(a, np.float32).tobytes())
            for i in range(len(d)):
                for a in (ew[i], eg1[i], eg2[i]):
                    fh.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([check_solver, "fixture", str(flat)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout


def test_restatement_equals_fixture_class_level(ref):
    seen_nan = False
    for s, L, w, g1, g2, d, ew, eg1, eg2 in _sessions(ref):
        for i in range(len(d)):
            w, g1, g2 = R.increment_w(s, w, d[i], g1, g2, L)
            assert np.array_equal(R.bits(w), R.bits(ew[i])), (s, i, "w")
            assert np.array_equal(R.bits(g1), R.bits(eg1[i])), (s, i, "g1")
            if s == "adam":
                assert np.array_equal(R.bits(g2), R.bits(eg2[i])), (s, i, "g2")
            nan = np.isnan(ew[i])
            seen_nan |= bool(nan.any())
            assert (R.bits(ew[i])[nan] == 0xFFC00000).all()  # every NaN of the contract's case 1 is x86's default
    assert seen_nan
    # the continued session really runs on denormal state
    tiny = np.abs(ref["c_adam_g2"][-1])
    assert ((tiny > 0) & (tiny < np.float32(1.1754944e-38))).sum() > 50


def test_restatement_equals_fixture_network_level(ref, oracle):
    grads = [g for _, g in R.network_gradients(MNIST, oracle)]
    for s in R.SOLVERS[1:]:
        w, b = ref["b_w0"].copy(), ref["b_b0"].copy()
        g1 = np.zeros_like(w)
        g2 = np.zeros_like(w) if s == "adam" else None
        for i, g in enumerate(grads):
            w, g1, g2, fcb = R.descent(s, MNIST, w, g1, g2, b[MNIST_FC], g, np.float32(R.NET_LRS[i]), R.SESSION)
            b[MNIST_FC] = fcb
            assert np.array_equal(R.bits(w[::R.NET_STRIDE]), R.bits(ref[f"b_{s}_w_sub"][i])), (s, i)
            assert np.array_equal(R.bits(b), R.bits(ref[f"b_{s}_b"][i])), (s, i)  # the other layers' biases never move
        assert np.array_equal(R.bits(w), R.bits(ref[f"b_{s}_w_last"])), s
    assert not np.array_equal(ref["b_adam_w_last"], ref["b_rmsprop_w_last"])


def test_fixture_is_reproducible(ref, tmp_path):
    """Where the reference and g++ are at hand: re-record and compare with the committed file."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_solver_golden as G
    if not os.path.isdir(os.path.join(G.DEFAULT_REFERENCE, "commonLib", "cppNN")) or shutil.which("g++") is None:
        pytest.skip("no reference sources or no g++ here")
    out = tmp_path / "again.npz"
    G.record(str(out))
    again = np.load(out)
    assert sorted(again.files) == sorted(ref.files)
    for k in ref.files:
        assert again[k].shape == ref[k].shape and np.array_equal(R.bits(again[k]), R.bits(ref[k])), k
    assert os.path.getsize(FIXTURE) < os.path.getsize(os.path.join(HERE, "golden", "descent_mnist.npz"))


def test_solver_names_and_argument_errors():
    L = F.lib()
    assert [L.fleet_solver_from_name(n.encode()) for n in ("sgd", "adagrad", "rmsprop", "adam")] == [0, 1, 2, 3]
    assert F.SOLVERS == ("sgd", "adagrad", "rmsprop", "adam") == R.SOLVERS
    for bad in (b"", b"Adam", b"adamw", b"sgd ", None):
        assert L.fleet_solver_from_name(bad) == -1
    assert L.fleet_model_set_solver(None, b"adam") == F.FLEET_ERR_ARG
    assert L.fleet_rmodel_set_solver(None, b"adam") == F.FLEET_ERR_ARG
    assert L.fleet_model_solver_state(None, 0, None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_rmodel_solver_state(None, 0, None, 0) == F.FLEET_ERR_ARG
    assert L.fleet_model_solver(None) == 0 and L.fleet_rmodel_solver(None) == 0
    assert L.fleet_descent_solver(None, 1, None, 0, None, None, None, 0, None, 0, None, None, 0, None, None, 0,
                                  0.0) == F.FLEET_ERR_ARG
    assert L.fleet_descent_solver_device(None, 1, None, None, None, None, None, None, None, 0, None, None, 0, 0.0,
                                         None) == F.FLEET_ERR_ARG


def test_digest_golden_names_its_functions():
    d = json.load(open(os.path.join(HERE, "golden", "solver_digests.json")))
    assert sorted(k for k in d if k.startswith("fn")) == ["fn25", "fn26", "fn27", "fn28", "fn29", "fn30"]
    assert all(len(d[f"fn{k}"]) == 16 for k in range(25, 31))
