"""DPgradients and the distillation cost on the host, without a GPU: the host mirror of the
kernels (tests/native/check_client_dp.cpp over fleet_amd/csrc/client_backward.h) reproduces
every recorded array of tests/golden/client_dp_ref.npz bit for bit, plainly and under the host
sanitizers; the library's noise table is the recorded one; the new entry points are declared,
exported, refuse a NULL context; and the Python keywords left at their defaults make the call
that was made before they existed."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import client_dp_ref as R
import fleet_amd as F
from fleet_amd import client as K
from test_native_math import _clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fleet_client_ex_grads", "fleet_client_ex_grads_device", "fleet_rmodel_client_ex_grads_device",
       "fleet_client_dp_noise"]
PLATFORM = ("the draws come from std::default_random_engine and std::normal_distribution<double> of the libstdc++ "
            "this library is built with (and the log and sqrt of its glibc); the fixture was recorded with the "
            "reference built against the same: another C++ library or libm gives another, equally valid, table, "
            "and the DP fixture cases then cannot match either")


@pytest.fixture(scope="module")
def z():
    return R.load()


# ------------------------------------------------------------------ the host mirror

def _checker(tmp_path_factory, z, flags):
    clang = _clang()
    if clang is None:
        pytest.skip("no clang++ for the host build of client_backward.h")
    d = tmp_path_factory.mktemp("client_dp_native")
    R.write_flat(str(d / "client_dp_ref.bin"), z)
    exe = d / "check_client_dp"
    cmd = [clang, "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", *flags,
           os.path.join(ROOT, "tests", "native", "check_client_dp.cpp"), "-o", str(exe)]
    return cmd, [str(exe), str(d / "client_dp_ref.bin"), str(d / "vectors.out")]


def _run(run, z):
    r = subprocess.run(run, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "ALL OK" in r.stdout
    cases = R.cases()
    assert r.stdout.count("reproduce ") == len(cases)
    raw = open(run[2], "rb").read()
    draws = np.frombuffer(raw, np.float64, R.N_UP, 0)
    assert hashlib.sha256(draws.tobytes()).hexdigest() == R.sha_of(z, "z_sha256"), PLATFORM
    vec = np.frombuffer(raw, np.float32, len(cases) * R.N_UP, 8 * R.N_UP).reshape(len(cases), R.N_UP)
    for (name, *_), v in zip(cases, vec):  # every bit of every vector, through its digest
        assert R.sha(v) == R.sha_of(z, f"{name}_grad_sha256"), name
        if name in R.FULL:
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


# ------------------------------------------------------------------ the fixture itself

def test_fixture_is_of_these_inputs_and_shows_what_it_must(z):
    assert bytes(z["digest"]).decode() == R.input_digest()
    c, d = z["c_norm"], z["d_norm"]
    assert (c[1:] > R.CLIP_C).any() and (c[1:] < R.CLIP_C).any() and c[0] > R.CLIP_C
    assert (d < R.CLIP_D).all() and (z["d_scale"] == 1).all()
    assert (R.bits(z["c_sqsum"][1:]) != R.bits(z["c_sqsum_layout"][1:])).any()  # the walk's order shows
    assert (R.bits(z["c_grad_i1"]) != R.bits(z["d_grad_i1"])).any()  # clipping shows in a bias block
    assert not bool(z["c_d_dw_differ"])  # the recorded fact: no dW block is scaled
    assert os.path.getsize(R.PATH) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "session_mnist.npz"))


# ------------------------------------------------------------------ the noise table

def test_noise_table_is_the_recorded_one(z):
    t = K.dp_noise_table()
    assert t.shape == (R.N_UP,) and t.dtype == np.float64
    assert np.array_equal(t[:32].view(np.uint64), z["z_head"].view(np.uint64)), PLATFORM
    assert np.array_equal(t[-32:].view(np.uint64), z["z_tail"].view(np.uint64)), PLATFORM
    assert hashlib.sha256(t.tobytes()).hexdigest() == R.sha_of(z, "z_sha256"), PLATFORM
    assert np.array_equal(K.dp_noise_table(5), t[:5])  # the same on every call
    L = F.lib()
    assert L.fleet_client_dp_noise(None, 4) == F.FLEET_ERR_ARG
    assert L.fleet_client_dp_noise(t.ctypes.data, R.N_UP + 1) == F.FLEET_ERR_ARG
    with pytest.raises(ValueError):
        K.dp_noise_table(R.N_UP + 1)


# ------------------------------------------------------------------ the C-ABI

def test_header_declares_and_library_exports_the_new_entries():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in NEW:
        assert s in declared, s
        assert hasattr(L, s), s


def test_null_context_is_refused():
    L = F.lib()
    x = np.zeros((2, 784), np.float32)
    lab = np.zeros(2, np.int32)
    w = np.zeros(L.fleet_teacher_weight_count(), np.float32)
    b = np.zeros(L.fleet_teacher_bias_count(), np.float32)
    g = np.zeros((1, R.N_UP), np.float32)
    cs = np.ones(1, np.float32)
    for cost, clip, sigma in ((0, None, None), (1, None, None), (0, cs.ctypes.data, cs.ctypes.data)):
        assert L.fleet_client_ex_grads(None, w.ctypes.data, len(w), b.ctypes.data, len(b), x.ctypes.data, 2, 784,
                                       lab.ctypes.data, None, None, 1, 2, 2.0, cost, clip, sigma, g.ctypes.data, None,
                                       0) == F.FLEET_ERR_ARG
        assert L.fleet_client_ex_grads_device(None, 1, 21530, 1, None, 1, 2, 784, 1, None, None, 1, 2, 2.0, cost, clip,
                                              sigma, 1, R.N_UP, None, 0, None) == F.FLEET_ERR_ARG
        v = np.zeros(1, np.int32)
        assert L.fleet_rmodel_client_ex_grads_device(None, v.ctypes.data, 1, 2, 784, 1, None, None, 1, 2, 2.0, cost, clip,
                                                     sigma, 1, R.N_UP, None, 0, None) == F.FLEET_ERR_ARG


# ------------------------------------------------------------------ the Python keywords

class _Recorder:
    """stands in for the library of a Codec: records the entry point and its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class _FakeCodec:
    def __init__(self):
        self._L = _Recorder()

    def _live(self):
        return 1234

    def _check(self, rc):
        assert rc == 0


def test_default_keywords_make_the_existing_host_call():
    w, b = np.zeros(21448, np.float32), np.zeros(82, np.float32)
    x, lab = np.zeros((3, 784), np.float32), np.zeros(3, np.int32)
    plain, kw = _FakeCodec(), _FakeCodec()
    K.client_gradients(plain, w, b, x, lab, None, None, 2.0, False)
    K.client_gradients(kw, w, b, x, lab, cost="cross_entropy", clip=None, sigma=None)
    (name, args), (name_kw, args_kw) = plain._L.calls[0], kw._L.calls[0]
    assert name == name_kw == "fleet_client_grads" and len(plain._L.calls) == len(kw._L.calls) == 1
    assert len(args) == len(args_kw) == 17
    # the handle, the counts and the temperature; the pointers are those of fresh arrays
    for i in (0, 2, 4, 6, 7, 9, 10, 11, 12, 13, 15, 16):
        assert args[i] == args_kw[i], i
    assert args[11:14] == (1, 3, 2.0) and args[9] is None and args[10] is None and args[15] is None


def test_keywords_reach_the_new_host_call():
    w, b = np.zeros(21448, np.float32), np.zeros(82, np.float32)
    x, lab = np.zeros((4, 784), np.float32), np.zeros(4, np.int32)
    idx = np.array([[0, 1], [2, 3]], np.int32)
    c = _FakeCodec()
    K.client_gradients(c, w, b, x, lab, idx=idx, cost="distillation")
    K.client_gradients(c, w, b, x, lab, idx=idx, clip=2.0, sigma=[0.0, 0.5])
    (n1, a1), (n2, a2) = c._L.calls
    assert n1 == n2 == "fleet_client_ex_grads" and len(a1) == len(a2) == 20
    assert a1[14:17] == (1, None, None)
    assert a2[14] == 0 and a2[15] is not None and a2[16] is not None
    assert K.ex_args("cross_entropy", None, None, 2) is None
    cost, clip, sigma = K.ex_args("cross_entropy", 2.0, [0.0, 0.5], 2)
    assert cost == 0 and clip.tolist() == [2.0, 2.0] and sigma.tolist() == [0.0, 0.5] and clip.dtype == np.float32
    for bad in (dict(cost="mse"), dict(clip=1.0), dict(sigma=1.0), dict(clip=[1.0, 2.0, 3.0], sigma=0.5)):
        with pytest.raises(ValueError):
            K.client_gradients(c, w, b, x, lab, idx=idx, **bad)
    assert len(c._L.calls) == 2
