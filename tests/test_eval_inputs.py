"""tests/golden/eval_ref.npz (the Driver's test() recorded from the reference): its shape, the
digest of the seeded inputs it was recorded from, the three conditions that make it able to
tell the evaluation from its nearest wrong neighbours, and the host mirror of the kernels
(tests/native/check_eval_forward.cpp over fleet_amd/csrc/eval_forward.h), stand-alone,
plainly and under the host sanitizers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_ref as R
from test_native_math import _clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

MAIN = ("a", "b_text", "b_copy", "b_bcast")


@pytest.fixture(scope="module")
def z():
    return R.load()


def test_inputs_are_the_recorded_ones(z):
    assert bytes(z["digest"]).decode() == R.input_digest()


def test_fixture_shape(z):
    for name in MAIN:
        c = R.case(z, name)
        assert c["pred"].shape == c["p"].shape == c["cost"].shape == c["error"].shape == (R.B_A,)
        assert c["accuracy"].shape == c["correct"].shape == (R.B_A,)
        assert c["probs"].shape == (R.N_PROBS, 10)
        assert c["pred"].dtype == c["correct"].dtype == np.int32
    for name in MAIN[1:]:
        assert z[f"{name}_w"].shape == (R.N_W,) and z[f"{name}_b"].shape == (R.N_B,)
    w_read = np.load(R.SEEDED_MODEL)["w_read"]
    assert np.array_equal(R.bits(z["b_text_w"]), R.bits(w_read))
    assert (R.bits(z["b_bcast_w"]) != R.bits(z["b_copy_w"])).any()  # the Driver's view is not the stored version
    names = [n for n, *_ in R.edge_cases()]
    assert names == ["c_zero", "c_tie", "c_denom_zero", "c_mixed_sign", "c_inf_pixels", "c_nan_weight", "c_labels"]
    for name, contract, w, b, x, lab in R.edge_cases():
        c = R.case(z, name)
        assert c["pred"].shape == (len(lab),) and c["probs"].shape == (len(lab), 10)


def test_conditions_hold_from_the_fixture(z, oracle):
    """The issue's three conditions, from the recorded numbers and the existing train-mode oracle."""
    import make_eval_golden as M
    w, b = R.model_a()
    M.conditions(z, oracle.teacher_forward(w, b, R.images_a(), temperature=1.0))


def test_prefixes_follow_from_the_costs(z):
    """error / accuracy / correct of every prefix are the ordered binary32 sum of the recorded
    costs: ordered_error is the reference's loop, usable for index lists the fixture does not hold."""
    labels = R.labels_a()
    for name in MAIN:
        c = R.case(z, name)
        s = np.float32(0)
        for k in range(R.B_A):
            s = np.float32(s + c["cost"][k])
            assert R.bits(np.float32(s / np.float32(k + 1))) == R.bits(c["error"][k]), (name, k)
        correct = np.cumsum(c["pred"] == labels)
        assert np.array_equal(correct, c["correct"])
        for k in (0, 1, 2, 8, R.B_A - 1):
            assert R.bits(R.accuracy_of(correct[k], k + 1)) == R.bits(c["accuracy"][k])
            assert R.bits(R.ordered_error(c["cost"][:k + 1])) == R.bits(c["error"][k])
    a = R.case(z, "a")
    assert R.bits(R.ordered_error(a["cost"][R.PERM])) == R.bits(z["a_perm_error"])
    assert int(z["a_perm_correct"].reshape(-1)[0]) == int(a["correct"][-1])
    assert np.array_equal(a["p"][:R.N_PROBS], a["probs"][np.arange(R.N_PROBS), a["pred"][:R.N_PROBS]])


def test_edges_show_what_they_are_for(z):
    c = R.case(z, "c_zero")
    assert (c["pred"] == 0).all() and (R.bits(c["probs"]) == R.bits(np.float32(0.1))).all()
    c = R.case(z, "c_tie")
    top = c["probs"].max(axis=1)
    assert ((c["probs"] == top[:, None]).sum(axis=1) >= 2).all()       # the largest probability is shared
    assert (c["pred"] == (c["probs"] == top[:, None]).argmax(axis=1)).all()  # and the first wins
    assert set(c["pred"]) == {0, 3}
    c = R.case(z, "c_inf_pixels")
    assert np.isnan(c["p"][:3]).all() and (c["pred"][:3] == 0).all() and not np.isnan(c["p"][3:]).any()
    assert (R.bits(c["p"][:3]) == 0xFFC00000).all()  # no NaN among the inputs: x86's default NaN, pinned
    c = R.case(z, "c_nan_weight")
    assert np.isnan(c["p"]).all()
    c = R.case(z, "c_labels")
    assert np.isfinite(c["cost"]).all() and c["correct"][-1] == 0


# ------------------------------------------------------------------ the host mirror

def _checker(tmp_path_factory, z, flags):
    clang = _clang()
    if clang is None:
        pytest.skip("no clang++ for the host build of eval_forward.h")
    d = tmp_path_factory.mktemp("eval_native")
    R.write_flat(str(d / "eval_ref.bin"), z)
    exe = d / "check_eval_forward"
    cmd = [clang, "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", *flags,
           os.path.join(ROOT, "tests", "native", "check_eval_forward.cpp"), "-o", str(exe)]
    return cmd, [str(exe), str(d / "eval_ref.bin")]


def _run(run):
    r = subprocess.run(run, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "ALL OK" in r.stdout
    assert r.stdout.count("reproduce ") == 4 + len(R.edge_cases())


def test_host_mirror_reproduces_every_case(tmp_path_factory, z):
    cmd, run = _checker(tmp_path_factory, z, [])
    subprocess.check_call(cmd)
    _run(run)


def test_host_mirror_under_sanitizers(tmp_path_factory, z):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
    cmd, run = _checker(tmp_path_factory, z, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitizer" in r.stderr.lower()):
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-4000:]
    _run(run)
