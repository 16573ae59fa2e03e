"""tests/golden/cifar_ref.npz (the Driver's test() on the CIFAR network, recorded from the
reference): its shape, the digest of the seeded inputs it was recorded from, the conditions that
make it able to tell the forward from its nearest wrong neighbours, and the host mirror of the
kernel (tests/native/check_cifar_forward.cpp over fleet_amd/csrc/cifar_forward.h), stand-alone,
plainly and under the host sanitizers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cifar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

EDGES = ["c_zero", "c_tie", "c_neg_bias", "c_relu_silent", "c_inf_pixels", "c_nan_weight", "c_nan_pixel", "c_labels"]


@pytest.fixture(scope="module")
def z():
    return R.load()


def test_inputs_are_the_recorded_ones(z):
    assert bytes(z["digest"]).decode() == R.input_digest()


def test_fixture_shape(z):
    for classes in (10, 100):
        c = R.case(z, f"a{classes}")
        B = R.B_MAIN[classes]
        assert c["pred"].shape == c["p"].shape == c["cost"].shape == c["error"].shape == (B,)
        assert c["accuracy"].shape == c["correct"].shape == (B,)
        assert c["probs"].shape == (R.N_PROBS, classes)
        assert c["pred"].dtype == c["correct"].dtype == np.int32
        assert R.n_w(classes) == {10: 306480, 100: 323760}[classes] and R.n_b(classes) == {10: 666, 100: 756}[classes]
    for name, shape in R.LAYERS:
        assert z[f"a10_{name}"].shape == (R.N_LAYERS,) + shape
    assert [n for n, *_ in R.edge_cases()] == EDGES
    for name, contract, w, b, x, lab in R.edge_cases():
        c = R.case(z, name)
        assert 1 <= len(lab) <= 6 and len(w) == R.n_w(10) and len(b) == R.n_b(10)
        assert c["pred"].shape == (len(lab),) and c["probs"].shape == (len(lab), 10)
    assert os.path.getsize(R.PATH) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "session_mnist.npz"))


def test_conditions_hold_from_the_fixture(z):
    import make_cifar_golden as M
    M.conditions(z)


def test_prefixes_follow_from_the_costs(z):
    """error / accuracy / correct of every prefix are the ordered binary32 sum of the recorded
    costs: ordered_error is the reference's loop, usable for index lists the fixture does not hold."""
    for classes in (10, 100):
        c = R.case(z, f"a{classes}")
        labels = R.main_case(classes)[3]
        B = R.B_MAIN[classes]
        s = np.float32(0)
        for k in range(B):
            s = np.float32(s + c["cost"][k])
            assert R.bits(np.float32(s / np.float32(k + 1))) == R.bits(c["error"][k]), (classes, k)
        correct = np.cumsum(c["pred"] == labels)
        assert np.array_equal(correct, c["correct"])
        for k in (0, 1, 2, 8, B - 1):
            assert R.bits(R.accuracy_of(correct[k], k + 1)) == R.bits(c["accuracy"][k])
            assert R.bits(R.ordered_error(c["cost"][:k + 1])) == R.bits(c["error"][k])
        assert np.array_equal(c["p"][:R.N_PROBS], c["probs"][np.arange(R.N_PROBS), c["pred"][:R.N_PROBS]])
    a = R.case(z, "a10")
    assert R.bits(R.ordered_error(a["cost"][R.PERM])) == R.bits(z["a10_perm_error"])
    assert int(z["a10_perm_correct"].reshape(-1)[0]) == int(a["correct"][-1])
    assert np.array_equal(R.bits(z["a10_fc2"]), R.bits(a["probs"][:R.N_LAYERS]))  # FC2's node is the probabilities


def test_edges_show_what_they_are_for(z):
    c = R.case(z, "c_zero")
    assert (c["pred"] == 0).all() and (R.bits(c["probs"]) == R.bits(np.float32(0.1))).all()
    c = R.case(z, "c_tie")
    top = c["probs"].max(axis=1)
    assert ((c["probs"] == top[:, None]).sum(axis=1) >= 2).all()       # the largest probability is shared
    assert (c["pred"] == (c["probs"] == top[:, None]).argmax(axis=1)).all()  # and the first wins
    assert set(c["pred"]) <= {0, 3} and 3 in set(c["pred"])
    a, c = R.case(z, "c_labels"), R.case(z, "c_neg_bias")
    assert (R.bits(a["probs"]) != R.bits(c["probs"])).any()   # the biases moved the answer
    c = R.case(z, "c_relu_silent")
    assert (R.bits(c["probs"]) == R.bits(c["probs"][0])).all()  # local5 sees its bias alone: one answer for every image
    c = R.case(z, "c_inf_pixels")
    assert np.isnan(c["p"]).any()
    assert (R.bits(c["p"][np.isnan(c["p"])]) == 0xFFC00000).all()  # no NaN among the inputs: x86's default NaN, pinned
    c = R.case(z, "c_nan_weight")
    assert np.isnan(c["p"]).all()
    c = R.case(z, "c_nan_pixel")
    assert np.isnan(c["p"]).all()  # the NaN in first place of its P1 window stays and reaches the head
    c = R.case(z, "c_labels")
    assert np.isfinite(c["cost"]).all() and c["correct"][-1] == 0


# ------------------------------------------------------------------ the host mirror

def _checker(tmp_path_factory, z, flags):
    d = tmp_path_factory.mktemp("cifar_native")
    R.write_flat(str(d / "cifar_ref.bin"), z)
    try:
        exe = R.build_checker(d, flags)
    except subprocess.CalledProcessError:
        if flags:
            pytest.skip("the compiler has no sanitizer runtime")
        raise
    if exe is None:
        pytest.skip("no clang++ for the host build of cifar_forward.h")
    return exe, d


def _run(run):
    r = subprocess.run(run, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "ALL OK" in r.stdout
    assert r.stdout.count("reproduce ") == 2 + len(EDGES)


def test_host_mirror_reproduces_every_case(tmp_path_factory, z):
    exe, d = _checker(tmp_path_factory, z, [])
    _run([exe, str(d / "cifar_ref.bin")])


def test_host_mirror_under_sanitizers(tmp_path_factory, z):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
    exe, d = _checker(tmp_path_factory, z, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _run([exe, str(d / "cifar_ref.bin")])


def test_mirror_mode_equals_the_fixture(tmp_path_factory, z):
    """--mirror, the form the GPU tests use for shapes the fixture does not hold, on a shape it holds"""
    exe, d = _checker(tmp_path_factory, z, [])
    w, b, x, lab = R.main_case(10)
    a = R.case(z, "a10")
    idx = np.array([5, 5, 0, 11, 3], np.int32)
    plain, picked = R.mirror(exe, d, [(10, w, b, x[:12], lab[:12], None), (10, w, b, x[:12], lab[:12], idx)])
    for k, want in (("pred", a["pred"][:12]), ("p", a["p"][:12]), ("cost", a["cost"][:12]), ("error", a["error"][11]),
                    ("accuracy", a["accuracy"][11]), ("probs", a["probs"])):
        got = plain[k][:R.N_PROBS] if k == "probs" else plain[k]
        assert not R.mismatch(1, np.atleast_1d(got), np.atleast_1d(want)), k
    assert plain["correct"] == a["correct"][11]
    assert np.array_equal(picked["pred"], a["pred"][idx]) and not R.mismatch(1, picked["cost"], a["cost"][idx])
    assert R.bits(picked["error"]) == R.bits(R.ordered_error(a["cost"][idx]))
