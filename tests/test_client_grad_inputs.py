"""tests/golden/client_grad_ref.npz (the client's getGradients recorded from the reference): its
shape, the digest of the seeded inputs it was recorded from, and the conditions that make it
able to tell the gradient from its nearest wrong neighbours, re-asserted from the fixture."""
import os
import sys

import numpy as np
import pytest

import client_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


@pytest.fixture(scope="module")
def z():
    return R.load()


def test_inputs_are_the_recorded_ones(z):
    assert bytes(z["digest"]).decode() == R.input_digest()


def test_fixture_is_no_larger_than_the_largest_golden():
    assert os.path.getsize(R.PATH) <= os.path.getsize(os.path.join(os.path.dirname(R.PATH), "session_mnist.npz"))


def test_fixture_shape(z):
    names = [c[0] for c in R.cases()]
    assert names == ["z"] + [R.shift_name(dx, dy) for dx, dy in R.SHIFTS8] + ["blank", "badlabel", "t1", "b2", "b5"]
    for name, B, *_ in R.cases():
        assert z[f"{name}_input"].shape == (B, R.PIX) and z[f"{name}_E"].shape == (B,)
        if name.startswith("s_"):
            assert z[f"{name}_grad_c1"].shape == (200,) and z[f"{name}_grad_i1"].shape == (784,)
            assert len(bytes(z[f"{name}_grad_sha256"])) == 64
        else:
            assert z[f"{name}_grad"].shape == (R.N_UP,)
    for name in R.FULL:
        for L, n in zip(R.LAYERS, R.SIZES):
            assert z[f"{name}_node_{L}"].shape == z[f"{name}_delta_{L}"].shape == (1, n)
        assert z[f"{name}_pmap_P1"].shape == (1, 512) and z[f"{name}_pmap_P2"].shape == (1, 192)


def test_conditions_hold_from_the_fixture(z):
    import make_client_grad_golden as M
    M.conditions(z)


def test_header_values_sit_at_the_layouts_positions(z):
    from fleet_amd.layouts import MNIST
    assert MNIST.n_up == R.N_UP
    for name in ("z", "t1", "blank", "badlabel", "b2", "b5"):
        assert np.array_equal(z[f"{name}_grad"][MNIST.header_positions()], np.array(MNIST.header_values(), np.float32))


def test_recorded_inputs_are_the_shifted_images(z):
    """every recorded input layer is matrix::shift(dx, dy, mojo::edge) of its image; the cases
    whose shifts the reference drew itself show mixed shifts"""
    for name, B, teacher, mode, seed, x, lab, sh in R.cases():
        if name == "blank":
            continue
        got = R.recorded_shifts(z, name, x)
        if mode == 0:
            assert np.array_equal(got, sh), name
        else:
            assert len({tuple(s) for s in got}) > 1, name


def test_the_traps_show_in_the_fixture(z):
    """convolution dW elements are 0.f + sum (no -0 among them), FC2's are bare products"""
    g = z["z_grad"]
    conv = np.concatenate([g[2:202], g[204:332], g[333:19533]])
    assert not (R.bits(conv) == 0x80000000).any()
    assert z["badlabel_E"][0] > 0 and (z["badlabel_delta_FC2"][0] > 0).all()  # an all-zero target
