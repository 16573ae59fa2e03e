"""The inputs of tests/test_gpu_model_topologies.py, proven on the CPU: tests/golden/session_fc3.npz
(the reference's own network on tests/model_nets.py's fc3, make_golden.py session_nets) holds
what the GPU tests assume of it. Sizes, the biases that move and those that do not, the
gradients' headers, the generator, and the chain condition of the `chain` session.

The chain condition. A recorded version holds the dictionary's entries, not the values that
were merged into them, so `oracle.dictionary` of a recorded version can show U < n_w but never
two bit-different values in one entry (an entry is further than 1e-8 from every earlier one).
The values that were merged are cnn's: they are restated here from the stored init text and
gradients (oracle.descent, pinned to the reference by descent_mnist.npz), their dictionary
must have U < n_w with entries shared by bit-different values, and the version it yields must
be the recorded one, bit for bit: so the reference's own copy met those chains."""
import os

import numpy as np
import pytest

import model_nets as N

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", N.GOLDEN["fc3"])
NET = N.FC3
f32 = np.float32
_rt = N.roundtrip


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def z():
    return np.load(PATH)


def _split(params):
    """getModelParams: the use_bias() biases once per graph edge, then the weights"""
    nb, e = NET.n_b, NET.edges
    reps = params[:nb * e].reshape(e, nb)
    assert (_bits(reps) == _bits(reps[0])).all()
    return params[nb * e:], reps[0]


def test_the_fixture_is_small():
    # 2 sessions x 4 states x 2 versions x 1195 floats do not compress: 76 KB; the texts add the rest
    assert os.path.getsize(PATH) < 160 * 1024


@pytest.mark.parametrize("ses", N.SESSIONS["fc3"])
def test_sizes_and_counts(z, ses):
    assert NET.n_b * NET.edges + NET.n_w == 1195
    for s in range(N.STEPS + 1):
        for key in ("newest", "oldest"):
            assert len(z[f"{ses}_{key}_params{s}"]) == NET.n_b * 5 + NET.n_w
    assert int(z[f"{ses}_n_models"]) == 2 and int(z[f"{ses}_stale"]) == 2 and int(z[f"{ses}_batch"]) == 8
    assert len(set(z[f"{ses}_lrates"].tolist())) == 3


@pytest.mark.parametrize("ses", N.SESSIONS["fc3"])
def test_fc_biases_move_and_conv_biases_stay(z, ses):
    assert [(s.start, s.stop) for s in NET.fc_slices()] == [(4, 13), (13, 20), (20, 25)]
    for s in range(N.STEPS):
        b0, b1 = _split(z[f"{ses}_newest_params{s}"])[1], _split(z[f"{ses}_newest_params{s + 1}"])[1]
        moved = _bits(b0) != _bits(b1)
        for sl in NET.fc_slices():
            assert moved[sl].any(), (ses, s, sl)
        assert not moved[~NET.fc_mask()].any()
        # after the first step the oldest version is the one that was the newest
        if s:
            assert np.array_equal(_bits(z[f"{ses}_oldest_params{s + 1}"]), _bits(z[f"{ses}_newest_params{s}"]))


@pytest.mark.parametrize("ses", N.SESSIONS["fc3"])
def test_gradients_carry_the_layouts_header(z, oracle, ses):
    lay = NET.layout
    for i in range(N.STEPS):
        g = oracle.decode_floats(bytes(z[f"{ses}_merged{i}"]))
        assert len(g) == lay.n_up == 1492
        assert g[lay.header_positions()].tolist() == lay.header_values()


@pytest.mark.parametrize("ses", N.SESSIONS["fc3"])
def test_the_generator_is_pinned(z, oracle, ses):
    w, b, merged = N.session_inputs(NET, ses, oracle)
    assert NET.text(1, w, b, oracle) == bytes(z[f"{ses}_init"])
    for i, m in enumerate(merged):
        assert m == bytes(z[f"{ses}_merged{i}"])
    assert tuple(z[f"{ses}_lrates"].tolist()) == N.LRATES


def _shared(w, idx, U):
    """dictionary entries that hold two bit-different values"""
    return sum(len(set(_bits(w[idx == u]).tolist())) > 1 for u in range(U))


@pytest.mark.parametrize("ses", N.SESSIONS["fc3"])
def test_restated_cnn_gives_the_recorded_versions_and_meets_chains(z, oracle, ses):
    lay = NET.layout
    w0, b0, _ = N.session_inputs(NET, ses, oracle)
    dims = list(NET.dims)
    w = oracle.read_weights_section(oracle.weights_section(oracle.quantize(w0, dims), dims), dims)
    b = _rt(b0)
    fc = NET.fc_mask()
    for s in range(N.STEPS + 1):
        if s:
            g = oracle.decode_floats(bytes(z[f"{ses}_merged{s - 1}"]))
            w, b[fc] = oracle.descent(w, b[fc], g, lay.w_present(), lay.fc_flags(), f32(N.LRATES[s - 1]))
        d, idx = oracle.dictionary(w)
        rw, rb = _split(z[f"{ses}_newest_params{s}"])
        assert np.array_equal(_bits(_rt(d)[idx]), _bits(rw)), (ses, s)
        assert np.array_equal(_bits(_rt(b)), _bits(rb)), (ses, s)
        if ses == "chain":
            assert np.abs(w).max() < 1e-6
            assert len(oracle.dictionary(rw)[0]) < NET.n_w       # of the recorded version itself
            if s:
                assert len(d) < NET.n_w and _shared(w, idx, len(d)) >= 1, (s, len(d))
