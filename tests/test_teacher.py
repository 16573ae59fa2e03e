"""The sampler's mode-1 teacher forward: uniformSample's
teacher.forward(sample, TEMPERATURE, -1, 1) (Server/src/main/c++/cppNN_backend.cpp:
596-613) of initSampler's network (:494-502).

Pins, strongest first:
* tests/golden/teacher_mnist.npz holds the class probabilities of the
  reference's OWN mojo network (commonLib/cppNN compiled by oracle/Makefile into
  oracle/_ref, tests/golden/make_golden.py teacher) for seeded weights and inputs;
* the oracle's C restatement (oracle/fleet_oracle.c fo_teacher_forward, libm
  expf) equals that fixture bit for bit, and equals the reference build on fresh
  inputs where oracle/_ref exists (this container);
* the device's expf (teacher_math.h glibc_expf, a restatement of glibc 2.35's)
  equals libm's expf on all 2^32 inputs (digest fn 18, tests/golden/digests.json,
  itself checked against this machine's libm here);
* the device forward equals the fixture bit for bit (NaN rows included: the
  reference's softmax overflows at the largest weight scale);
* tests/golden/teacher_edges.npz (make_golden.py teacher_edges, layout in
  tests/teacher_edges.py) holds the reference network's answers at the forward's
  data-dependent branches and at non-finite and subnormal values;
  tests/test_teacher_census.py proves on the CPU which branches it reaches and that
  it tells mutated arithmetic from the original. Contract:
  1. no NaN among weights, biases and pixels (+-inf allowed): oracle and device
     equal the reference bit for bit, NaN outputs (0xFFC00000) included;
  2. NaN among them: NaN at the same positions, every other value bitwise equal,
     the mini-batch text byte-equal (the codec has one code for every NaN); the
     NaN bit patterns are not pinned -- the reference's depend on its compiler's
     operand order per instruction.
"""
import json
import os

import numpy as np
import pytest

import teacher_edges as TE

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "teacher_mnist.npz")
REF_SO = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libfleetref_model.so")


def _cases():
    z = np.load(GOLDEN)
    n = len([k for k in z.files if k.startswith("probs")])
    return [(z[f"w{i}"], z[f"b{i}"], z[f"x{i}"], z[f"probs{i}"]) for i in range(n)]


_EDGES = []


def _edges():
    """{name: (contract, w, b, x, probs)} of teacher_edges.npz, expanded once and left unchanged."""
    if not _EDGES:
        _EDGES.append({name: rest for name, *rest in TE.load()})
    return _EDGES[0]


EDGE_NAMES = [str(n) for n in np.load(TE.PATH)["names"]]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_fixture_shape_and_coverage():
    cases = _cases()
    assert len(cases) == 3
    for w, b, x, p in cases:
        assert w.shape == (21448,) and b.shape == (82,) and x.shape[1] == 784 and p.shape == (x.shape[0], 10)
    # typical scales give proper distributions; the largest overflows the softmax as the reference does
    for _, _, _, p in cases[:2]:
        assert np.all(np.isfinite(p)) and np.allclose(p.sum(1), 1.0, atol=1e-5)
    assert np.any(~np.isfinite(cases[2][3]))


def test_oracle_teacher_matches_reference_fixture(oracle):
    for w, b, x, p in _cases():
        assert np.array_equal(_bits(oracle.teacher_forward(w, b, x)), _bits(p))


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref (reference build) absent")
def test_oracle_teacher_matches_reference_build(oracle):
    import pyoracle
    ref = pyoracle.ReferenceModel()
    rng = np.random.default_rng(77)
    for scale in (0.02, 0.1, 0.4):
        w = (rng.standard_normal(21448) * scale).astype(np.float32)
        b = (rng.standard_normal(82) * 0.2).astype(np.float32)
        x = np.where(rng.random((16, 784)) < 0.6, 0.0, rng.random((16, 784))).astype(np.float32)
        assert np.array_equal(_bits(oracle.teacher_forward(w, b, x)), _bits(ref.teacher_forward(w, b, x)))


def test_edge_fixture_is_small_data_with_the_stated_contracts():
    assert os.path.getsize(TE.PATH) <= os.path.getsize(GOLDEN)
    z = np.load(TE.PATH)  # allow_pickle stays False: arrays only
    assert all(z[k].dtype.kind in "fiuU" for k in z.files)
    edges = _edges()
    assert list(edges) == EDGE_NAMES and len(set(EDGE_NAMES)) == len(EDGE_NAMES)
    for name, (contract, w, b, x, p) in edges.items():
        assert w.shape == (21448,) and b.shape == (82,) and x.shape[1] == 784 and p.shape == (x.shape[0], 10), name
        assert 1 <= x.shape[0] <= 8, name
        has_nan = bool(np.isnan(w).any() or np.isnan(b).any() or np.isnan(x).any())
        assert contract == (2 if has_nan else 1), name
        if contract == 1:  # the reference's NaN without NaN inputs is x86's default NaN
            assert set(_bits(p)[np.isnan(p)].tolist()) <= {0xFFC00000}, name
    # what the GPU tests below rely on: NaN, exact 0 and 1 and the smallest subnormal among the answers
    allp = np.concatenate([v[4].reshape(-1) for v in edges.values()])
    assert np.isnan(allp).any() and (allp == 0).any() and (allp == 1).any() and (_bits(allp) == 1).any()
    # finite answers although an inf / a NaN entered a pooling window (at a slot the scan drops)
    for name in ("inf_pixel_corner", "nan_pixel_corner"):
        assert np.isfinite(edges[name][4]).all() and not np.isfinite(edges[name][3]).all()


def test_oracle_teacher_matches_edge_fixture(oracle):
    for name, (contract, w, b, x, p) in _edges().items():
        assert TE.mismatch(contract, oracle.teacher_forward(w, b, x), p) == "", name


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref (reference build) absent")
def test_edge_fixture_and_oracle_match_reference_build(oracle):
    import pyoracle
    ref = pyoracle.ReferenceModel()
    for name, (contract, w, b, x, p) in _edges().items():
        r = ref.teacher_forward(w, b, x)
        assert np.array_equal(_bits(r), _bits(p)), name  # the recording is this build's answer, NaN bits included
        assert TE.mismatch(contract, oracle.teacher_forward(w, b, x), r) == "", name


def test_libm_expf_digest_matches_golden(oracle):
    """digests.json fn 18 is this libm's expf (the reference's std::exp(float))."""
    ref = json.load(open(os.path.join(HERE, "golden", "digests.json")))
    assert f"{oracle.expf_digest():016x}" == ref["fn18"]


def test_teacher_symbols_and_sizes():
    import fleet_amd as F
    L = F.lib()
    assert L.fleet_teacher_weight_count() == 21448
    assert L.fleet_teacher_bias_count() == 82


@pytest.mark.gpu
def test_device_teacher_matches_reference_fixture(codec):
    for w, b, x, p in _cases():
        assert np.array_equal(_bits(codec.teacher_forward(w, b, x)), _bits(p))


@pytest.mark.gpu
def test_device_teacher_indices_device_path_and_errors(codec, oracle):
    import fleet_amd as F
    torch = pytest.importorskip("torch")
    w, b, x, p = _cases()[1]
    rng = np.random.default_rng(3)
    feats = np.concatenate([x, rng.random((x.shape[0], 1)).astype(np.float32)], axis=1)  # F = 785 rows
    idx = rng.integers(0, x.shape[0], 40).astype(np.int32)
    assert np.array_equal(_bits(codec.teacher_forward(w, b, feats, idx)), _bits(p[idx]))
    dev = torch.device("cuda", 0)
    probs = torch.zeros((len(idx), 10), dtype=torch.float32, device=dev)
    codec.teacher_forward_device(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev),
                                 torch.from_numpy(feats).to(dev), probs, torch.from_numpy(idx).to(dev))
    codec.check()
    assert np.array_equal(_bits(probs.cpu().numpy()), _bits(p[idx]))
    with pytest.raises(F.FleetError):
        codec.teacher_forward(w, b, feats, np.array([0, x.shape[0]], np.int32))
    with pytest.raises(F.FleetError):
        codec.teacher_forward(w[:-1], b, feats)
    bad = torch.tensor([1, x.shape[0] + 3], dtype=torch.int32, device=dev)
    codec.teacher_forward_device(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev),
                                 torch.from_numpy(feats).to(dev), probs, bad)
    with pytest.raises(F.FleetError):
        codec.check()


@pytest.mark.gpu
def test_sampler_minibatch_with_device_teacher(codec, oracle):
    """uniformSample + getMiniBatch in mode 1 end to end: the request text equals the
    oracle's composition with the reference's teacher probabilities."""
    import pyoracle
    from fleet_amd import sampler as S
    w, b, x, p = _cases()[0]
    labels = (np.arange(x.shape[0]) % 10).astype(np.int32)
    s = S.OfflineSampler(codec, x, labels, E=1, sigma=0.0, C=0.0, num_labels=10, lr=0.01, iid=True)
    teacher = S.Teacher(codec, w, b, x)
    S.srand(5)
    text = s.getMiniBatch(12, teacher=teacher)
    S.srand(5)
    idx = S.uniform_indices(x.shape[0], 12)
    hdr = S.minibatch_header(1, 0.0, 0.0, 0.01, 12, 784, 10)
    assert text == oracle.encode_floats(pyoracle.minibatch_vector(x, labels, idx, hdr, p[idx]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_device_teacher_edge_case(codec, name):
    contract, w, b, x, p = _edges()[name]
    assert TE.mismatch(contract, codec.teacher_forward(w, b, x), p) == ""


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["inf_c2", "zero_bias"])
def test_device_teacher_edges_indices_and_device_path(codec, name):
    """A contract-1 case with NaN answers (a NaN born in C2's sum) and the zero-bias case
    through idx with repeats, the device-resident form with F = 785, B = 1, and B = 300
    from 8 resident rows (more blocks than CUs)."""
    torch = pytest.importorskip("torch")
    contract, w, b, x, p = _edges()[name]
    assert contract == 1 and x.shape[0] == 8
    rng = np.random.default_rng(11)
    feats = np.concatenate([x, rng.random((8, 1)).astype(np.float32)], axis=1)
    idx = np.array([7, 7, 0, 3, 3, 3, 0, 5], np.int32)
    assert np.array_equal(_bits(codec.teacher_forward(w, b, feats, idx)), _bits(p[idx]))
    for i in (0, 6):
        assert np.array_equal(_bits(codec.teacher_forward(w, b, x[i:i + 1])), _bits(p[i:i + 1]))
        assert np.array_equal(_bits(codec.teacher_forward(w, b, x, np.array([i], np.int32))), _bits(p[i:i + 1]))
    dev = torch.device("cuda", 0)
    dw, db, df = (torch.from_numpy(a).to(dev) for a in (w, b, feats))
    for ix in (idx, np.array([4], np.int32), rng.integers(0, 8, 300).astype(np.int32)):
        probs = torch.zeros((len(ix), 10), dtype=torch.float32, device=dev)
        codec.teacher_forward_device(dw, db, df, probs, torch.from_numpy(ix).to(dev))
        codec.check()
        assert np.array_equal(_bits(probs.cpu().numpy()), _bits(p[ix]))


@pytest.mark.gpu
def test_sampler_minibatch_over_edge_cases(codec, oracle):
    """S.Teacher + getMiniBatch over every edge case's samples -- probabilities that are NaN,
    exactly 0, exactly 1 and 2^-149 among them: the request text is the oracle's encoding of
    the vector built with the reference's probabilities (for contract-2 cases that is the
    whole requirement: every NaN has the same code)."""
    import pyoracle
    from fleet_amd import sampler as S
    nan_codes = {oracle.encode_floats(TE.from_bits(np.array([u], np.uint32)))
                 for u in (0x7FC00000, 0xFFC00000, 0x7FC00123, 0xFFC00456)}
    assert len(nan_codes) == 1
    for name, (contract, w, b, x, p) in _edges().items():
        labels = (np.arange(x.shape[0]) % 10).astype(np.int32)
        s = S.OfflineSampler(codec, x, labels, E=1, sigma=0.0, C=0.0, num_labels=10, lr=0.01, iid=True)
        S.srand(9)
        text = s.getMiniBatch(8, teacher=S.Teacher(codec, w, b, x))
        S.srand(9)
        idx = S.uniform_indices(x.shape[0], 8)
        hdr = S.minibatch_header(1, 0.0, 0.0, 0.01, 8, 784, 10)
        assert text == oracle.encode_floats(pyoracle.minibatch_vector(x, labels, idx, hdr, p[idx])), name
