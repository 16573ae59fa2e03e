"""The client's gradients on the CIFAR network without a GPU: the host mirror of the kernels
(fleet_amd/csrc/cifar_backward.h through tests/native/check_cifar_backward.cpp, built plainly and
under the host sanitizers) against the float64 restatement of tests/cifar_grad_ref.py, the C-ABI's
surface, and its refusals before any launch."""

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd import cifar_client as K

import cifar_grad_ref as G

RGBNET = ["fleet_rgbnet_grad_len", "fleet_rgbnet_grads", "fleet_rgbnet_grads_device", "fleet_rgbnet_sample_tile",
          "fleet_rgbnet_set_chunk", "fleet_rmodel_rgbnet_grads_device"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# (classes, B, temperature, seed): every shift but (0, 0) within a case, one label outside [0, classes)
JOBS = [(10, 3, 2.0, 1), (100, 2, 1.0, 2)]


def _job(classes, B, temperature, seed):
    w, b = G.model(seed, classes)
    lab = np.array([3, classes + 5, 0][:B], np.int32)
    sh = np.array([(-1, 1), (1, 0), (0, -1)][:B], np.int32)
    return classes, w, b, G.images(seed + 100, B), lab, sh, temperature


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "sanitized"])
def test_mirror_against_the_float64_restatement(tmp_path, flags):
    """Per block of the layout the mirror lies within 4 * d_block of the float64 values, d_block =
    max |restatement(float32) - restatement(float64)| on the same inputs: the factor covers numpy's
    float32 exp and its order inside a vectorised step. First the precondition, on the restatement
    alone: both precisions agree on every pool pick and on the side of every elu and relu (else the
    gradient is discontinuous between them), and the inputs reach the paths named below."""
    exe = G.build_checker(tmp_path, flags)
    assert exe is not None, "no clang++ for the host mirror"
    jobs = [_job(*j) for j in JOBS]
    ref = [(G.gradients(np.float32, *j), G.gradients(np.float64, *j)) for j in jobs]
    for (_, t32), (_, t64) in ref:
        assert sum(int((a[k] != c[k]).sum()) for a, c in zip(t32, t64) for k in a) == 0
        assert max(int(t["fed"].max()) for t in t64) >= 2                     # a C1 element fed by several P1 outputs
        assert any((t["pk1"] != 0).any() and (t["pk2"] != 0).any() for t in t64)  # a maximum not in first place
        for k in ("elu C1", "elu C2", "relu local4", "relu local5"):          # both sides of every activation
            assert all(t[k].any() and not t[k].all() for t in t64), k
    for job, ((r32, _), (r64, _)), (got, blown) in zip(jobs, ref, G.mirror(exe, tmp_path, jobs)):
        assert blown == 0
        lay = F.layouts.CIFAR10 if job[0] == 10 else F.layouts.CIFAR100
        assert np.array_equal(got[lay.header_positions()], np.array(lay.header_values(), np.float32))
        for name, lo, hi in G.blocks(job[0]):
            d_block = np.abs(r32[lo:hi].astype(np.float64) - r64[lo:hi]).max()
            err = np.abs(got[lo:hi].astype(np.float64) - r64[lo:hi]).max()
            print(f"classes {job[0]} {name}: d_block {d_block:.3e}, mirror {err:.3e}")
            assert err <= 4 * d_block, (job[0], name, err, d_block)


def test_header_declares_and_library_exports_the_entry_points():
    declared = F.exported_symbols_from_header()
    assert sorted(s for s in declared if "rgbnet" in s) == RGBNET
    for s in RGBNET:
        assert hasattr(F.lib(), s), s
    assert (K.grad_len(10), K.grad_len(100), K.grad_len(7)) == (F.layouts.CIFAR10.n_up, F.layouts.CIFAR100.n_up, 0)
    assert K.sample_tile() >= 2
    with K.chunk_override(3):
        assert F.lib().fleet_rgbnet_set_chunk(3) == 3
    assert F.lib().fleet_rgbnet_set_chunk(0) == 0


@pytest.mark.parametrize("kw", [dict(classes=7), dict(B=0), dict(B=-2), dict(n_w=306479), dict(n_b=667), dict(F_=3071)])
def test_refusals_before_any_launch(kw):
    """on a NULL context, as test_cifar_cpu.py: no impossible argument reaches a launch or a crash"""
    x, lab, g = np.zeros((2, 3072), np.float32), np.zeros(2, np.int32), np.zeros(313867, np.float32)
    w, b = np.zeros(306480, np.float32), np.zeros(666, np.float32)
    a = dict(classes=10, n_w=len(w), n_b=len(b), F_=3072, B=2)
    a.update(kw)
    L = F.lib()
    assert L.fleet_rgbnet_grads(None, a["classes"], w.ctypes.data, a["n_w"], b.ctypes.data, a["n_b"], x.ctypes.data, 2,
                                a["F_"], lab.ctypes.data, None, None, 1, a["B"], 2.0, g.ctypes.data, None,
                                0) == F.FLEET_ERR_ARG
    assert L.fleet_rgbnet_grads_device(None, a["classes"], 1, 307146, 1, None, 1, 2, a["F_"], 1, None, None, 1, a["B"],
                                       2.0, 1, 313867, None, 0, None) == F.FLEET_ERR_ARG
    assert L.fleet_rmodel_rgbnet_grads_device(None, None, 1, 2, 3072, 1, None, None, 1, 2, 2.0, 1, 313867, None, 0,
                                              None) == F.FLEET_ERR_ARG
    with pytest.raises(ValueError):
        K.client_gradients_device(None, 11, None, None, None)
