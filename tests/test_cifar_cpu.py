"""The CIFAR evaluation's C-ABI without a GPU: the header declares and the library exports its
entry points, the vector lengths answer, NULL handles and impossible arguments are refused
before anything is launched, and the grid cap nests and restores."""
import ctypes as C

import numpy as np
import pytest

import fleet_amd as F
from fleet_amd import cifar

CIFAR = ["fleet_cifar_bias_count", "fleet_cifar_block_images", "fleet_cifar_set_grid", "fleet_cifar_test",
         "fleet_cifar_test_device", "fleet_cifar_weight_count", "fleet_model_cifar_test", "fleet_rmodel_cifar_test",
         "fleet_rmodel_cifar_test_device"]


def test_header_declares_and_library_exports_the_entry_points():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in CIFAR:
        assert s in declared, s
        assert hasattr(L, s), s
    assert sorted(s for s in declared if "cifar" in s) == sorted(CIFAR)


def test_counts():
    assert (cifar.weight_count(10), cifar.bias_count(10)) == (306480, 666)
    assert (cifar.weight_count(100), cifar.bias_count(100)) == (323760, 756)
    for classes in (0, 7, 11, 99, 101, -10, 1000):
        assert cifar.weight_count(classes) == 0 and cifar.bias_count(classes) == 0
    assert cifar.weight_count(10) == 432 + 9216 + 221184 + 73728 + 1920
    assert cifar.block_images() >= 1 and cifar.block_images() == F.lib().fleet_cifar_block_images()


def test_grid_override_nests_and_restores():
    L = F.lib()
    assert L.fleet_cifar_set_grid(0) == 0
    with cifar.grid_override(3):
        assert L.fleet_cifar_set_grid(3) == 3
        with cifar.grid_override(1):
            assert L.fleet_cifar_set_grid(1) == 1
        assert L.fleet_cifar_set_grid(3) == 3
    assert L.fleet_cifar_set_grid(0) == 0
    assert L.fleet_cifar_set_grid(-5) == 0  # a negative cap is the default
    assert L.fleet_cifar_set_grid(0) == 0
    assert F.lib().fleet_evaluate_set_grid(0) == 0  # the MNIST evaluation's cap is another


def _host_call(ctx, classes, w, b, x, lab, idx, B):
    e, a, c = C.c_float(), C.c_float(), C.c_int32()
    return F.lib().fleet_cifar_test(ctx, classes, w.ctypes.data, len(w), b.ctypes.data, len(b), x.ctypes.data, x.shape[0],
                                    x.shape[1], lab.ctypes.data, None if idx is None else idx.ctypes.data, B, C.byref(e),
                                    C.byref(a), C.byref(c), None, None, None, None)


def test_null_handles_are_refused():
    L = F.lib()
    x = np.zeros((2, 3072), np.float32)
    lab = np.zeros(2, np.int32)
    w, b = np.zeros(306480, np.float32), np.zeros(666, np.float32)
    e, a, c = C.c_float(), C.c_float(), C.c_int32()
    assert _host_call(None, 10, w, b, x, lab, None, 2) == F.FLEET_ERR_ARG
    assert L.fleet_cifar_test_device(None, 10, 1, 1, 1, 2, 3072, 1, None, 2, None, None, None, None, 1, None) == F.FLEET_ERR_ARG
    for fn in (L.fleet_model_cifar_test, L.fleet_rmodel_cifar_test):
        assert fn(None, -1, x.ctypes.data, 2, 3072, lab.ctypes.data, None, 2, C.byref(e), C.byref(a), C.byref(c), None,
                  None) == F.FLEET_ERR_ARG
    assert L.fleet_rmodel_cifar_test_device(None, -1, 1, 2, 3072, 1, None, 2, None, None, 1, None) == F.FLEET_ERR_ARG


def test_impossible_arguments_are_refused_before_any_launch():
    """Without a device no context exists, so these calls carry a NULL one: what they show is that
    no impossible argument reaches a launch, or a crash, on the way to FLEET_ERR_ARG. The same
    refusals against a live context, each with its message, are in test_gpu_cifar.py."""
    x = np.zeros((2, 3072), np.float32)
    lab = np.zeros(2, np.int32)
    w, b = np.zeros(306480, np.float32), np.zeros(666, np.float32)
    L = F.lib()
    assert _host_call(None, 10, w, b, x[:, :3071].copy(), lab, None, 2) == F.FLEET_ERR_ARG     # F < 3072
    assert _host_call(None, 10, w, b, x, lab, None, 0) == F.FLEET_ERR_ARG                      # B <= 0
    assert _host_call(None, 10, w, b, x, lab, None, -3) == F.FLEET_ERR_ARG
    assert _host_call(None, 7, w, b, x, lab, None, 2) == F.FLEET_ERR_ARG                       # classes 7
    assert _host_call(None, 10, w[:-1], b, x, lab, None, 2) == F.FLEET_ERR_ARG                 # n_w
    assert _host_call(None, 10, w, b[:-1], x, lab, None, 2) == F.FLEET_ERR_ARG                 # n_b
    # the device form: the same refusals come before the context is locked
    for classes, n, Fp, B in ((7, 2, 3072, 2), (10, 2, 3071, 2), (10, 2, 3072, 0), (10, 2, 3072, 3), (10, 0, 3072, 1)):
        assert L.fleet_cifar_test_device(None, classes, 1, 1, 1, n, Fp, 1, None, B, None, None, None, None, 1,
                                         None) == F.FLEET_ERR_ARG


def test_python_refuses_mismatched_inputs():
    with pytest.raises(ValueError):
        cifar.evaluate(None, np.zeros(306480), np.zeros(666), np.zeros((3, 3072), np.float32), np.zeros(2, np.int32))
