"""The evaluation's C-ABI without a GPU: the header declares and the library exports its
entry points, NULL handles and impossible arguments are refused before anything is launched,
and the host-only pieces (the group size, the grid cap) answer."""
import ctypes as C

import numpy as np
import pytest

import fleet_amd as F

EVAL = ["fleet_evaluate", "fleet_evaluate_block_images", "fleet_evaluate_device", "fleet_evaluate_set_grid",
        "fleet_model_evaluate", "fleet_rmodel_evaluate", "fleet_rmodel_evaluate_device"]


def test_header_declares_and_library_exports_the_evaluation():
    declared = F.exported_symbols_from_header()
    L = F.lib()
    for s in EVAL:
        assert s in declared, s
        assert hasattr(L, s), s
    assert sorted(s for s in declared if "evaluate" in s) == sorted(EVAL)


def test_block_images_is_a_group_size():
    n = F.lib().fleet_evaluate_block_images()
    assert n >= 1
    assert F.evaluate_block_images() == n


def test_grid_override_is_restored():
    L = F.lib()
    assert L.fleet_evaluate_set_grid(0) == 0
    with F.evaluate_grid_override(3):
        assert L.fleet_evaluate_set_grid(3) == 3
        with F.evaluate_grid_override(1):
            assert L.fleet_evaluate_set_grid(1) == 1
        assert L.fleet_evaluate_set_grid(3) == 3
    assert L.fleet_evaluate_set_grid(0) == 0
    assert L.fleet_evaluate_set_grid(-5) == 0  # a negative cap is the default
    assert L.fleet_evaluate_set_grid(0) == 0


def test_null_handles_are_refused():
    L = F.lib()
    x = np.zeros((2, 784), np.float32)
    lab = np.zeros(2, np.int32)
    w = np.zeros(L.fleet_teacher_weight_count(), np.float32)
    b = np.zeros(L.fleet_teacher_bias_count(), np.float32)
    e, a, c = C.c_float(), C.c_float(), C.c_int32()
    assert L.fleet_evaluate(None, w.ctypes.data, len(w), b.ctypes.data, len(b), x.ctypes.data, 2, 784, lab.ctypes.data,
                            None, 2, C.byref(e), C.byref(a), C.byref(c), None, None) == F.FLEET_ERR_ARG
    assert L.fleet_evaluate_device(None, 1, 1, 1, 2, 784, 1, None, 2, None, None, None, None, 1, None) == F.FLEET_ERR_ARG
    for fn in (L.fleet_model_evaluate, L.fleet_rmodel_evaluate):
        assert fn(None, -1, x.ctypes.data, 2, 784, lab.ctypes.data, None, 2, C.byref(e), C.byref(a), C.byref(c), None,
                  None) == F.FLEET_ERR_ARG
    assert L.fleet_rmodel_evaluate_device(None, -1, 1, 2, 784, 1, None, 2, None, None, 1, None) == F.FLEET_ERR_ARG


def test_python_refuses_mismatched_inputs():
    with pytest.raises(ValueError):
        F._eval_host_args(np.zeros((3, 784), np.float32), np.zeros(2, np.int32), None)
    x, lab, ix, B = F._eval_host_args(np.zeros(784), [5], None)
    assert x.shape == (1, 784) and lab.dtype == np.int32 and ix is None and B == 1
    assert F._eval_host_args(np.zeros((3, 800)), [1, 2, 3], [2, 2, 0, 1])[3] == 4


def test_evaluation_unpacks_as_the_reference_tuple():
    ev = F.Evaluation(np.float32(1.5), np.float32(50), 3, None, None)
    error, accuracy = ev
    assert (error, accuracy, ev.correct) == (1.5, 50.0, 3)
